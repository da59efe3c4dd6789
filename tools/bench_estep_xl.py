"""Timing of the LDS E-step for latent dimensions 65..128 (svae_amd/csrc/lds_estep_xl.hip): `plan.launch` at
n in {80, 96, 128}, T = 200, B in {256, 512} on the rotation model, in ms per E-step and algorithmic TFLOP/s
(bench.algorithmic_flops_per_seq against bench.FP64_MFMA_PEAK_TFLOPS).  With --ref, also one sequence of the reference's
compiled E-step (oracle/_ref) on the host, for scale.
Usage: python tools/bench_estep_xl.py [--reps 5] [--ref] [--n 128] [--B 512]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import FP64_MFMA_PEAK_TFLOPS, algorithmic_flops_per_seq   # noqa: E402  (read-only)
from svae_amd.lds.lds_inference import LDSEStepPlan                    # noqa: E402
from svae_amd.lds.synthetic_data import rand_node_potentials, rotation_lds_natparam  # noqa: E402

DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--n", type=int, nargs="*", default=[80, 96, 128])
    ap.add_argument("--B", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--ref", action="store_true", help="also time one sequence of oracle/_ref (the reference, CPU)")
    args = ap.parse_args()
    T = args.T
    for n in args.n:
        rng = np.random.default_rng(n)
        (J0, h0, z0), (J11, J12, J22, zp) = rotation_lds_natparam(n, rng)
        t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=DEV).contiguous()
        params = (t(J0), t(h0), t([z0]), t(J11), t(J12), t(J22), t([zp]))
        for B in args.B:
            nJ, nh = rand_node_potentials((B, T, n), rng)
            plan = LDSEStepPlan(B, T, n, DEV)
            nodeJ, nodeh = t(nJ), t(nh)
            go = lambda: plan.launch(*params, nodeJ, nodeh)
            go()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.reps):
                go()
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / args.reps
            tf = B * algorithmic_flops_per_seq(T, n) / (ms * 1e-3) / 1e12
            print(json.dumps({"n": n, "T": T, "B": B, "ms_per_estep": round(ms, 3), "algorithmic_tflops": round(tf, 2),
                              "frac_fp64_mfma_peak": round(tf / FP64_MFMA_PEAK_TFLOPS, 3),
                              "workspace_gb": round(plan.ws_bytes / 1e9, 2)}), flush=True)
            del plan
            torch.cuda.empty_cache()
        if args.ref:
            from oracle import ref
            if ref.available():
                node = rand_node_potentials((T, n), rng)
                t0 = time.perf_counter()
                ref.estep(((J0, h0, z0), (J11, J12, J22, zp)), (node[0], node[1], np.zeros(T)))
                print(json.dumps({"n": n, "T": T, "reference_cpu_ms_per_sequence": round(1e3 * (time.perf_counter() - t0), 1)}),
                      flush=True)


if __name__ == "__main__":
    main()
