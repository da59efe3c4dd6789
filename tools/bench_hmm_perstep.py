"""The HMM E-step with per-step transition potentials against the uniform E-step at the same shapes, in one process:
python tools/bench_hmm_perstep.py [--json FILE]

Shapes: K = 8, T = 500, B = 2048 and K = 64, T = 500, B = 512.  Each shape runs svae_hmm_perstep_estep_f64 with shared
(T-1,K,K) and per-sequence (B,T-1,K,K) pair parameters, with and without E_trans, next to svae_hmm_estep_f64 on the same
node potentials.  All entry points are called through the C ABI on preallocated buffers (no allocation inside the timed
window), timed with device events after warm-up, in 7 windows that alternate between the five; the median window and the
spread are printed with the ratio to the uniform E-step and the ALGORITHMIC bytes of the call -- the pair parameters
read (once per sequence when per-sequence, once in all when shared), E_trans written, the node potentials read and
E_states written -- against the time those bytes take at the HBM rate of bench.py's roofline.  (The kernel's own
workspace traffic, B T K doubles written and read, is not algorithmic and not counted.)  There is no pass/fail threshold:
the per-step kernel pays 2 K^2 exponentials per step that the uniform kernels pay once per sequence."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import HBM_PEAK_GBPS  # noqa: E402  (read-only)
from svae_amd import _lib  # noqa: E402

SHAPES = [(8, 500, 2048), (64, 500, 512)]
WINDOWS, MIN_WINDOW_MS = 7, 60.0


def algorithmic_bytes(B, T, K, pair_batched, want_trans):
    pair = (B if pair_batched else 1) * (T - 1) * K * K
    trans = B * (T - 1) * K * K if want_trans else 0
    node = 2 * B * T * K                                    # node potentials read, E_states written
    return 8 * (pair + trans + node)


def main(argv):
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no fallback"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = _lib.ptr
    rng = np.random.default_rng(0)
    rows = []
    for K, T, B in SHAPES:
        f64 = dict(dtype=torch.float64, device=dev)
        init = torch.as_tensor(rng.standard_normal(K), device=dev)
        pair_u = torch.as_tensor(rng.standard_normal((K, K)), device=dev)
        pair_s = torch.as_tensor(rng.standard_normal((T - 1, K, K)), device=dev)
        pair_b = torch.randn(B, T - 1, K, K, generator=torch.Generator(device=dev).manual_seed(K), **f64)
        node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), device=dev)
        uws_b = int(lib.svae_hmm_workspace_bytes(B, T, K))
        pws_b = int(lib.svae_hmm_perstep_workspace_bytes(B, T, K))
        uws, pws = torch.empty(uws_b // 8, **f64), torch.empty(pws_b // 8, **f64)
        logZ, Ei, Es = torch.empty(B, **f64), torch.empty(B, K, **f64), torch.empty(B, T, K, **f64)
        Et_u, Et_p = torch.empty(B, K, K, **f64), torch.empty(B, T - 1, K, K, **f64)
        stream = _lib.current_stream(dev)

        def uniform():
            rc = lib.svae_hmm_estep_f64(B, T, K, 0, p(init), p(pair_u), p(node), p(logZ), p(Ei), p(Et_u), p(Es), p(uws),
                                        uws_b, stream)
            assert rc == 0, rc

        def perstep(pair, batched, want):
            def fn():
                rc = lib.svae_hmm_perstep_estep_f64(B, T, K, int(batched), p(init), p(pair), p(node), None, p(logZ), p(Ei),
                                                    p(Et_p) if want else None, p(Es), None, p(pws), pws_b, stream)
                assert rc == 0, rc
            return fn

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        variants = (("shared", False, True), ("shared_no_trans", False, False),
                    ("batched", True, True), ("batched_no_trans", True, False))
        fns = [("uniform", uniform)] + [(name, perstep(pair_b if batched else pair_s, batched, want))
                                        for name, batched, want in variants]
        res, calls = {}, {}
        for name, fn in fns:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once = window(fn, 3)
            calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
            res[name] = []
        for _ in range(WINDOWS):                            # alternate: the five see the same machine
            for name, fn in fns:
                res[name].append(window(fn, calls[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        print("K=%2d T=%d B=%4d  uniform hmm_estep %.4f ms [%.4f, %.4f]"
              % (K, T, B, med["uniform"], min(res["uniform"]), max(res["uniform"])), flush=True)
        for name, batched, want in variants:
            nbytes = algorithmic_bytes(B, T, K, batched, want)
            hbm_ms = nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3
            row = dict(K=K, T=T, B=B, variant=name, pair_batched=batched, want_trans=want, windows=WINDOWS,
                       calls_per_window=calls[name], ms=med[name], min_ms=min(res[name]), max_ms=max(res[name]),
                       uniform_ms=med["uniform"], ratio_to_uniform=med[name] / med["uniform"],
                       algorithmic_bytes=nbytes, hbm_peak_GBps=HBM_PEAK_GBPS, hbm_ms=hbm_ms,
                       ratio_to_hbm=med[name] / hbm_ms)
            rows.append(row)
            print("    per-step %-17s %.4f ms [%.4f, %.4f]  %.1fx uniform | %.1f MB algorithmic = %.4f ms at %.0f GB/s: "
                  "%.1fx that" % (name, row["ms"], row["min_ms"], row["max_ms"], row["ratio_to_uniform"], nbytes / 1e6,
                                  hbm_ms, HBM_PEAK_GBPS, row["ratio_to_hbm"]), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
