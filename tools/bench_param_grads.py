"""Timing of the LDS VJP with and without the gradients of the natural parameters (svae_lds_estep_vjp_params_f64 vs
svae_lds_estep_vjp_ex_f64), both in one process on the full records of the same forward pass.
Usage: python tools/bench_param_grads.py [B T n S] [--layout homog|step|batched] [--reps R]
Without a shape: 512 and 4096 sequences of T = 200, n = 10, S = 1 (the headline shapes).  Device events around `reps`
back-to-back calls after a warm-up of 3; the median of 5 such windows."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402
from svae_amd.lds.lds_inference import LDSEStepPlan  # noqa: E402
from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials  # noqa: E402


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run(B, T, n, S, layout, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    (J0, h0, z0), pair = rand_lds_natparam(n, rng)
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev).contiguous()
    lead = {"homog": (), "step": (T - 1,), "batched": (B, T - 1)}[layout]
    pair = [t(x).expand(*lead, *np.shape(x)).contiguous() if lead else t(x) for x in pair]
    pair[3] = pair[3].reshape(-1)
    nJ, nh = rand_node_potentials((B, T, n), rng)
    eps = torch.randn(B, T, max(S, 1), n, dtype=torch.float64, device=dev)
    g = [torch.randn(B, dtype=torch.float64, device=dev), torch.randn(B, T, n, dtype=torch.float64, device=dev),
         torch.randn(B, T, n, dtype=torch.float64, device=dev), torch.randn(B, T, max(S, 1), n, dtype=torch.float64, device=dev)]
    plan = LDSEStepPlan(B, T, n, dev, layout != "homog", layout == "batched", options=_lib.OPT_LEAN_OFF)
    plan.launch(t(J0), t(h0), t(z0).reshape(1), *pair, t(nJ), t(nh), None, layout == "batched", True, True)
    smp = plan.sample(eps) if S > 0 else None
    sc = (g[3], eps, smp) if S > 0 else (None, None, None)
    plain = lambda: plan.vjp(g[0], g[1], g[2], *sc)
    params = lambda: plan.vjp(g[0], g[1], g[2], *sc, param_out=True)
    a, b = plain(), params()
    same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for _ in range(3):
        plain(), params()
    tp, tq = [], []
    for _ in range(5):                      # alternating windows
        tp.append(window(plain, reps))
        tq.append(window(params, reps))
    mp, mq = float(np.median(tp)), float(np.median(tq))
    print("B=%d T=%d n=%d S=%d %s (full records): VJP %.3f ms [%.3f .. %.3f] | VJP + parameter gradients %.3f ms "
          "[%.3f .. %.3f] | ratio %.2f | node gradients bit-identical: %s | extra scratch %.1f MB"
          % (B, T, n, S, layout, mp, min(tp), max(tp), mq, min(tq), max(tq), mq / mp, same, plan.param_ws_bytes / 1e6))


def main():
    argv = sys.argv[1:]
    layout = argv[argv.index("--layout") + 1] if "--layout" in argv else "homog"
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 20
    if len(argv) >= 4 and not argv[0].startswith("--"):
        shapes = [tuple(int(x) for x in argv[:4])]
    else:
        shapes = [(512, 200, 10, 1), (4096, 200, 10, 1)]
    for B, T, n, S in shapes:
        run(B, T, n, S, layout, reps)


if __name__ == "__main__":
    main()
