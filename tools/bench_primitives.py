"""Times the reverse-mode primitives of svae_amd/lds/cython_lds_inference.py -- each *_grad alone and the composed
filter + smoother + sampler backward -- against the fused VJP (lds_inference_differentiable backward, which runs
svae_lds_estep_vjp_ex_f64) at the same shape.  Device events, warm-up; one JSON line.

    python tools/bench_primitives.py [--B 512 4096] [--T 200] [--n 10] [--S 1] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd.lds import cython_lds_inference as P  # noqa: E402
from svae_amd.lds.lds_inference import lds_inference_differentiable  # noqa: E402
from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials  # noqa: E402


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def one(B, T, n, S, reps):
    rng = np.random.default_rng(0)
    init, pair = rand_lds_natparam(n, rng)
    node = [torch.as_tensor(x).cuda() for x in rand_node_potentials((B, T, n), rng)]
    eps = torch.randn(B, T, S, n, dtype=torch.float64, device="cuda")
    cot = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda")
    (msgs, lognorm), fi = P.natural_filter_forward_general(init, pair, node)
    _, si = P.natural_smoother_general(msgs, pair)
    _, qi = P.natural_sample_backward(msgs, pair, S, eps=eps)
    g_f = (((cot(B, T, n, n), cot(B, T, n)), (cot(B, T, n, n), cot(B, T, n))), cot(B))
    g_s = ((None, None, 1., 1.), None, (cot(B, T, n), cot(B, T, n), None))
    g_q = cot(B, T, S, n)
    gd, gx, gl = cot(B, T, n), cot(B, T, n), cot(B)
    out = dict(B=B, T=T, n=n, S=S)
    out["filter_grad_ms"] = _time(lambda: P.natural_filter_grad(g_f, fi), reps)
    out["smoother_grad_ms"] = _time(lambda: P.natural_smoother_general_grad(g_s, si), reps)
    out["sample_grad_ms"] = _time(lambda: P.natural_sample_backward_grad(g_q, qi), reps)

    def composed():
        J, h = (x.clone().requires_grad_(True) for x in node)
        m, ln = P.filter_forward_differentiable(init, pair, (J, h))
        _, _, En = P.smoother_differentiable(m, pair)
        smp = P.sample_backward_differentiable(m, pair, S, eps=eps)
        ((ln * gl).sum() + (En[0] * gd).sum() + (En[1] * gx).sum() + (smp * g_q).sum()).backward()

    def fused():
        J, h = (x.clone().requires_grad_(True) for x in node)
        ln, (dxx, x), smp, _ = lds_inference_differentiable((init, pair), (J, h), eps=eps)
        ((ln * gl).sum() + (dxx * gd).sum() + (x * gx).sum() + (smp * g_q).sum()).backward()
    out["composed_fwd_bwd_ms"] = _time(composed, reps)
    out["fused_fwd_bwd_ms"] = _time(fused, reps)
    out["composed_over_fused"] = out["composed_fwd_bwd_ms"] / out["fused_fwd_bwd_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--S", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print(json.dumps({"bench_primitives": [one(B, a.T, a.n, a.S, a.reps) for B in a.B]}))


if __name__ == "__main__":
    main()
