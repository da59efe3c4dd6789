"""The E-step's derivative against the E-step at the same shapes, in one process:
python tools/bench_hmm_vjp.py [--json FILE]

Shapes of tools/bench_hmm_sample.py: K = 8, T = 500, B = 2048 (the SLDS configuration) and K = 64, T = 500,
B in {64, 512, 2048}.  Timed: the plain E-step and the derivative alone (both through the C ABI on preallocated
buffers), and hmm_estep_differentiable forward and forward plus backward with all four cotangents (the Python layer,
allocations included) -- device events after warm-up, 7 windows that alternate between the four; the median window and
the spread are printed, and the ratio derivative / E-step (the E-step's kernels are those of the commit before this
feature: nothing in them changed)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402
from svae_amd.hmm.hmm_inference import hmm_estep_differentiable, vjp_redone_sequences  # noqa: E402

SHAPES = [(8, 500, 2048), (64, 500, 64), (64, 500, 512), (64, 500, 2048)]
WINDOWS, MIN_WINDOW_MS = 7, 60.0


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
        pair = torch.as_tensor(rng.standard_normal((K, K)), device=dev)
        node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), device=dev)
        g0, g1 = torch.randn(B, **f64), torch.randn(B, K, **f64)
        g2, g3 = torch.randn(B, K, K, **f64), torch.randn(B, T, K, **f64)
        ews_b = int(lib.svae_hmm_workspace_bytes(B, T, K))
        vws_b = int(lib.svae_hmm_estep_vjp_workspace_bytes(B, T, K))
        ews, vws = torch.empty(ews_b // 8, **f64), torch.empty(vws_b // 8, **f64)
        logZ = torch.empty(B, **f64)
        Ei, Et, Es = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
        di, dp, dn = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
        stream = _lib.current_stream(dev)
        ti, tp, tn = (x.clone().requires_grad_() for x in (init, pair, node))

        def estep():
            rc = lib.svae_hmm_estep_f64(B, T, K, 0, p(init), p(pair), p(node), p(logZ), p(Ei), p(Et), p(Es), p(ews), ews_b,
                                        stream)
            assert rc == 0, rc

        def vjp():
            rc = lib.svae_hmm_estep_vjp_f64(B, T, K, 0, p(init), p(pair), p(node), p(g0), p(g1), p(g2), p(g3),
                                            p(di), p(dp), p(dn), p(vws), vws_b, stream)
            assert rc == 0, rc

        def forward():
            with torch.no_grad():
                hmm_estep_differentiable((ti, tp, tn))

        def forward_backward():
            lz, (a, b, c) = hmm_estep_differentiable((ti, tp, tn))
            torch.autograd.backward((lz, a, b, c), (g0, g1, g2, g3))
            ti.grad = tp.grad = tn.grad = None

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        fns = [("estep", estep), ("vjp", vjp), ("forward", forward), ("forward_backward", forward_backward)]
        res, calls = {}, {}
        for name, fn in fns:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once = window(fn, 3)
            calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
            res[name] = []
        for _ in range(WINDOWS):                        # alternate: all four see the same machine
            for name, fn in fns:
                res[name].append(window(fn, calls[name]))
        row = dict(K=K, T=T, B=B, calls_per_window=calls, windows=WINDOWS,
                   redone=int(vjp_redone_sequences(vws, B, T, K).sum()))
        for name, _ in fns:
            w = sorted(res[name])
            row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = w[len(w) // 2], w[0], w[-1]
        row["ratio_vjp_over_estep"] = row["vjp_ms"] / row["estep_ms"]
        row["ratio_forward_backward_over_estep"] = row["forward_backward_ms"] / row["estep_ms"]
        rows.append(row)
        print("K=%2d T=%d B=%4d: E-step %.4f ms [%.4f, %.4f]   derivative %.4f ms [%.4f, %.4f]   derivative / E-step %.2f"
              % (K, T, B, row["estep_ms"], row["estep_min_ms"], row["estep_max_ms"], row["vjp_ms"], row["vjp_min_ms"],
                 row["vjp_max_ms"], row["ratio_vjp_over_estep"]))
        print("    hmm_estep_differentiable: forward %.4f ms [%.4f, %.4f]   forward + backward %.4f ms [%.4f, %.4f]   "
              "(%.2f x E-step; %d sequences redone in log space)"
              % (row["forward_ms"], row["forward_min_ms"], row["forward_max_ms"], row["forward_backward_ms"],
                 row["forward_backward_min_ms"], row["forward_backward_max_ms"], row["ratio_forward_backward_over_estep"],
                 row["redone"]), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
