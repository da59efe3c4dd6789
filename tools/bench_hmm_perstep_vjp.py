"""The derivative of the HMM E-step with per-step transition potentials against that E-step at the same shapes, in one
process:  python tools/bench_hmm_perstep_vjp.py [--json FILE]

Shapes: K = 8, T = 500, B = 2048 and K = 64, T = 500, B = 512, shared (T-1,K,K) and per-sequence (B,T-1,K,K) pair
parameters.  Each runs
  estep            svae_hmm_perstep_estep_f64 with E_trans (the yardstick of every ratio)
  vjp              svae_hmm_perstep_estep_vjp_f64 with all four cotangents and d_pair
  vjp_no_dpair     ... without d_pair (the pair parameters need no gradient)
  vjp_no_gtrans    ... without g_trans (no V_t load, no V tile traffic), with d_pair
  vjp_lean         ... without either
  autograd         forward + backward of hmm_estep_perstep_differentiable on a scalar of all four outputs, all three
                   inputs requiring gradients (this one allocates its outputs inside the timed window, as a training step does)
The C entry points are called on preallocated buffers (no allocation inside the timed window), timed with device events
after warm-up, in 7 windows that alternate between the variants; the median window and the spread are printed with the
ratio to the E-step.  There is no pass/fail threshold.  The expectation from operation counts alone: the derivative has
the E-step's 2 K^2 exponentials per step, plus two K^2 reads of V_t and one K^2 store, so `vjp` should sit within a small
multiple of `estep`."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402
from svae_amd.hmm import hmm_estep_perstep_differentiable  # noqa: E402

SHAPES = [(8, 500, 2048), (64, 500, 512)]
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
        gen = torch.Generator(device=dev).manual_seed(K)
        init = torch.as_tensor(rng.standard_normal(K), device=dev)
        pair_s = torch.as_tensor(rng.standard_normal((T - 1, K, K)), device=dev)
        pair_b = torch.randn(B, T - 1, K, K, generator=gen, **f64)
        node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), device=dev)
        g0, g1 = torch.randn(B, generator=gen, **f64), torch.randn(B, K, generator=gen, **f64)
        g2, g3 = torch.randn(B, T - 1, K, K, generator=gen, **f64), torch.randn(B, T, K, generator=gen, **f64)
        ews_b = int(lib.svae_hmm_perstep_workspace_bytes(B, T, K))
        vws_b = int(lib.svae_hmm_perstep_estep_vjp_workspace_bytes(B, T, K))
        ews, vws = torch.empty(ews_b // 8, **f64), torch.empty(vws_b // 8, **f64)
        logZ, Ei, Es = torch.empty(B, **f64), torch.empty(B, K, **f64), torch.empty(B, T, K, **f64)
        Et = torch.empty(B, T - 1, K, K, **f64)
        di, dn, dp = torch.empty(B, K, **f64), torch.empty(B, T, K, **f64), torch.empty(B, T - 1, K, K, **f64)
        stream = _lib.current_stream(dev)

        def estep(pair, batched):
            def fn():
                rc = lib.svae_hmm_perstep_estep_f64(B, T, K, int(batched), p(init), p(pair), p(node), None, p(logZ), p(Ei),
                                                    p(Et), p(Es), None, p(ews), ews_b, stream)
                assert rc == 0, rc
            return fn

        def vjp(pair, batched, with_gtrans, with_dpair):
            def fn():
                rc = lib.svae_hmm_perstep_estep_vjp_f64(B, T, K, int(batched), p(init), p(pair), p(node), None, p(g0), p(g1),
                                                        p(g2) if with_gtrans else None, p(g3), p(di),
                                                        p(dp) if with_dpair else None, p(dn), None, p(vws), vws_b, stream)
                assert rc == 0, rc
            return fn

        def autograd(pair):
            ti, tp, tn = (x.clone().requires_grad_() for x in (init, pair, node))

            def fn():
                ti.grad = tp.grad = tn.grad = None
                lz, (ei, et, es) = hmm_estep_perstep_differentiable((ti, tp, tn))
                ((lz * g0).sum() + (ei * g1).sum() + (et * g2).sum() + (es * g3).sum()).backward()
            return fn

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        for pname, pair, batched in (("shared", pair_s, False), ("batched", pair_b, True)):
            fns = [("estep", estep(pair, batched)), ("vjp", vjp(pair, batched, True, True)),
                   ("vjp_no_dpair", vjp(pair, batched, True, False)), ("vjp_no_gtrans", vjp(pair, batched, False, True)),
                   ("vjp_lean", vjp(pair, batched, False, False)), ("autograd", autograd(pair))]
            res, calls = {}, {}
            for name, fn in fns:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                once = window(fn, 3)
                calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
                res[name] = []
            for _ in range(WINDOWS):                        # alternate: the variants see the same machine
                for name, fn in fns:
                    res[name].append(window(fn, calls[name]))
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            print("K=%2d T=%d B=%4d pair %-7s  hmm_estep_perstep %.4f ms [%.4f, %.4f]"
                  % (K, T, B, pname, med["estep"], min(res["estep"]), max(res["estep"])), flush=True)
            for name, _ in fns[1:]:
                row = dict(K=K, T=T, B=B, pair=pname, variant=name, windows=WINDOWS, calls_per_window=calls[name],
                           ms=med[name], min_ms=min(res[name]), max_ms=max(res[name]), estep_ms=med["estep"],
                           ratio_to_estep=med[name] / med["estep"])
                rows.append(row)
                print("    %-14s %.4f ms [%.4f, %.4f]  %.2fx the E-step"
                      % (name, row["ms"], row["min_ms"], row["max_ms"], row["ratio_to_estep"]), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
