"""Viterbi decoding against the E-step at the same shapes, in one process: python tools/bench_hmm_viterbi.py [--json FILE]

Shapes: K = 8, T = 500, B = 2048 (the SLDS configuration) and K = 64, T = 500, B in {64, 512, 2048}.  Both entry points
are called through the C ABI on preallocated buffers (no allocation inside the timed window), timed with device events
after warm-up, in windows that alternate between the two; the median window and the spread are printed.  Viterbi does a
forward pass of adds and compares where the E-step does forward and backward passes of multiply-adds: a ratio above 1
is a defect to explain."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402

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
        vws_b = int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K))
        ews_b = int(lib.svae_hmm_workspace_bytes(B, T, K))
        vws = torch.empty(vws_b, dtype=torch.uint8, device=dev)
        ews = torch.empty(ews_b // 8, **f64)
        states = torch.empty(B, T, dtype=torch.int32, device=dev)
        score, logZ = torch.empty(B, **f64), torch.empty(B, **f64)
        Ei, Et, Es = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
        stream = _lib.current_stream(dev)

        def viterbi():
            rc = lib.svae_hmm_viterbi_f64(B, T, K, 0, p(init), p(pair), p(node), p(states), p(score), p(vws), vws_b, stream)
            assert rc == 0, rc

        def estep():
            rc = lib.svae_hmm_estep_f64(B, T, K, 0, p(init), p(pair), p(node), p(logZ), p(Ei), p(Et), p(Es), p(ews), ews_b,
                                        stream)
            assert rc == 0, rc

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        res = {}
        calls = {}
        for name, fn in (("viterbi", viterbi), ("estep", estep)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once = window(fn, 3)
            calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
            res[name] = []
        for _ in range(WINDOWS):                        # alternate: the two see the same machine
            for name, fn in (("viterbi", viterbi), ("estep", estep)):
                res[name].append(window(fn, calls[name]))
        v, e = (sorted(res[k]) for k in ("viterbi", "estep"))
        vm, em = v[len(v) // 2], e[len(e) // 2]
        row = dict(K=K, T=T, B=B, viterbi_ms=vm, viterbi_min_ms=v[0], viterbi_max_ms=v[-1], estep_ms=em, estep_min_ms=e[0],
                   estep_max_ms=e[-1], ratio=vm / em, calls_per_window=calls, windows=WINDOWS,
                   node_GB_per_s_viterbi=8.0 * B * T * K / (vm * 1e-3) / 1e9)
        rows.append(row)
        print("K=%2d T=%d B=%4d: viterbi %.4f ms [%.4f, %.4f]   E-step %.4f ms [%.4f, %.4f]   ratio %.3f   "
              "(score[0] %.6f, logZ[0] %.6f)" % (K, T, B, vm, v[0], v[-1], em, e[0], e[-1], vm / em, float(score[0]),
                                                 float(logZ[0])), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
