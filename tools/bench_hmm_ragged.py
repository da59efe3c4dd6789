"""Per-sequence lengths against the uniform HMM calls at the same shapes, in one process:
python tools/bench_hmm_ragged.py [--json FILE]

Shapes: K = 8, T = 500, B = 2048 (DPP-row kernels) and K = 64, T = 500, B = 512 (one wavefront per sequence).  Each shape
runs the ragged E-step and Viterbi with lengths = T and with lengths uniform in [T/2, T], next to the uniform E-step and
Viterbi on the same padded batch.  All four entry points are called through the C ABI on preallocated buffers (no
allocation inside the timed window), timed with device events after warm-up, in windows that alternate between the
four; the median window and the spread are printed with the ragged / uniform ratios.  There is no pass/fail threshold:
for K <= 16 the ragged E-step is the one-directional kernel against the two-ended uniform path, so its ratio at
lengths = T is expected well above 1; for K >= 17 ragged with lengths = T runs the uniform kernel's shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402

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
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = _lib.current_stream(dev)
        for mode in ("full", "half_to_full"):
            lens_h = np.full(B, T) if mode == "full" else rng.integers(T // 2, T + 1, size=B)
            lens = torch.as_tensor(lens_h.astype(np.int32), device=dev)

            def estep_uniform():
                rc = lib.svae_hmm_estep_f64(B, T, K, 0, p(init), p(pair), p(node), p(logZ), p(Ei), p(Et), p(Es), p(ews),
                                            ews_b, stream)
                assert rc == 0, rc

            def estep_ragged():
                rc = lib.svae_hmm_ragged_estep_f64(B, T, K, 0, p(init), p(pair), p(node), p(lens), p(logZ), p(Ei), p(Et),
                                                   p(Es), p(info), p(ews), ews_b, stream)
                assert rc == 0, rc

            def viterbi_uniform():
                rc = lib.svae_hmm_viterbi_f64(B, T, K, 0, p(init), p(pair), p(node), p(states), p(score), p(vws), vws_b,
                                              stream)
                assert rc == 0, rc

            def viterbi_ragged():
                rc = lib.svae_hmm_ragged_viterbi_f64(B, T, K, 0, p(init), p(pair), p(node), p(lens), p(states), p(score),
                                                     p(info), p(vws), vws_b, stream)
                assert rc == 0, rc

            def window(fn, calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / calls

            fns = (("estep_uniform", estep_uniform), ("estep_ragged", estep_ragged),
                   ("viterbi_uniform", viterbi_uniform), ("viterbi_ragged", viterbi_ragged))
            res, calls = {}, {}
            for name, fn in fns:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                once = window(fn, 3)
                calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
                res[name] = []
            for _ in range(WINDOWS):                        # alternate: the four see the same machine
                for name, fn in fns:
                    res[name].append(window(fn, calls[name]))
            assert int(info.item()) == 0
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            row = dict(K=K, T=T, B=B, lengths=mode, mean_length=float(lens_h.mean()), windows=WINDOWS, calls_per_window=calls,
                       estep_ratio=med["estep_ragged"] / med["estep_uniform"],
                       viterbi_ratio=med["viterbi_ragged"] / med["viterbi_uniform"])
            for k, v in res.items():
                row[k + "_ms"], row[k + "_min_ms"], row[k + "_max_ms"] = med[k], min(v), max(v)
            rows.append(row)
            print("K=%2d T=%d B=%4d lengths %-12s (mean %.0f): E-step uniform %.4f ms [%.4f, %.4f]  ragged %.4f ms [%.4f, %.4f]  "
                  "ratio %.3f | Viterbi uniform %.4f ms [%.4f, %.4f]  ragged %.4f ms [%.4f, %.4f]  ratio %.3f"
                  % (K, T, B, mode, lens_h.mean(),
                     med["estep_uniform"], min(res["estep_uniform"]), max(res["estep_uniform"]),
                     med["estep_ragged"], min(res["estep_ragged"]), max(res["estep_ragged"]), row["estep_ratio"],
                     med["viterbi_uniform"], min(res["viterbi_uniform"]), max(res["viterbi_uniform"]),
                     med["viterbi_ragged"], min(res["viterbi_ragged"]), max(res["viterbi_ragged"]), row["viterbi_ratio"]),
                  flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
