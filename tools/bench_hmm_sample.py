"""Posterior sampling against the E-step and Viterbi at the same shapes, in one process:
python tools/bench_hmm_sample.py [--json FILE] [--all-flagged]

Shapes: K = 8, T = 500, B = 2048 (the SLDS configuration) and K = 64, T = 500, B in {64, 512, 2048}; the sampler at
S = 1 and S = 8 samples per sequence.  Every entry point is called through the C ABI on preallocated buffers (no
allocation inside the timed window), timed with device events after warm-up, in 7 windows that alternate between the
four; the median window and the spread are printed.  The sampler's three launches (filter, log-space filter, draw) are then split with the
profiler's kernel times over a few calls: the filter launch is the forward half of the one-directional E-step, so
filter / E-step well above 1/2 is a defect to explain (the E-step at K <= 16 is the two-ended kernel: its chain is T/2).
--all-flagged forbids state 1 at t = 0 (init[1] = -1e4): every sequence leaves the range of the scaled recursions, so the
sampler's filter (and the E-step) redo every sequence in log space -- the cost of the redone route against a run without
the option.  The number of sequences the sampler redid is printed with every shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402
from svae_amd.hmm.hmm_inference import sample_redone_sequences  # noqa: E402

SHAPES = [(8, 500, 2048), (64, 500, 64), (64, 500, 512), (64, 500, 2048)]
SAMPLES = (1, 8)
WINDOWS, MIN_WINDOW_MS = 7, 60.0


def _kernel_split(fn, calls=5):
    """mean device time (ms) per call of the kernels whose names hold `hmm_filter` (the scaled filter, without
    `hmm_filter_log`) / `hmm_filter_log` (the log-space filter launch) / `hmm_draw`, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for key in ("hmm_filter", "hmm_filter_log", "hmm_draw"):
            us = sum(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))
                     for e in prof.key_averages() if key in e.key and (key != "hmm_filter" or "hmm_filter_log" not in e.key))
            out[key] = us / calls / 1e3 if us > 0 else None
        return out
    except Exception as e:                                  # the split is an extra: the windows above stand without it
        print("kernel split unavailable:", repr(e))
        return {"hmm_filter": None, "hmm_filter_log": None, "hmm_draw": None}


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
        if "--all-flagged" in argv:
            init[1] = -1e4
        pair = torch.as_tensor(rng.standard_normal((K, K)), device=dev)
        node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), device=dev)
        SM = max(SAMPLES)
        u = torch.rand(B, SM, T, **f64)
        vws_b = int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K))
        ews_b = int(lib.svae_hmm_workspace_bytes(B, T, K))
        sws_b = int(lib.svae_hmm_sample_workspace_bytes(B, T, K))
        vws = torch.empty(vws_b, dtype=torch.uint8, device=dev)
        ews = torch.empty(ews_b // 8, **f64)
        sws = torch.empty(sws_b // 8, **f64)
        states = torch.empty(B, T, dtype=torch.int32, device=dev)
        sstates = torch.empty(B, SM, T, dtype=torch.int32, device=dev)
        score, logZ, slogZ = torch.empty(B, **f64), torch.empty(B, **f64), torch.empty(B, **f64)
        Ei, Et, Es = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
        stream = _lib.current_stream(dev)

        def viterbi():
            rc = lib.svae_hmm_viterbi_f64(B, T, K, 0, p(init), p(pair), p(node), p(states), p(score), p(vws), vws_b, stream)
            assert rc == 0, rc

        def estep():
            rc = lib.svae_hmm_estep_f64(B, T, K, 0, p(init), p(pair), p(node), p(logZ), p(Ei), p(Et), p(Es), p(ews), ews_b,
                                        stream)
            assert rc == 0, rc

        def sampler(S):
            def run():
                # (the first S samples of every sequence: u and states are addressed as (B,S,T))
                rc = lib.svae_hmm_sample_f64(B, T, K, S, 0, p(init), p(pair), p(node), p(u), p(sstates), p(slogZ), p(sws),
                                             sws_b, stream)
                assert rc == 0, rc
            return run

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        fns = [("viterbi", viterbi), ("estep", estep)] + [("sample_S%d" % S, sampler(S)) for S in SAMPLES]
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
        row = dict(K=K, T=T, B=B, calls_per_window=calls, windows=WINDOWS)
        for name, _ in fns:
            w = sorted(res[name])
            row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = w[len(w) // 2], w[0], w[-1]
        split = _kernel_split(sampler(1))
        row["filter_ms"], row["draw_S1_ms"], row["filter_log_ms"] = split["hmm_filter"], split["hmm_draw"], split["hmm_filter_log"]
        row["sample_redone"] = int(sample_redone_sequences(sws, B, T, K).sum())
        for S in SAMPLES:
            row["ratio_sample_S%d_over_viterbi" % S] = row["sample_S%d_ms" % S] / row["viterbi_ms"]
        row["ratio_filter_over_estep"] = None if row["filter_ms"] is None else row["filter_ms"] / row["estep_ms"]
        rows.append(row)
        print("K=%2d T=%d B=%4d: viterbi %.4f ms [%.4f, %.4f]   E-step %.4f ms [%.4f, %.4f]" % (
            K, T, B, row["viterbi_ms"], row["viterbi_min_ms"], row["viterbi_max_ms"], row["estep_ms"],
            row["estep_min_ms"], row["estep_max_ms"]))
        for S in SAMPLES:
            n = "sample_S%d" % S
            print("    sampler S=%d %.4f ms [%.4f, %.4f]   sampler / viterbi %.3f   (%d of %d sequences redone)" % (
                S, row[n + "_ms"], row[n + "_min_ms"], row[n + "_max_ms"], row["ratio_%s_over_viterbi" % n],
                row["sample_redone"], B))
        if row["filter_ms"] is not None:
            print("    filter launch %.4f ms, log-space filter launch %s ms, draw launch (S=1) %s ms   filter / E-step %.3f   "
                  "(logZ[0] %.6f vs %.6f)" % (
                row["filter_ms"], "%.4f" % row["filter_log_ms"] if row["filter_log_ms"] else "?",
                "%.4f" % row["draw_S1_ms"] if row["draw_S1_ms"] else "?", row["ratio_filter_over_estep"],
                float(slogZ[0]), float(logZ[0])), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
