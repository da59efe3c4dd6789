"""Viterbi decoding and posterior sampling with per-step transition potentials next to the per-step E-step and the uniform
Viterbi / sampler at the same shapes, in one process:  python tools/bench_hmm_perstep_decode.py [--json FILE]

Shapes: K = 8, T = 500, B = 2048 and K = 64, T = 500, B = 512, each with shared (T-1,K,K) and per-sequence (B,T-1,K,K)
pair parameters.  Timed per shape and pair layout: svae_hmm_perstep_viterbi_f64, svae_hmm_perstep_sample_f64 at S = 1 and
S = 8, svae_hmm_perstep_estep_f64 without E_trans (hmm_estep_perstep(want_trans=False)); per shape the uniform
svae_hmm_viterbi_f64 and svae_hmm_sample_f64 (S = 1, S = 8) on the same node potentials.  All entry points are called
through the C ABI on preallocated buffers (no allocation inside the timed window), timed with device events after
warm-up, in 7 windows that alternate between all of a shape's calls; the median window and the spread are printed with
the ratio to the per-step E-step without E_trans and the ALGORITHMIC bytes of the call -- the pair parameters read (once
per sequence when per-sequence, once in all when shared), the node potentials read, the uniforms read and the labels
written -- against the time those bytes take at the HBM rate of bench.py's roofline (workspace traffic is not algorithmic
and not counted).  The sampler's filter launch has no entry of its own in the C ABI and is not timed alone.  There is no
pass/fail threshold."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import HBM_PEAK_GBPS  # noqa: E402  (read-only)
from svae_amd import _lib  # noqa: E402

SHAPES = [(8, 500, 2048), (64, 500, 512)]
WINDOWS, MIN_WINDOW_MS = 7, 40.0
SMAX = 8


def algorithmic_bytes(B, T, K, pair_batched, op, S=0):
    pair = 8 * (B if pair_batched else 1) * (T - 1) * K * K
    node = 8 * B * T * K
    if op == "viterbi":
        return pair + node + 4 * B * T
    if op == "sample":
        return pair + node + (8 + 4) * B * S * T
    return pair + 2 * node                                  # E-step without E_trans: E_states written


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
        u = torch.rand(B, SMAX, T, generator=torch.Generator(device=dev).manual_seed(K + 1), **f64)
        pws_b = int(lib.svae_hmm_perstep_workspace_bytes(B, T, K))
        vws_b = int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K))
        sws_b = int(lib.svae_hmm_sample_workspace_bytes(B, T, K))
        pws, sws = torch.empty(pws_b // 8, **f64), torch.empty(sws_b // 8, **f64)
        vws = torch.empty(vws_b, dtype=torch.uint8, device=dev)
        logZ, Ei, Es = torch.empty(B, **f64), torch.empty(B, K, **f64), torch.empty(B, T, K, **f64)
        labels = torch.empty(B, T, dtype=torch.int32, device=dev)
        states = torch.empty(B, SMAX, T, dtype=torch.int32, device=dev)
        score = torch.empty(B, **f64)
        stream = _lib.current_stream(dev)

        def checked(call):
            def fn():
                rc = call()
                assert rc == 0, rc
            return fn

        def ps_viterbi(pair, pb):
            return checked(lambda: lib.svae_hmm_perstep_viterbi_f64(B, T, K, pb, p(init), p(pair), p(node), None, p(labels),
                                                                    p(score), None, p(vws), vws_b, stream))

        def ps_sample(pair, pb, S):
            us = u[:, :S].contiguous()
            return checked(lambda: lib.svae_hmm_perstep_sample_f64(B, T, K, S, pb, p(init), p(pair), p(node), None, p(us),
                                                                   p(states), p(logZ), None, p(pws), pws_b, stream))

        def ps_estep(pair, pb):
            return checked(lambda: lib.svae_hmm_perstep_estep_f64(B, T, K, pb, p(init), p(pair), p(node), None, p(logZ),
                                                                  p(Ei), None, p(Es), None, p(pws), pws_b, stream))

        def un_sample(S):
            us = u[:, :S].contiguous()
            return checked(lambda: lib.svae_hmm_sample_f64(B, T, K, S, 0, p(init), p(pair_u), p(node), p(us), p(states),
                                                           p(logZ), p(sws), sws_b, stream))

        un_viterbi = checked(lambda: lib.svae_hmm_viterbi_f64(B, T, K, 0, p(init), p(pair_u), p(node), p(labels), p(score),
                                                              p(vws), vws_b, stream))

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        fns = [("uniform_viterbi", un_viterbi), ("uniform_sample_S1", un_sample(1)), ("uniform_sample_S8", un_sample(8))]
        meta = {}
        for layout, pair, pb in (("shared", pair_s, 0), ("batched", pair_b, 1)):
            for op, S, fn in (("estep_no_trans", 0, ps_estep(pair, pb)), ("viterbi", 0, ps_viterbi(pair, pb)),
                              ("sample", 1, ps_sample(pair, pb, 1)), ("sample", 8, ps_sample(pair, pb, 8))):
                name = "%s_%s%s" % (layout, op, "_S%d" % S if S else "")
                fns.append((name, fn))
                meta[name] = (layout, bool(pb), op, S)
        res, calls = {}, {}
        for name, fn in fns:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            once = window(fn, 3)
            calls[name] = max(5, int(MIN_WINDOW_MS / max(once, 1e-3)))
            res[name] = []
        for _ in range(WINDOWS):                            # alternate: all see the same machine
            for name, fn in fns:
                res[name].append(window(fn, calls[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        print("K=%2d T=%d B=%4d  uniform: hmm_viterbi %.4f ms, hmm_sample S=1 %.4f ms, S=8 %.4f ms"
              % (K, T, B, med["uniform_viterbi"], med["uniform_sample_S1"], med["uniform_sample_S8"]), flush=True)
        for name, (layout, pb, op, S) in meta.items():
            nbytes = algorithmic_bytes(B, T, K, pb, op, S)
            hbm_ms = nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3
            estep = med["%s_estep_no_trans" % layout]
            uniform = {"viterbi": med["uniform_viterbi"], "sample": med.get("uniform_sample_S%d" % S)}.get(op)
            row = dict(K=K, T=T, B=B, variant=name, pair_batched=pb, op=op, S=S, windows=WINDOWS,
                       calls_per_window=calls[name], ms=med[name], min_ms=min(res[name]), max_ms=max(res[name]),
                       estep_no_trans_ms=estep, ratio_to_estep_no_trans=med[name] / estep, uniform_ms=uniform,
                       ratio_to_uniform=None if uniform is None else med[name] / uniform,
                       algorithmic_bytes=nbytes, hbm_peak_GBps=HBM_PEAK_GBPS, hbm_ms=hbm_ms, ratio_to_hbm=med[name] / hbm_ms)
            rows.append(row)
            print("    %-26s %.4f ms [%.4f, %.4f]  %.2fx E-step without E_trans%s | %.1f MB algorithmic = %.4f ms at "
                  "%.0f GB/s: %.1fx that"
                  % (name, row["ms"], row["min_ms"], row["max_ms"], row["ratio_to_estep_no_trans"],
                     "" if uniform is None else ", %.2fx uniform" % row["ratio_to_uniform"], nbytes / 1e6, hbm_ms,
                     HBM_PEAK_GBPS, row["ratio_to_hbm"]), flush=True)
    if "--json" in argv:
        path = argv[argv.index("--json") + 1]
        with open(path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
