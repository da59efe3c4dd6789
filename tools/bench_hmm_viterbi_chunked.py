"""The time-chunked Viterbi decoder against the serial one, by sequence length and batch:
   python tools/bench_hmm_viterbi_chunked.py [--out FILE.json] [--K 8 16] [--chunks 32 64 128 256 512] [--shapes B,T ...]
C ABI on preallocated buffers, device events, every shape warmed up, the median of 7 windows that alternate
svae_hmm_viterbi_f64 and svae_hmm_chunked_viterbi_f64 in one process.  Per shape: the serial time and its window spread,
the chunked time and spread at every chunk size and at svae_hmm_chunked_viterbi_default_chunk, whether the chunked labels
equal the serial ones at that size and the largest deviation of the chunked score from the serial one."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402

SHAPES = [(1, 500), (8, 500), (32, 500), (1, 5000), (8, 5000), (32, 5000), (1, 50000), (8, 50000), (32, 50000), (512, 500)]
WINDOWS = 7


def _opt(argv, name, default):
    if name not in argv:
        return default
    i = argv.index(name)
    j = i + 1
    while j < len(argv) and not argv[j].startswith("--"):
        j += 1
    vals = argv[i + 1:j]
    del argv[i:j]
    return vals


def main():
    argv = sys.argv[1:]
    out_path = _opt(argv, "--out", [None])[0]
    Ks = [int(x) for x in _opt(argv, "--K", [8, 16])]
    chunks = [int(x) for x in _opt(argv, "--chunks", [32, 64, 128, 256, 512])]
    shapes = [tuple(int(v) for v in str(x).split(",")) for x in _opt(argv, "--shapes", ["%d,%d" % s for s in SHAPES])]
    dev = torch.device("cuda:0")
    lib, p = _lib.load(), _lib.ptr
    stream = _lib.current_stream(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    rows = []
    for K in Ks:
        for B, T in shapes:
            init = torch.as_tensor(rng.standard_normal(K), **f64)
            pair = torch.as_tensor(rng.standard_normal((K, K)), **f64)
            node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), **f64)
            outs = {name: [torch.empty(B, T, dtype=torch.int32, device=dev), torch.empty(B, **f64)]
                    for name in ("serial", "chunked")}
            default = int(lib.svae_hmm_chunked_viterbi_default_chunk(B, T, K))
            cands = sorted({c for c in chunks if c < T} | ({default} if default < T else set()))
            ws_serial = torch.empty(int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K)) // 8, **f64)
            wsb = {c: int(lib.svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, c)) for c in cands}
            ws_chunked = torch.empty(max(wsb.values()) // 8, **f64)

            def serial():
                rc = lib.svae_hmm_viterbi_f64(B, T, K, 0, p(init), p(pair), p(node), *map(p, outs["serial"]), p(ws_serial),
                                              ws_serial.numel() * 8, stream)
                assert rc == 0, rc

            def chunked(c):
                rc = lib.svae_hmm_chunked_viterbi_f64(B, T, K, 0, c, p(init), p(pair), p(node), *map(p, outs["chunked"]),
                                                      p(ws_chunked), wsb[c], stream)
                assert rc == 0, rc

            arms = [("serial", serial)] + [("chunk %d" % c, lambda c=c: chunked(c)) for c in cands]
            # warm-up, and from it the repetitions that make a window of about 20 ms
            reps = {}
            for name, fn in arms:
                fn(); fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); fn(); e1.record()
                torch.cuda.synchronize()
                reps[name] = int(min(200, max(3, 20.0 / max(e0.elapsed_time(e1) / 2, 1e-3))))
            # correctness at the timed size: labels against the serial ones, the score's deviation
            serial()
            same, dev_max = True, 0.0
            for c in cands:
                chunked(c)
                torch.cuda.synchronize()
                same = same and bool(torch.equal(outs["serial"][0], outs["chunked"][0]))
                dev_max = max(dev_max, float((outs["serial"][1] - outs["chunked"][1]).abs().max()))
            times = {name: [] for name, _ in arms}
            for _ in range(WINDOWS):
                for name, fn in arms:                                   # alternating: one window of each arm per round
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps[name]):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / reps[name])
            med = {name: float(np.median(v)) for name, v in times.items()}
            spread = {name: float((max(v) - min(v)) / np.median(v)) for name, v in times.items()}
            row = dict(K=K, B=B, T=T, default_chunk=default, serial_ms=med["serial"], serial_spread=spread["serial"],
                       chunked_ms={c: med["chunk %d" % c] for c in cands},
                       chunked_spread={c: spread["chunk %d" % c] for c in cands},
                       labels_equal_serial=same, max_abs_score_dev_from_serial=dev_max)
            rows.append(row)
            print("K=%2d B=%3d T=%5d serial %8.3f ms (spread %4.1f %%) | " % (K, B, T, med["serial"], 100 * spread["serial"])
                  + " ".join("L=%d: %.3f (%.0f %%)" % (c, med["chunk %d" % c], 100 * spread["chunk %d" % c]) for c in cands)
                  + " | default %d | labels equal %s | score dev %.1e" % (default, same, dev_max), flush=True)
            if out_path:                                                # (kept up to date: a long run leaves what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "w") as f:
                    json.dump(rows, f, indent=1)
    print(json.dumps(dict(bench="hmm_viterbi_chunked", rows=len(rows))))


if __name__ == "__main__":
    main()
