"""The time-chunked posterior sampler against the serial one, by sequence length, batch and samples per sequence:
   python tools/bench_hmm_sample_chunked.py [--out FILE.json] [--K 8 16] [--S 1 8] [--chunks 32 64 128 256 512]
                                            [--shapes B,T ...]
C ABI on preallocated buffers, device events, every shape warmed up, the median of 7 windows that alternate
svae_hmm_sample_f64 and svae_hmm_chunked_sample_f64 in one process.  Per shape: the serial time and its window spread, the
chunked time and spread at every chunk size and at svae_hmm_chunked_sample_default_chunk, and the largest deviation of the
chunked log Z from the serial one.  The chunked labels must equal the serial ones (same uniforms) at every size: asserted."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib  # noqa: E402

SHAPES = [(1, 500), (8, 500), (32, 500), (128, 500), (512, 500), (1, 5000), (8, 5000), (32, 5000), (128, 5000), (1, 50000),
          (8, 50000), (32, 50000)]
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
    Ss = [int(x) for x in _opt(argv, "--S", [1, 8])]
    chunks = [int(x) for x in _opt(argv, "--chunks", [32, 64, 128, 256, 512])]
    shapes = [tuple(int(v) for v in str(x).split(",")) for x in _opt(argv, "--shapes", ["%d,%d" % s for s in SHAPES])]
    dev = torch.device("cuda:0")
    lib, p = _lib.load(), _lib.ptr
    stream = _lib.current_stream(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    rows = []
    for K, S in [(K, S) for K in Ks for S in Ss]:
        for B, T in shapes:
            init = torch.as_tensor(rng.standard_normal(K), **f64)
            pair = torch.as_tensor(rng.standard_normal((K, K)), **f64)
            node = torch.as_tensor(3.0 * rng.standard_normal((B, T, K)), **f64)
            u = torch.as_tensor(rng.random((B, S, T)), **f64)
            outs = {name: [torch.empty(B, S, T, dtype=torch.int32, device=dev), torch.empty(B, **f64)]
                    for name in ("serial", "chunked")}
            default = int(lib.svae_hmm_chunked_sample_default_chunk(B, T, K, S))
            cands = sorted({c for c in chunks if c < T} | ({default} if default < T else set()))
            ws_serial = torch.empty(int(lib.svae_hmm_sample_workspace_bytes(B, T, K)) // 8, **f64)
            wsb = {c: int(lib.svae_hmm_chunked_sample_workspace_bytes(B, T, K, S, c)) for c in cands}
            ws_chunked = torch.empty(max(wsb.values()) // 8, **f64)
            if not cands:
                continue

            def serial():
                rc = lib.svae_hmm_sample_f64(B, T, K, S, 0, p(init), p(pair), p(node), p(u), *map(p, outs["serial"]),
                                             p(ws_serial), ws_serial.numel() * 8, stream)
                assert rc == 0, rc

            def chunked(c):
                rc = lib.svae_hmm_chunked_sample_f64(B, T, K, S, 0, c, p(init), p(pair), p(node), p(u),
                                                     *map(p, outs["chunked"]), p(ws_chunked), wsb[c], stream)
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
            # correctness at the timed size: labels equal to the serial ones (asserted), log Z's deviation
            serial()
            same, dev_max = True, 0.0
            for c in cands:
                chunked(c)
                torch.cuda.synchronize()
                same = same and bool(torch.equal(outs["serial"][0], outs["chunked"][0]))
                assert same, "chunked labels differ from the serial ones at K=%d S=%d B=%d T=%d chunk=%d" % (K, S, B, T, c)
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
            row = dict(K=K, S=S, B=B, T=T, default_chunk=default, serial_ms=med["serial"], serial_spread=spread["serial"],
                       chunked_ms={c: med["chunk %d" % c] for c in cands},
                       chunked_spread={c: spread["chunk %d" % c] for c in cands},
                       labels_equal_serial=same, max_abs_logZ_dev_from_serial=dev_max)
            rows.append(row)
            print("K=%2d S=%d B=%3d T=%5d serial %8.3f ms (spread %4.1f %%) | " % (K, S, B, T, med["serial"], 100 * spread["serial"])
                  + " ".join("L=%d: %.3f (%.0f %%)" % (c, med["chunk %d" % c], 100 * spread["chunk %d" % c]) for c in cands)
                  + " | default %d | labels equal %s | logZ dev %.1e" % (default, same, dev_max), flush=True)
            if out_path:                                                # (kept up to date: a long run leaves what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "w") as f:
                    json.dump(rows, f, indent=1)
    print(json.dumps(dict(bench="hmm_sample_chunked", rows=len(rows))))


if __name__ == "__main__":
    main()
