"""Timing of the LDS E-step and of the training pass (inference + VJP) on a batch of sequences of different lengths
(`lengths=`, svae_lds_ragged_*) next to the existing uniform path at the same B and T, both in one process.
Usage: python tools/bench_ragged.py [B T n S] [--reps R]
Without a shape: 512 and 4096 sequences of T = 200, n = 10, S = 1 (the headline shapes).  Three inputs per shape: the uniform
call (no lengths: unchanged code), the ragged call with all lengths = T, and the ragged call with lengths uniform in
[T/2, T].  Device events around `reps` back-to-back calls after a warm-up of 3; the median of 5 alternating windows.
The ragged calls take the packed one-directional kernels at every batch size, the uniform ones the
dispatcher's choice for the shape (two-ended / producer / lean kernels): the ratio is the price of the route as well as of
the per-step parameter loads and the masks."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def run(B, T, n, S, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    (J0, h0, z0), pair = rand_lds_natparam(n, rng)
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev).contiguous()
    params = (t(J0), t(h0), t(z0).reshape(1), t(pair[0]), t(pair[1]), t(pair[2]), t(pair[3]).reshape(1))
    nJ, nh = (t(x) for x in rand_node_potentials((B, T, n), rng))
    eps = torch.randn(B, T, S, n, dtype=torch.float64, device=dev)
    g = [torch.randn(B, dtype=torch.float64, device=dev), torch.randn(B, T, n, dtype=torch.float64, device=dev),
         torch.randn(B, T, n, dtype=torch.float64, device=dev), torch.randn(B, T, S, n, dtype=torch.float64, device=dev)]
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    half = torch.as_tensor(rng.integers(T // 2, T + 1, size=B), dtype=torch.int32, device=dev)
    plans = {k: LDSEStepPlan(B, T, n, dev) for k in ("uniform", "ragged, lengths = T", "ragged, lengths in [T/2, T]")}
    lens = {"uniform": None, "ragged, lengths = T": full, "ragged, lengths in [T/2, T]": half}

    def estep(k):
        return lambda: plans[k].launch(*params, nJ, nh, None, lengths=lens[k])

    def train(k):
        def fn():
            smp = plans[k].infer(*params, nJ, nh, None, eps=eps, lengths=lens[k])
            plans[k].vjp(g[0], g[1], g[2], g[3], eps, smp)
        return fn
    for name, make in (("E-step", estep), ("inference + VJP", train)):
        fns = {k: make(k) for k in plans}
        for fn in fns.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in plans}
        for _ in range(5):                      # alternating windows
            for k, fn in fns.items():
                times[k].append(window(fn, reps))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in plans:
            print("B=%d T=%d n=%d S=%d %-16s %-28s %.3f ms [%.3f .. %.3f] | ratio to uniform %.2f"
                  % (B, T, n, S, name, k, med[k], min(times[k]), max(times[k]), med[k] / med["uniform"]))
    for p in plans.values():
        p.check_info()


def main():
    argv = sys.argv[1:]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 20
    if len(argv) >= 4 and not argv[0].startswith("--"):
        shapes = [tuple(int(x) for x in argv[:4])]
    else:
        shapes = [(512, 200, 10, 1), (4096, 200, 10, 1)]
    for B, T, n, S in shapes:
        run(B, T, n, S, reps)


if __name__ == "__main__":
    main()
