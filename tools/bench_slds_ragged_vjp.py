"""The training path of the ragged SLDS against the uniform one at the same shape, in one process:
python tools/bench_slds_ragged_vjp.py [--json FILE] [--batch B]

Shape: K = 8, n = 10, T = 500, 2048 sequences, S = 1.  One workload -- forward + backward of the differentiable local step
(ascent on detached values, final pass, sampler, backward of local_vlb + sum(samples) to the node potentials) -- in three
cases: run_inference_differentiable on the uniform batch, forced onto the materialised route (the fused mean-field kernels
have no ragged form, so they are switched off for the whole process: the uniform case is what the ragged route is built
from); run_inference_ragged_differentiable with lengths = T; and with lengths uniform in [T/2, T].  Inputs are preallocated
device tensors; every window is one forward + backward between two device events after a warm-up call; the windows of the
three cases alternate; the median of 7 and the spread are printed with the ratio to the uniform run.  No threshold.
Python's cyclic garbage of the previous window is collected BEFORE the clock starts: left to itself the collector ran
inside the first ragged window that followed a uniform one and cost 300 ms there (measured; 347 instead of 45 ms forward,
whichever ragged case came first), which says nothing about either route."""
import gc
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd.models import slds_svae  # noqa: E402

K, N, T, B = 8, 10, 500, 2048
WINDOWS = 7


def main(argv):
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no fallback"
    batch = int(argv[argv.index("--batch") + 1]) if "--batch" in argv else B
    dev = torch.device("cuda:0")
    slds_svae.SLDSMeanfieldPlan.supported = staticmethod(lambda n, T, K: False)       # the materialised route in every case
    gen = torch.Generator(device="cpu").manual_seed(0)
    to = lambda x: x.to(dev) if isinstance(x, torch.Tensor) else x
    nest = lambda g: ((to(g[0][0]), to(g[0][1])), [(to(a), tuple(to(y) for y in m)) for a, m in g[1]])
    glob = nest(slds_svae.make_slds_global_natparam(K, N, random=True, generator=gen))
    prior = nest(slds_svae.make_slds_global_natparam(K, N))
    rng = np.random.default_rng(0)
    nJ = torch.as_tensor(-0.5 * (0.5 + rng.random((batch, T, N))), device=dev).requires_grad_(True)
    nh = torch.as_tensor(2.0 * rng.standard_normal((batch, T, N)), device=dev).requires_grad_(True)
    init_eps = torch.as_tensor(rng.standard_normal((batch, T, 1, N)), device=dev)
    eps = torch.as_tensor(rng.standard_normal((batch, T, 1, N)), device=dev)
    lens = {"uniform": None,
            "full": torch.full((batch,), T, dtype=torch.int32, device=dev),
            "half_to_full": torch.as_tensor(rng.integers(T // 2, T + 1, size=batch).astype(np.int32), device=dev)}

    def step(L):
        nJ.grad = nh.grad = None
        if L is None:
            samples, _, _, local_vlb = slds_svae.run_inference_differentiable(prior, glob, (nJ, nh), 1, init_eps=init_eps, eps=eps)
        else:
            samples, _, _, local_vlb = slds_svae.run_inference_ragged_differentiable(prior, glob, (nJ, nh), L, 1,
                                                                                    init_eps=init_eps, eps=eps)
        (local_vlb + samples.sum()).backward()
        return nJ.grad

    def window(L):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gc.collect()
        torch.cuda.synchronize()
        e0.record()
        out = step(L)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    res = {k: [] for k in lens}
    for k, L in lens.items():
        _, g = window(L)                                        # warm-up (allocator, first-use costs)
        assert bool(torch.isfinite(g).all()), k
    for _ in range(WINDOWS):                                    # alternate: the three see the same machine
        for k, L in lens.items():
            res[k].append(window(L)[0])
    slds_svae.check_info()
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    rows = []
    for k in lens:
        row = dict(workload="forward+backward", K=K, n=N, T=T, B=batch, S=1, lengths=k, windows=WINDOWS, ms=med[k],
                   min_ms=min(res[k]), max_ms=max(res[k]), ratio_to_uniform=med[k] / med["uniform"])
        rows.append(row)
        print("forward+backward K=%d n=%d T=%d B=%d S=1 lengths %-12s: %.2f ms [%.2f, %.2f]  ratio to uniform %.3f"
              % (K, N, T, batch, k, med[k], min(res[k]), max(res[k]), row["ratio_to_uniform"]), flush=True)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
