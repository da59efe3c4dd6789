"""Per-sequence lengths on the SLDS model layer against the uniform materialised route at the same shape, in one process:
python tools/bench_slds_ragged.py [--json FILE] [--batch B]

Shape: K = 8, n = 10, T = 500, 2048 sequences.  Two workloads -- one coordinate ascent (optimize_local_meanfield,
pair_stats=False) and run_inference (ascent + final pass + sampler, S = 1) -- in three cases: the uniform call on the
materialised route (the fused mean-field kernels have no ragged form, so they are switched off for the whole process: the
uniform case is what the ragged route is built from), lengths = T, and lengths uniform in [T/2, T].  Inputs are
preallocated device tensors; every window is one call between two device events after a warm-up call; the windows of the
three cases alternate; the median of 7 and the spread are printed with the ratio to the uniform run.  No threshold."""
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
    # the materialised route in every case (run_inference has no `fused` argument: the selector is switched off instead)
    slds_svae.SLDSMeanfieldPlan.supported = staticmethod(lambda n, T, K: False)
    gen = torch.Generator(device="cpu").manual_seed(0)
    to = lambda x: x.to(dev) if isinstance(x, torch.Tensor) else x
    nest = lambda g: ((to(g[0][0]), to(g[0][1])), [(to(a), tuple(to(y) for y in m)) for a, m in g[1]])
    glob = nest(slds_svae.make_slds_global_natparam(K, N, random=True, generator=gen))
    prior = nest(slds_svae.make_slds_global_natparam(K, N))
    rng = np.random.default_rng(0)
    node = (torch.as_tensor(-0.5 * (0.5 + rng.random((batch, T, N))), device=dev),
            torch.as_tensor(2.0 * rng.standard_normal((batch, T, N)), device=dev))
    init_eps = torch.as_tensor(rng.standard_normal((batch, T, 1, N)), device=dev)
    eps = torch.as_tensor(rng.standard_normal((batch, T, 1, N)), device=dev)
    lens = {"uniform": None,
            "full": torch.full((batch,), T, dtype=torch.int32, device=dev),
            "half_to_full": torch.as_tensor(rng.integers(T // 2, T + 1, size=batch).astype(np.int32), device=dev)}

    def ascent(L):
        return slds_svae.optimize_local_meanfield(glob, node, init_eps, pair_stats=False, lengths=L)[3]

    def inference(L):
        return slds_svae.run_inference(prior, glob, node, 1, init_eps=init_eps, eps=eps, lengths=L)[3]

    def window(fn, L):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn(L)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rows = []
    for name, fn in (("ascent", ascent), ("run_inference", inference)):
        res = {k: [] for k in lens}
        sweeps = {}
        for k, L in lens.items():
            _, out = window(fn, L)                              # warm-up (allocator, first-use costs)
            if name == "ascent":
                sweeps[k] = float(out.double().mean())
        for _ in range(WINDOWS):                                # alternate: the three see the same machine
            for k, L in lens.items():
                res[k].append(window(fn, L)[0])
        slds_svae.check_info()
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        for k in lens:
            row = dict(workload=name, K=K, n=N, T=T, B=batch, lengths=k, windows=WINDOWS, ms=med[k], min_ms=min(res[k]),
                       max_ms=max(res[k]), ratio_to_uniform=med[k] / med["uniform"], mean_sweeps=sweeps.get(k))
            rows.append(row)
            print("%-13s K=%d n=%d T=%d B=%d lengths %-12s: %.2f ms [%.2f, %.2f]  ratio to uniform %.3f%s"
                  % (name, K, N, T, batch, k, med[k], min(res[k]), max(res[k]), row["ratio_to_uniform"],
                     "" if k not in sweeps else "  (mean sweeps %.2f)" % sweeps[k]), flush=True)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
