"""Per-phase cycle counts of the two-ended kernel (variants/te_timing.so, built with
-DSVAE_PHASE_TIMING): SVAE_AMD_LIB=variants/te_timing.so python tools/te_phase_timing.py

Up to 512 sequences the kernel is the S4 variant (second wavefront per sequence in the smoother phase): the timing
build leaves [wavefront][16] counters at the head of every sequence's E_init row (lds_estep_twoend_s4.hpp), printed
here as one table per batch, mean over the sequences.  Above, the one-wavefront kernel's six counters as before."""
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd.lds.lds_inference import LDSEStepPlan
from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
T, n = 200, 10
dev = torch.device("cuda:0")
# (row label, counter indices summed) in the order the phases run on chain A's wavefront; chain B's wavefront runs the
# smoother's set-up first and then sleeps at the barrier through chain A's elimination
S4_PHASES = [("prologue", (11,)), ("elimination loop", (0, 1, 2, 3, 12)), ("smoother set-up (reads no record)", (9,)),
             ("meeting node", (13,)), ("wait at the barrier", (10,)), ("log-normaliser", (14,)),
             ("barrier exit -> first smoother multiply-add", (4,)), ("peeled steps", (5,)), ("four-step loop", (6,)),
             ("remainder", (7,)), ("statistics epilogue", (8,))]
for B in (256, 512, 1024, 4096):
    init, pair = rand_lds_natparam(n, np.random.default_rng(0))
    node = rand_node_potentials((B, T, n), np.random.default_rng(1))
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev).contiguous()
    plan = LDSEStepPlan(B, T, n, dev)
    args = [t(init[0]), t(init[1]), t(init[2]).reshape(1), t(pair[0]), t(pair[1]), t(pair[2]), t(pair[3]).reshape(1), t(node[0]), t(node[1]), None]
    for _ in range(3):
        plan.launch(*args)
    torch.cuda.synchronize()
    e = T // 2
    if B <= 512:
        tm = plan.E_init[:, :32].cpu().numpy().reshape(B, 2, 16).mean(0)
        print("B=%d cycles per launch (mean over sequences)  %-44s %10s %10s" % (B, "", "chain A", "chain B"))
        for name, idx in S4_PHASES:
            print("  %-44s %10.0f %10.0f" % (name, tm[0, list(idx)].sum(), tm[1, list(idx)].sum()))
        print("  %-44s %10.0f %10.0f" % ("total", tm[0].sum(), tm[1].sum()))
        continue
    tm = plan.E_init[:, :6].cpu().numpy()
    m = tm.mean(0)
    print("B=%d cycles per iteration (mean over waves): setup %.0f  gauss_jordan %.0f  schur %.0f  scale+store+gather %.0f | fwd %.0f   meeting+lognorm %.0f (once)   smoother %.0f per step | total %.0f cycles"
          % (B, m[0] / e, m[1] / e, m[2] / e, m[3] / e, m[:4].sum() / e, m[4], m[5] / (e + 1), m.sum()))
