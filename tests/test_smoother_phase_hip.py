"""The smoother phase of the headline E-step (lds_estep_twoend_s4.hpp: one chain per wavefront, four DPP rows per chain)
issues its three product stages as one generated statement each, and the hand-over between the two phases is
re-ordered: chain B's wavefront sets up before its barrier, chain A's computes the log-normaliser behind it.  None of
that may change a bit: the default kernel is compared with the row-per-chain kernel (lds_estep_twoend_rpc.hpp, forced
with KERNEL_OPTIONS["twoend_rpc"]), which performs the same operations in the same order per output element, with
torch.equal on all eight outputs.

Shapes: n = 5, 6, 8, 10 are the slot shapes (J, J1, N & 3) = (2, 2, 1), (2, 2, 2), (2, 3, 0), (3, 3, 2) of the four-row layout
(tests/test_twoend_schedule_hip.py has 10 alone of these); T = 40 .. 47 takes both parities of the meeting node with every
remainder of the four-steps-per-trip loop at four trips or more; B = 2 keeps the records in LDS, B = 257 in the HBM
workspace.  The status word must stay 0 and the log-normaliser -- now written after the barrier -- must be written for
every sequence: its buffer is filled with NaN before the launch.

What this test found: at n = 5 and n = 6 the two kernels' `lognorm` differed (7.1e-15 .. 9.1e-13, once 5.8e-11; the
other seven outputs bit-identical), before the re-scheduling as after.  The log-normaliser's row sums are butterflies, so
their grouping depends on the lane of each term, and the default kernel kept the quadratic term in lane 15 where the
row-per-chain kernel keeps it in lane n: the same sum grouped differently at n = 3, 5, 6, 7.  The default kernel now
moves the term to lane n before it sums (lds_estep_twoend.hpp, log_normaliser)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [5, 6, 8, 10]
TS = list(range(40, 48))
BS = [2, 257]

_INPUTS = {}


def _inputs(n, T):
    """parameters and node potentials of the LARGEST batch at (n, T), on the device; the smaller batch is its head"""
    if (n, T) not in _INPUTS:
        from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
        rng = np.random.default_rng(77000 + 100 * n + T)
        init, pair = rand_lds_natparam(n, rng)
        node = rand_node_potentials((max(BS), T, n), rng, with_logZ=True)
        t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda:0")
        _INPUTS[(n, T)] = ((tuple(t(x) for x in init), tuple(t(x) for x in pair)), tuple(t(x) for x in node))
    return _INPUTS[(n, T)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_smoother_phase_agrees_with_the_row_per_chain_kernel_bit_for_bit(n, T):
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    natparam, node = _inputs(n, T)
    assert len(node) == 3, "node_logZ given"
    for B in BS:
        outs = []
        for name in ("twoend", "twoend_rpc"):
            plan = LDSEStepPlan(B, T, n, "cuda:0", options=_lib.KERNEL_OPTIONS[name])
            plan.lognorm.fill_(float("nan"))
            plan.info.zero_()
            lognorm, (Ei, Ep, En) = natural_lds_estep_general(natparam, tuple(x[:B].contiguous() for x in node), plan=plan)
            torch.cuda.synchronize()
            assert int(plan.info.item()) == 0, (name, n, T, B, int(plan.info.item()))
            assert lognorm.shape == (B,) and bool(torch.isfinite(lognorm).all()), (name, n, T, B)
            outs.append({"lognorm": lognorm, "E_node_x": En[1], "E_node_diagxx": En[0], "E_init_xx": Ei[0],
                         "E_init_x": Ei[1], "E_pair_0": Ep[0], "E_pair_1": Ep[1], "E_pair_2": Ep[2]})
        for key in outs[0]:
            a, b = outs[0][key], outs[1][key]
            assert bool(torch.isfinite(a).all()), (key, n, T, B)
            assert torch.equal(a, b), "%s differs at n=%d T=%d B=%d: max |a-b| = %.3e" % (
                key, n, T, B, float((a - b).abs().max()))
