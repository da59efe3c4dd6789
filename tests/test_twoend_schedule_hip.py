"""The two-ended E-step kernels are re-scheduled, never re-computed: the default kernel (one sequence per workgroup, the
elimination step's stages as generated asm statements, lds_estep_twoend.hpp) and the row-per-chain kernel
(lds_estep_twoend_rpc.hpp, forced with KERNEL_OPTIONS["twoend_rpc"]) perform the same operations in the same order
per output element, so every output agrees BIT FOR BIT -- at every latent dimension, at the chain lengths that take
each remainder of the smoother's four-step loop and each parity of the meeting node, and on both elimination loops
(records in LDS up to 256 sequences, in the HBM workspace above).

One output is exempt at two sizes: `lognorm` at n = 3 and n = 7.  There the two kernels differ in the last bits (up to
2.8e-14 absolute on values of order 10, in 45 of these 56 shapes) BEFORE and after the re-scheduling alike -- the
log-normaliser is a sum over lanes and chains that the row-per-chain layout takes in another order when n & 3 == 3 -- so
it is held to the rounding of such a sum instead; every other output is bit-identical there too.  (The re-scheduled
default kernel itself reproduces its predecessor's bytes on all 8 outputs of all 196 shapes.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 7, 9, 10]          # odd and even slot counts, the right-hand-side lane split
TS = [4, 5, 8, 9, 16, 17, 33]        # TE_MIN_T, odd / even meeting node, the (s & 3) == 3 renormalisation, every loop remainder
BS = [1, 3, 11, 300]                 # odd batches; 300 > 256: the HBM-record elimination loop, <= 256: the LDS-record one
LOGNORM_REORDERED_NS = (3, 7)        # see above

_INPUTS = {}


def _inputs(n, T):
    """parameters and node potentials of the LARGEST batch at (n, T), on the device; smaller batches are its head"""
    if (n, T) not in _INPUTS:
        from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
        rng = np.random.default_rng(1000 * n + T)
        init, pair = rand_lds_natparam(n, rng)
        node = rand_node_potentials((max(BS), T, n), rng, with_logZ=True)
        t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda:0")
        _INPUTS[(n, T)] = ((tuple(t(x) for x in init), tuple(t(x) for x in pair)), tuple(t(x) for x in node))
    return _INPUTS[(n, T)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_default_kernel_and_row_per_chain_kernel_agree_bit_for_bit(n, T):
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    natparam, node = _inputs(n, T)
    for B in BS:
        outs = []
        for name in ("twoend", "twoend_rpc"):
            plan = LDSEStepPlan(B, T, n, "cuda:0", options=_lib.KERNEL_OPTIONS[name])
            lognorm, (Ei, Ep, En) = natural_lds_estep_general(natparam, tuple(x[:B].contiguous() for x in node), plan=plan)
            torch.cuda.synchronize()
            outs.append({"lognorm": lognorm, "E_node_x": En[1], "E_node_diagxx": En[0], "E_init_xx": Ei[0],
                         "E_init_x": Ei[1], "E_pair_0": Ep[0], "E_pair_1": Ep[1], "E_pair_2": Ep[2]})
        for key in outs[0]:
            a, b = outs[0][key], outs[1][key]
            assert bool(torch.isfinite(a).all()), (key, n, T, B)
            if key == "lognorm" and n in LOGNORM_REORDERED_NS:
                # ~ 2 T (n + 1) terms of magnitude <= max(1, |lognorm|) each, summed in two orders: a few ulp per term
                bound = 4.0 * 2 * T * (n + 1) * 2.0 ** -53 * max(1.0, float(a.abs().max()))
                assert float((a - b).abs().max()) <= bound, (key, n, T, B, float((a - b).abs().max()), bound)
                continue
            assert torch.equal(a, b), "%s differs at n=%d T=%d B=%d: max |a-b| = %.3e" % (
                key, n, T, B, float((a - b).abs().max()))
