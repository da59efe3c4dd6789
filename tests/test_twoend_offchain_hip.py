"""The headline E-step (lds_estep_twoend.hpp, S4 path: one chain per wavefront in the smoother phase) computes its
log-normaliser and raises its status word on chain B's wavefront, behind that wavefront's smoother: chain A's wavefront
-- the critical one -- hands the nine operands over through LDS (seven when the elimination loop ends, the meeting
node's two right behind the meeting node) and goes straight to its own smoother.  None of that may change a bit.

Reference: the row-per-chain kernel (lds_estep_twoend_rpc.hpp, forced with KERNEL_OPTIONS["twoend_rpc"]), which performs
the same operations in the same order per output element; all eight outputs are compared with torch.equal.

Shapes: n = 1, 2, 3, 5, 7, 10 -- the log-normaliser's row sum groups its terms by lane, differently at 3, 5, 6, 7;
T = 4 (the smallest the kernel takes), 5, 6, 7 (both parities of the meeting node, only peeled and remainder steps), 9 and
41 (loop trips); B = 1, 2 (records in LDS), 257, 512 (records in HBM; the largest batch of this path); with and
without node_logZ.  `lognorm` is filled with NaN before every launch -- every sequence's value has to be written, now by
the other wavefront -- and the status word must stay 0.

Two launches of one plan on different node potentials: the second equals a fresh plan's, so nothing of the hand-over block
survives a launch.

Status word: in a batch of 16, sequences 3 and 7 get node potentials that are not positive definite (node_J = +10 at
every step); checked first on the CPU (oracle/lds_numpy.py) that exactly these two fail.  Both kernels must report 4 (the
smallest failing index + 1), agree bit for bit on the other 14 sequences, and check_info() must name sequence 3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 5, 7, 10]
TS = [4, 5, 6, 7, 9, 41]
BS = [1, 2, 257, 512]

_INPUTS = {}


def _t(x):
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda:0")


def _inputs(n, T, seed=0):
    """parameters and node potentials of the LARGEST batch at (n, T), on the device; smaller batches are its head"""
    key = (n, T, seed)
    if key not in _INPUTS:
        from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
        rng = np.random.default_rng(91000 + 1000 * seed + 100 * n + T)
        init, pair = rand_lds_natparam(n, rng)
        node = rand_node_potentials((max(BS), T, n), rng, with_logZ=True)
        _INPUTS[key] = ((tuple(_t(x) for x in init), tuple(_t(x) for x in pair)), tuple(_t(x) for x in node))
    return _INPUTS[key]


def _run(plan, natparam, node):
    """one launch of `plan` with lognorm poisoned; -> (status word, the eight outputs, cloned)"""
    from svae_amd.lds.lds_inference import natural_lds_estep_general
    plan.lognorm.fill_(float("nan"))
    plan.info.zero_()
    lognorm, (Ei, Ep, En) = natural_lds_estep_general(natparam, node, plan=plan)
    torch.cuda.synchronize()
    outs = {"lognorm": lognorm, "E_node_x": En[1], "E_node_diagxx": En[0], "E_init_xx": Ei[0], "E_init_x": Ei[1],
            "E_pair_0": Ep[0], "E_pair_1": Ep[1], "E_pair_2": Ep[2]}
    return int(plan.info.item()), {k: v.clone() for k, v in outs.items()}


def _plan(name, B, T, n):
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan
    return LDSEStepPlan(B, T, n, "cuda:0", options=_lib.KERNEL_OPTIONS[name])


def _assert_equal(a, b, where, rows=None):
    assert a.keys() == b.keys() and len(a) == 8
    for key in a:
        x, y = (a[key], b[key]) if rows is None else (a[key][rows], b[key][rows])
        assert bool(torch.isfinite(x).all()), (key,) + where
        assert torch.equal(x, y), "%s differs at %r: max |a-b| = %.3e" % (key, where, float((x - y).abs().max()))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_log_normaliser_on_chain_b_agrees_with_the_row_per_chain_kernel_bit_for_bit(n, T):
    natparam, node = _inputs(n, T)
    for B in BS:
        for with_logZ in (True, False):
            nd = tuple(x[:B].contiguous() for x in (node if with_logZ else node[:2]))
            got = []
            for name in ("twoend", "twoend_rpc"):
                info, outs = _run(_plan(name, B, T, n), natparam, nd)
                assert info == 0, (name, n, T, B, with_logZ, info)
                assert outs["lognorm"].shape == (B,) and bool(torch.isfinite(outs["lognorm"]).all()), (name, n, T, B, with_logZ)
                got.append(outs)
            _assert_equal(got[0], got[1], (n, T, B, with_logZ))


@pytest.mark.parametrize("B", [2, 257])
@pytest.mark.parametrize("n,T", [(10, 41), (5, 6), (3, 9)])
def test_second_launch_of_a_plan_equals_a_fresh_plan(n, T, B):
    natparam, node1 = _inputs(n, T)
    _, node2 = _inputs(n, T, seed=1)
    nd1 = tuple(x[:B].contiguous() for x in node1)
    nd2 = tuple(x[:B].contiguous() for x in node2)
    assert not torch.equal(nd1[1], nd2[1])
    plan = _plan("twoend", B, T, n)
    info1, first = _run(plan, natparam, nd1)
    info2, second = _run(plan, natparam, nd2)
    info3, fresh = _run(_plan("twoend", B, T, n), natparam, nd2)
    assert (info1, info2, info3) == (0, 0, 0)
    assert not torch.equal(first["lognorm"], second["lognorm"])
    _assert_equal(second, fresh, (n, T, B))


BAD = (3, 7)


@pytest.mark.parametrize("n,T", [(10, 9), (3, 6)])
def test_status_word_reports_the_smallest_failing_sequence(n, T):
    from oracle import lds_numpy
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    B = 16
    rng = np.random.default_rng(93000 + 100 * n + T)
    init, pair = rand_lds_natparam(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    for b in BAD:
        node[0][b] = 10.0                        # natural parameter -1/2 J: precision -20 on the diagonal at every step
    # on the CPU first: exactly these two fail (a Cholesky factorisation meets a non-positive pivot), the others are
    # well conditioned (every filtered precision's condition number far below 1 / eps)
    failing = []
    for b in range(B):
        try:
            (_, (Jf, _)), ln = lds_numpy.natural_filter_forward_general(init, pair, tuple(x[b] for x in node))
            worst = max(np.linalg.cond(-2.0 * J) for J in Jf)
            assert np.isfinite(ln) and worst < 1e8, (b, ln, worst)
        except np.linalg.LinAlgError:
            failing.append(b)
    assert tuple(failing) == BAD, failing

    natparam = (tuple(_t(x) for x in init), tuple(_t(x) for x in pair))
    nd = tuple(_t(x) for x in node)
    good = torch.as_tensor([b for b in range(B) if b not in BAD], device="cuda:0")
    got = []
    for name in ("twoend", "twoend_rpc"):
        plan = _plan(name, B, T, n)
        info, outs = _run(plan, natparam, nd)
        assert info == min(BAD) + 1, (name, info)
        with pytest.raises(FloatingPointError, match="sequence %d " % min(BAD)):
            plan.check_info()
        got.append(outs)
    _assert_equal(got[0], got[1], (n, T, "the other 14 sequences"), rows=good)
