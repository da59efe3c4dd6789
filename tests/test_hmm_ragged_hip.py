"""GPU tests of per-sequence lengths in the HMM E-step, log-normaliser and Viterbi (lengths=, svae_hmm_ragged_estep_f64 /
svae_hmm_ragged_viterbi_f64): every sequence of a padded batch against the oracle on the sequence CUT to its own length
(oracle/hmm_numpy, the reference's compiled hmm_logZ / hmm_logZ_grad where built, tests/_hmm_viterbi_numpy.py), with
the padded region of the node potentials filled with NaN.  Tolerances: those of tests/test_hmm_hip.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_viterbi_numpy as vit  # noqa: E402
from oracle import hmm_numpy, ref  # noqa: E402  (checker only)

TOL = dict(lz=dict(rel=1e-10, abs=1e-10), st=dict(rtol=1e-8, atol=1e-12), tr=dict(rtol=1e-8, atol=1e-11))
TOL_LOG = dict(lz=dict(rel=1e-9, abs=1e-9), st=dict(rtol=1e-7, atol=1e-10), tr=dict(rtol=1e-7, atol=1e-9))


def _np(x):
    return x.detach().cpu().numpy()


def _problem(B, T, K, rng, scale=1.0):
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))   # unnormalised
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


def _padded(node, lengths):
    """a copy with everything from each sequence's length on replaced by NaN"""
    out = np.array(node, dtype=np.float64)
    for b, L in enumerate(lengths):
        out[b, L:] = np.nan
    return out


def _check_estep(init, pair, node, lengths, got, tol=TOL, with_ref=True):
    """every sequence against the oracle on node[b, :L]; the padded marginals exactly 0; the sums"""
    logZ, (Ei, Et, Es) = got
    logZ, Ei, Et, Es = _np(logZ), _np(Ei), _np(Et), _np(Es)
    pair = np.asarray(pair)
    for b, L in enumerate(lengths):
        pb = pair[b] if pair.ndim == 3 else pair
        cut = node[b, :L]
        lz, (oi, ot, os_) = hmm_numpy.hmm_estep((init, pb, cut))
        assert np.isfinite(lz) and logZ[b] == pytest.approx(lz, **tol["lz"]), b
        np.testing.assert_allclose(Ei[b], oi, **tol["st"])
        np.testing.assert_allclose(Et[b], ot, **tol["tr"])
        np.testing.assert_allclose(Es[b, :L], os_, **tol["st"])
        if with_ref and ref.available():
            rz, aux = ref.hmm_logZ((init, pb, cut))
            gi, gp, gn = ref.hmm_logZ_grad(1.0, aux)
            assert logZ[b] == pytest.approx(rz, **tol["lz"])
            np.testing.assert_allclose(Ei[b], gi, **tol["st"])
            np.testing.assert_allclose(Et[b], gp, **tol["tr"])
            np.testing.assert_allclose(Es[b, :L], gn, **tol["st"])
        assert (Es[b, L:] == 0.0).all() and not np.signbit(Es[b, L:]).any(), b      # exactly 0.0
        if tol is TOL:                                   # (scaled steps only: the sums are not pinned for log-space steps)
            assert np.abs(Es[b, :L].sum(-1) - 1).max() < 1e-12
            assert abs(Et[b].sum() - (L - 1)) < 1e-10 * max(1, L)
        if L == 1:
            assert (Et[b] == 0.0).all()
            np.testing.assert_array_equal(Ei[b], Es[b, 0])
    assert np.isfinite(logZ).all() and np.isfinite(Ei).all() and np.isfinite(Et).all() and np.isfinite(Es).all()


ROW_LENGTHS = [20, 1, 17, 2, 16, 15]


@pytest.mark.parametrize("K", [1, 3, 8, 9, 16])
def test_ragged_estep_rows_against_the_oracle_on_the_cut_sequences(K):
    """B = 6: the second wavefront has two idle rows; lengths on both sides of the 16-step renormalisation"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_logZ
    B, T = 6, 20
    rng = np.random.default_rng(1000 + K)
    init, pair, node = _problem(B, T, K, rng, 1.5)
    nan_node = _padded(node, ROW_LENGTHS)
    got = hmm_estep((init, pair, nan_node), lengths=np.array(ROW_LENGTHS))
    _check_estep(init, pair, node, ROW_LENGTHS, got)
    lz = hmm_logZ((init, pair, nan_node), lengths=torch.tensor(ROW_LENGTHS))          # a host int64 tensor
    assert torch.equal(lz, got[0])


def test_ragged_estep_rows_with_per_sequence_pair_parameters():
    from svae_amd.hmm.hmm_inference import hmm_estep
    B, T, K = 6, 20, 4
    rng = np.random.default_rng(11)
    init, _, node = _problem(B, T, K, rng)
    pairs = np.stack([_problem(1, 1, K, rng)[1] for _ in range(B)])
    got = hmm_estep((init, pairs, _padded(node, ROW_LENGTHS)), lengths=ROW_LENGTHS)
    _check_estep(init, pairs, node, ROW_LENGTHS, got)


WIDE_LENGTHS = [12, 1, 2, 7]


@pytest.mark.parametrize("K", [17, 32, 33, 64])
def test_ragged_estep_wide_against_the_oracle_on_the_cut_sequences(K):
    from svae_amd.hmm.hmm_inference import hmm_estep
    B, T = 4, 12
    rng = np.random.default_rng(2000 + K)
    init, pair, node = _problem(B, T, K, rng, 1.5)
    got = hmm_estep((init, pair, _padded(node, WIDE_LENGTHS)), lengths=np.array(WIDE_LENGTHS, np.int32))
    _check_estep(init, pair, node, WIDE_LENGTHS, got)


def test_ragged_estep_wide_with_per_sequence_pair_parameters():
    from svae_amd.hmm.hmm_inference import hmm_estep
    B, T, K = 4, 12, 24
    rng = np.random.default_rng(12)
    init, _, node = _problem(B, T, K, rng)
    pairs = np.stack([_problem(1, 1, K, rng)[1] for _ in range(B)])
    got = hmm_estep((init, pairs, _padded(node, WIDE_LENGTHS)), lengths=WIDE_LENGTHS)
    _check_estep(init, pairs, node, WIDE_LENGTHS, got)


# ---- log-space steps inside a ragged batch -----------------------------------------------------------------------------
@pytest.mark.parametrize("L_forced", [9, 5])
def test_ragged_rows_forced_transition_inside_and_beyond_the_length(L_forced):
    """the forced-transition chain of tests/test_hmm_hip.py (K = 3, T = 12, the -800 entry crossed at t = 6) as row 1 of
    a wavefront of ordinary rows with other lengths.  L = 9: the log-space step lies inside the sequence (logZ ~ -800);
    L = 5: it lies beyond the length and must not be seen -- logZ is that of the cut chain, far above -790"""
    from svae_amd.hmm.hmm_inference import hmm_estep
    K, T, B = 3, 12, 5
    init = np.array([0.0, -1e4, -1e4])
    pair = np.array([[0.0, -800.0, -1e4], [-1e4, 0.0, -1.0], [-1e4, -1.0, 0.0]])
    node = 0.3 * np.random.default_rng(0).standard_normal((B, T, K))
    node[1] = 0.0
    node[1, :6, 1:] = -1e4
    node[1, 6:, 0] = -1e4
    lengths = [12, L_forced, 3, 7, 11]
    got = hmm_estep((init, pair, _padded(node, lengths)), lengths=lengths)
    _check_estep(init, pair, node, lengths, got, tol=TOL_LOG, with_ref=False)
    lz = float(got[0][1])
    if L_forced == 9:
        assert lz < -790
    else:
        assert lz > -1.0                      # the chain stays in state 0 on zero potentials: log Z = 0


def test_ragged_wide_log_space_redo_of_a_flagged_sequence():
    """the K = 24 construction of test_hmm_wide_kernel_log_space_redo_... with T = 14: the flagged sequence (3) has L = 10
    (the forced step at t = 7 inside it), its neighbours L = 3"""
    from svae_amd.hmm.hmm_inference import hmm_estep
    K, T, B = 24, 14, 5
    rng = np.random.default_rng(8)
    init = np.full(K, -1e4); init[0] = 0.0
    pair = -2.0 + 0.3 * rng.standard_normal((K, K))
    pair[0, :] = -1e4; pair[0, 0] = 0.0; pair[0, 1] = -800.0
    pair[1:, 0] = -1e4
    node = 0.5 * rng.standard_normal((B, T, K))
    node[3] = 0.0
    node[3, :7, 1:] = -1e4
    node[3, 7:, 0] = -1e4
    lengths = [14, 5, 3, 10, 3]
    got = hmm_estep((init, pair, _padded(node, lengths)), lengths=lengths)
    _check_estep(init, pair, node, lengths, got, tol=TOL_LOG, with_ref=False)
    assert float(got[0][3]) < -790


# ---- isolation and determinism -----------------------------------------------------------------------------------------
def _flat(got):
    logZ, (Ei, Et, Es) = got
    return [_np(x) for x in (logZ, Ei, Et, Es)]


@pytest.mark.parametrize("K,B,len_a,len_b", [(5, 4, [13, 20, 7, 18], [13, 3, 20, 1]), (20, 2, [13, 20], [13, 2])])
def test_ragged_estep_isolation_and_determinism(K, B, len_a, len_b):
    """sequence 0's outputs do not change by a bit when the other rows' lengths and data are replaced; a repeated call
    is bit-identical"""
    from svae_amd.hmm.hmm_inference import hmm_estep
    T = 20
    rng = np.random.default_rng(77 + K)
    init, pair, node = _problem(B, T, K, rng)
    node_a = _padded(node, len_a)
    first, again = _flat(hmm_estep((init, pair, node_a), lengths=len_a)), _flat(hmm_estep((init, pair, node_a), lengths=len_a))
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    other = 3.0 * rng.standard_normal((B, T, K))
    other[0] = node[0]
    swapped = _flat(hmm_estep((init, pair, _padded(other, len_b)), lengths=len_b))
    for x, y in zip(first, swapped):
        assert x[0].tobytes() == y[0].tobytes()


@pytest.mark.parametrize("K", [6, 20])
def test_ragged_with_every_length_equal_to_T_agrees_with_the_uniform_call(K):
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_viterbi
    B, T = 5, 20
    rng = np.random.default_rng(300 + K)
    init, pair, node = _problem(B, T, K, rng, 2.0)
    lu, (iu, tu, su) = hmm_estep((init, pair, node))
    lr, (ir, tr, sr) = hmm_estep((init, pair, node), lengths=[T] * B)
    for b in range(B):
        assert float(lr[b]) == pytest.approx(float(lu[b]), **TOL["lz"])
    np.testing.assert_allclose(_np(ir), _np(iu), **TOL["st"])
    np.testing.assert_allclose(_np(sr), _np(su), **TOL["st"])
    np.testing.assert_allclose(_np(tr), _np(tu), **TOL["tr"])
    zu, scu = hmm_viterbi((init, pair, node), return_score=True)
    zr, scr = hmm_viterbi((init, pair, node), return_score=True, lengths=[T] * B)
    assert torch.equal(zu, zr) and _np(scu).tobytes() == _np(scr).tobytes()


# ---- Viterbi ---------------------------------------------------------------------------------------------------------------
def _check_viterbi(init, pair, node, lengths, states, score):
    states, score = _np(states), _np(score)
    assert states.dtype == np.int32
    pair = np.asarray(pair)
    for b, L in enumerate(lengths):
        want, ws = vit.viterbi(init, pair[b] if pair.ndim == 3 else pair, node[b, :L])
        np.testing.assert_array_equal(states[b, :L], want)
        assert vit.bits(score[b]) == vit.bits(ws), (b, score[b], ws)
        assert (states[b, L:] == -1).all(), b


VIT_ROW_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 40]
VIT_WIDE_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 140]


@pytest.mark.parametrize("K,batched_pairs,minus_inf", [(1, False, False), (3, True, False), (8, False, True),
                                                       (16, False, False)])
def test_ragged_viterbi_rows_bit_for_bit(K, batched_pairs, minus_inf):
    """lengths on both sides of the 8-step look-ahead and of the 16-step backtrace blocks; B = 9: three wavefronts, the
    last with three idle rows"""
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    B, T = 9, 40
    rng = np.random.default_rng(4000 + K)
    init = rng.standard_normal(K)
    pair = 2.0 * rng.standard_normal((B, K, K) if batched_pairs else (K, K))
    node = 3.0 * rng.standard_normal((B, T, K))
    if minus_inf:
        node[:, 5, 2] = -np.inf                         # a forbidden state inside the live region of every L > 5
        node[4, 10, :4] = -np.inf
    states, score = hmm_viterbi((init, pair, _padded(node, VIT_ROW_LENGTHS)), return_score=True,
                                lengths=np.array(VIT_ROW_LENGTHS))
    _check_viterbi(init, pair, node, VIT_ROW_LENGTHS, states, score)
    only = hmm_viterbi((init, pair, _padded(node, VIT_ROW_LENGTHS)), lengths=VIT_ROW_LENGTHS)
    assert torch.equal(only, states)


@pytest.mark.parametrize("K", [17, 32, 33, 64])
def test_ragged_viterbi_wide_bit_for_bit(K):
    """lengths on both sides of the 64-step backtrace blocks"""
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    B, T = 8, 140
    rng = np.random.default_rng(5000 + K)
    init = rng.standard_normal(K)
    pair = 2.0 * rng.standard_normal((K, K))
    node = 3.0 * rng.standard_normal((B, T, K))
    states, score = hmm_viterbi((init, pair, _padded(node, VIT_WIDE_LENGTHS)), return_score=True,
                                lengths=torch.tensor(VIT_WIDE_LENGTHS, dtype=torch.int32, device="cuda"))
    _check_viterbi(init, pair, node, VIT_WIDE_LENGTHS, states, score)


# ---- bad lengths and argument errors -------------------------------------------------------------------------------------
def _clear_status():
    from svae_amd.hmm.hmm_inference import check_lengths_status
    try:
        check_lengths_status()
    except FloatingPointError:
        pass


@pytest.mark.parametrize("K", [4, 20])
def test_bad_lengths_are_clamped_and_raise_the_status_word(K):
    """a device `lengths` holding 0 and T + 1 among good ones: the call completes, the good sequences match the oracle,
    check=True raises, and a following clean call with check=True does not"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_viterbi
    _clear_status()
    B, T = 5, 9
    rng = np.random.default_rng(600 + K)
    init, pair, node = _problem(B, T, K, rng)
    raw = [4, 0, 9, T + 1, 6]
    good = [0, 2, 4]
    lengths = torch.tensor(raw, dtype=torch.int32, device="cuda")
    clamped = [min(max(l, 1), T) for l in raw]
    nan_node = _padded(node, clamped)
    logZ, (Ei, Et, Es) = hmm_estep((init, pair, nan_node), lengths=lengths)
    states, score = hmm_viterbi((init, pair, nan_node), return_score=True, lengths=lengths)
    torch.cuda.synchronize()
    pick = lambda x: x[good]
    _check_estep(init, pair, node[good], [raw[b] for b in good], (pick(logZ), (pick(Ei), pick(Et), pick(Es))))
    _check_viterbi(init, pair, node[good], [raw[b] for b in good], pick(states), pick(score))
    with pytest.raises(FloatingPointError):
        hmm_estep((init, pair, nan_node), lengths=lengths, check=True)
    ok = torch.tensor(clamped, dtype=torch.int32, device="cuda")
    hmm_estep((init, pair, nan_node), lengths=ok, check=True)                     # the word was cleared: no raise
    with pytest.raises(FloatingPointError):
        hmm_viterbi((init, pair, nan_node), lengths=lengths, check=True)
    hmm_viterbi((init, pair, nan_node), lengths=ok, check=True)


def test_argument_errors_come_before_any_launch():
    """unbatched node potentials with lengths, a wrong shape, a float dtype: ValueError, and the caller's workspace (which
    every kernel writes from its first step on) is untouched"""
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_logZ, hmm_logZ_differentiable, hmm_viterbi
    B, T, K = 3, 6, 4
    rng = np.random.default_rng(9)
    init, pair, node = _problem(B, T, K, rng)
    lib = _lib.load()
    ews = torch.full((int(lib.svae_hmm_workspace_bytes(B, T, K)) // 8,), 7.25, dtype=torch.float64, device="cuda")
    vws = torch.full((int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K)),), 113, dtype=torch.uint8, device="cuda")
    bad = [dict(natparam=(init, pair, node[0]), lengths=[3]),                        # unbatched
           dict(natparam=(init, pair, node), lengths=[3, 4]),                        # wrong shape
           dict(natparam=(init, pair, node), lengths=np.array([[3, 4, 5]])),
           dict(natparam=(init, pair, node), lengths=np.array([3.0, 4.0, 5.0])),     # float dtype
           dict(natparam=(init, pair, node), lengths=torch.tensor([3.0, 4.0, 5.0], device="cuda"))]
    for kw in bad:
        with pytest.raises(ValueError):
            hmm_estep(kw["natparam"], workspace=ews, lengths=kw["lengths"])
        with pytest.raises(ValueError):
            hmm_viterbi(kw["natparam"], workspace=vws, lengths=kw["lengths"])
        with pytest.raises(ValueError):
            hmm_logZ(kw["natparam"], lengths=kw["lengths"])
        with pytest.raises(ValueError):
            hmm_logZ_differentiable(kw["natparam"], lengths=kw["lengths"])
    torch.cuda.synchronize()
    assert bool((ews == 7.25).all()) and bool((vws == 113).all())
    # (the same buffers ARE written by a good call: the check above is not vacuous)
    hmm_estep((init, pair, node), workspace=ews, lengths=[3, 4, 5])
    hmm_viterbi((init, pair, node), workspace=vws, lengths=[3, 4, 5])
    torch.cuda.synchronize()
    assert not bool((ews == 7.25).all()) and not bool((vws == 113).all())


@pytest.mark.parametrize("K", [4, 20])
def test_ragged_logZ_gradient_is_the_marginals_and_zero_from_the_length_on(K):
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_logZ_differentiable
    B, T = 4, 10
    lengths = [10, 1, 6, 3]
    rng = np.random.default_rng(700 + K)
    init, pair, node = _problem(B, T, K, rng)
    nan_node = torch.tensor(_padded(node, lengths), device="cuda", requires_grad=True)
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device="cuda")
    logZ = hmm_logZ_differentiable((t(init), t(pair), nan_node), lengths=lengths)
    logZ.sum().backward()
    want_lz, (_, _, Es) = hmm_estep((init, pair, nan_node.detach()), lengths=lengths)
    assert torch.equal(logZ.detach(), want_lz)
    assert torch.equal(nan_node.grad, Es)
    for b, L in enumerate(lengths):
        assert bool((nan_node.grad[b, L:] == 0.0).all())
        _, (_, _, os_) = hmm_numpy.hmm_estep((init, pair, node[b, :L]))
        np.testing.assert_allclose(_np(nan_node.grad[b, :L]), os_, **TOL["st"])
