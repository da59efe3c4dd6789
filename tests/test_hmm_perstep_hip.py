"""GPU tests of the HMM E-step with per-step transition potentials (hmm_estep_perstep, hmm_logZ_perstep,
hmm_logZ_perstep_differentiable; svae_hmm_perstep_estep_f64, csrc/hmm_estep_perstep.hip) against the log-space NumPy
oracle tests/_hmm_perstep_numpy.py: parity over every K range and group width, the reduction to hmm_estep at constant
P_t, the range cases, per-sequence lengths, the gradient and graph capture.

Tolerances: those of tests/test_hmm_ragged_hip.py.  The kernel has ONE route, log space throughout, so every comparison
with the oracle uses TOL_LOG (the tolerance of the log-space route), element-wise on the per-step E_trans; the reduction
to hmm_estep on mild potentials uses TOL.  There is no fallback and so no perstep_redone_sequences to test."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_perstep_numpy as ps  # noqa: E402

TOL = dict(lz=dict(rel=1e-10, abs=1e-10), st=dict(rtol=1e-8, atol=1e-12), tr=dict(rtol=1e-8, atol=1e-11))
TOL_LOG = dict(lz=dict(rel=1e-9, abs=1e-9), st=dict(rtol=1e-7, atol=1e-10), tr=dict(rtol=1e-7, atol=1e-9))


def _np(x):
    return x.detach().cpu().numpy()


def _problem(B, T, K, rng, pair_batched, scale=1.0):
    init = np.log(rng.dirichlet(np.ones(K)))
    lead = (B, T - 1) if pair_batched else (T - 1,)
    pair = np.log(rng.dirichlet(np.ones(K), size=lead + (K,))) + 0.5 * rng.standard_normal(lead + (K, K))
    pair = pair + 3.0 * rng.standard_normal(lead + (1, 1))              # every step at its own offset
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


def _check(init, pair, node, got, lengths=None, tol=TOL_LOG, want_trans=True):
    """every sequence against the oracle on the sequence cut to its length; exact zeros behind it; everything finite"""
    logZ, (Ei, Et, Es) = got
    logZ, Ei, Es = _np(logZ), _np(Ei), _np(Es)
    B, T, K = node.shape
    assert logZ.shape == (B,) and Ei.shape == (B, K) and Es.shape == (B, T, K)
    if want_trans:
        Et = _np(Et)
        assert Et.shape == (B, T - 1, K, K)
    else:
        assert Et is None
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        pb = pair[b] if pair.ndim == 4 else pair
        lz, (oi, ot, os_) = ps.hmm_estep_perstep((init, pb[:L - 1], node[b, :L]))
        assert np.isfinite(lz) and logZ[b] == pytest.approx(lz, **tol["lz"]), b
        np.testing.assert_allclose(Ei[b], oi, **tol["st"])
        np.testing.assert_allclose(Es[b, :L], os_, **tol["st"])
        assert (Es[b, L:] == 0.0).all() and not np.signbit(Es[b, L:]).any(), b
        np.testing.assert_array_equal(Ei[b], Es[b, 0])
        if want_trans:
            np.testing.assert_allclose(Et[b, :L - 1], ot, **tol["tr"])
            assert (Et[b, L - 1:] == 0.0).all() and not np.signbit(Et[b, L - 1:]).any(), b
            # the kernel forms a row of xi_t from gamma_t[j] and the backward step's own normalised terms
            np.testing.assert_allclose(Et[b, :L - 1].sum(-1), Es[b, :L - 1], rtol=1e-12, atol=1e-15)
    assert np.isfinite(logZ).all() and np.isfinite(Ei).all() and np.isfinite(Es).all()
    assert not want_trans or np.isfinite(Et).all()


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip((a[0],) + tuple(a[1]), (b[0],) + tuple(b[1])) if x is not None
               and y is not None)


# ---- parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 16, 17, 32, 33, 64])
def test_perstep_estep_against_the_oracle(K):
    """T on both sides of every trip count that can go wrong (1: no pair step at all), B with partially filled
    wavefronts at every group width (8, 4, 2 or 1 sequences per wavefront), shared and per-sequence pair parameters,
    with and without E_trans (the other three outputs bit for bit the same)"""
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep, hmm_logZ_perstep
    rng = np.random.default_rng(3000 + K)
    for T in (1, 2, 3, 7, 37):
        for B in (1, 5, 9):
            for pair_batched in (False, True):
                init, pair, node = _problem(B, T, K, rng, pair_batched, 1.5)
                got = hmm_estep_perstep((init, pair, node))
                _check(init, pair, node, got)
                lean = hmm_estep_perstep((init, pair, node), want_trans=False)
                _check(init, pair, node, lean, want_trans=False)
                assert _same_bits(got, lean), (T, B, pair_batched)
                assert torch.equal(hmm_logZ_perstep((init, pair, node)), got[0])
    # the unbatched call: unbatched results, those of the batch's sequence bit for bit
    init, pair, node = _problem(2, 7, K, rng, True)
    lz, (ei, et, es) = hmm_estep_perstep((init, pair[1], node[1]))
    assert lz.shape == () and ei.shape == (K,) and et.shape == (6, K, K) and es.shape == (7, K)
    both = hmm_estep_perstep((init, pair, node))
    assert _same_bits((lz, (ei, et, es)), (both[0][1], tuple(x[1] for x in both[1])))
    lz1, (_, et1, _) = hmm_estep_perstep((init, pair[1], node[1]), want_trans=False)
    assert et1 is None and torch.equal(lz1, lz)


@pytest.mark.parametrize("K", [3, 16, 17, 64])
def test_perstep_estep_reduces_to_the_uniform_estep_at_constant_matrices(K):
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_estep_perstep
    B, T = 5, 37
    rng = np.random.default_rng(4000 + K)
    init = np.log(rng.dirichlet(np.ones(K)))
    P = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    node = 1.5 * rng.standard_normal((B, T, K))
    lz, (ei, et, es) = hmm_estep_perstep((init, np.broadcast_to(P, (T - 1, K, K)).copy(), node))
    uz, (ui, ut, us) = hmm_estep((init, P, node))
    for b in range(B):
        assert float(lz[b]) == pytest.approx(float(uz[b]), **TOL["lz"])
    np.testing.assert_allclose(_np(ei), _np(ui), **TOL["st"])
    np.testing.assert_allclose(_np(es), _np(us), **TOL["st"])
    np.testing.assert_allclose(_np(et).sum(1), _np(ut), **TOL["tr"])


# ---- range ------------------------------------------------------------------------------------------------------------------
def _range_case(case, B, T, K, rng):
    init, pair, node = _problem(B, T, K, rng, True, 1.0)
    if case == "offsets":                       # (a) one step's matrix offset by -2000 and another's by +900
        pair[:, 1] -= 2000.0
        pair[:, T - 2] += 900.0
        pair[0, 3] -= 2000.0
    elif case == "left_to_right":               # (b) at some steps only: -inf below the diagonal
        for t in (0, 2, 3, T - 2):
            pair[:, t][:, np.tril_indices(K, -1)[0], np.tril_indices(K, -1)[1]] = -np.inf
    elif case == "deep_entries":                # (c) entries 800 nats below their row's maximum, nodes spread over 1e3 nats
        deep = rng.random(pair.shape) < 0.5
        deep[..., np.arange(K), np.arange(K)] = False                   # every row keeps its diagonal
        pair[deep] -= 800.0
        node = node + 1e3 * rng.random(node.shape)
    elif case == "forbidden_stretch":           # (d) a state forbidden by -inf node potentials on a stretch of steps
        node[:, 2:6, K - 1] = -np.inf
        node[1, 0, 0] = -np.inf
    return init, pair, node


@pytest.mark.parametrize("K", [2, 8, 16, 24, 64])
@pytest.mark.parametrize("case", ["offsets", "left_to_right", "deep_entries", "forbidden_stretch"])
def test_perstep_estep_keeps_the_oracle_over_the_whole_domain(case, K):
    """finite or -inf potentials, any offset per step, entries hundreds of nats down: logZ stays finite and every
    sequence has the log-space result (one route: nothing is flagged, nothing is redone)"""
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep
    B, T = 3, 9
    rng = np.random.default_rng(5000 + K)
    init, pair, node = _range_case(case, B, T, K, rng)
    got = hmm_estep_perstep((init, pair, node))
    _check(init, pair, node, got)
    if case == "offsets":                       # a step's common offset only shifts logZ
        init0, pair0, node0 = _range_case("none", B, T, K, np.random.default_rng(5000 + K))
        base = hmm_estep_perstep((init0, pair0, node0))
        shift = np.array([-2000.0 + 900.0 - 2000.0, -2000.0 + 900.0, -2000.0 + 900.0])
        np.testing.assert_allclose(_np(got[0]) - shift, _np(base[0]), rtol=0, atol=1e-9)
        np.testing.assert_allclose(_np(got[1][1]), _np(base[1][1]), **TOL_LOG["tr"])
    # a sequence's results do not depend on its neighbours: alone, bit for bit
    alone = hmm_estep_perstep((init, pair[1:2], node[1:2]))
    assert _same_bits(alone, (got[0][1:2], tuple(x[1:2] for x in got[1])))


# ---- lengths ----------------------------------------------------------------------------------------------------------------
def _padded(pair, node, lengths):
    """copies with node steps >= L and pair steps >= L - 1 replaced by NaN (pair per sequence)"""
    node = np.array(node)
    pair = np.array(pair)
    for b, L in enumerate(lengths):
        node[b, L:] = np.nan
        pair[b, L - 1:] = np.nan
    return pair, node


@pytest.mark.parametrize("K", [3, 8, 16, 17, 33, 64])
def test_perstep_estep_with_lengths_against_the_oracle_on_the_cut_sequences(K):
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep, hmm_logZ_perstep
    B, T = 9, 12
    rng = np.random.default_rng(6000 + K)
    lengths = np.array([1, 2, T - 1, T] + list(rng.integers(1, T + 1, B - 4)))
    init, pair, node = _problem(B, T, K, rng, True, 1.5)
    nan_pair, nan_node = _padded(pair, node, lengths)
    got = hmm_estep_perstep((init, nan_pair, nan_node), lengths=lengths, check=True)
    _check(init, pair, node, got, lengths)
    lean = hmm_estep_perstep((init, nan_pair, nan_node), lengths=torch.tensor(lengths), want_trans=False)
    assert _same_bits(got, lean)
    assert torch.equal(hmm_logZ_perstep((init, nan_pair, nan_node), lengths=lengths), got[0])
    # shared pair parameters (finite everywhere: another sequence may need the step), NaN nodes
    shared = hmm_estep_perstep((init, pair[0], nan_node), lengths=lengths)
    _check(init, pair[0], node, shared, lengths)
    # no sequence sees another's length: the other sequences' lengths permuted, sequence by sequence the same bits
    perm = rng.permutation(B)
    got_p = hmm_estep_perstep((init, nan_pair[perm], nan_node[perm]), lengths=lengths[perm])
    idx = torch.as_tensor(perm, device=got[0].device)
    assert _same_bits(got_p, (got[0][idx], tuple(x[idx] for x in got[1])))
    other = lengths.copy()
    other[1:] = other[1:][::-1]                                          # sequence 0 keeps L = 1, its wavefront's lengths move
    o_pair, o_node = _padded(pair, node, other)
    got_o = hmm_estep_perstep((init, o_pair, o_node), lengths=other)
    assert _same_bits((got_o[0][:1], tuple(x[:1] for x in got_o[1])), (got[0][:1], tuple(x[:1] for x in got[1])))


def test_perstep_estep_clamps_a_length_outside_1_to_T_and_says_so():
    from svae_amd.hmm.hmm_inference import check_lengths_status, hmm_estep_perstep
    B, T, K = 5, 6, 4
    rng = np.random.default_rng(61)
    init, pair, node = _problem(B, T, K, rng, False)
    try:
        check_lengths_status()                                           # start from a clean word
    except FloatingPointError:
        pass
    good = np.array([1, T, 3, 1, T])
    for bad in (np.array([0, T + 1, 3, -5, 1000]), np.array([0, T, 3, 1, T]), np.array([1, T + 1, 3, 1, T])):
        got = hmm_estep_perstep((init, pair, node), lengths=bad)        # check=False: no synchronisation, no error
        clamped = hmm_estep_perstep((init, pair, node), lengths=np.clip(bad, 1, T))
        with pytest.raises(FloatingPointError):
            check_lengths_status()
        assert _same_bits(got, clamped)
        with pytest.raises(FloatingPointError):
            hmm_estep_perstep((init, pair, node), lengths=bad, check=True)
        hmm_estep_perstep((init, pair, node), lengths=good, check=True)  # the word was cleared: a clean call stays clean
    _check(init, pair, node, hmm_estep_perstep((init, pair, node), lengths=good, check=True), good)


# ---- gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_batched", [False, True])
@pytest.mark.parametrize("with_lengths", [False, True])
def test_perstep_logZ_gradcheck(pair_batched, with_lengths):
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep, hmm_logZ_perstep_differentiable
    B, T, K = 2, 4, 3
    rng = np.random.default_rng(70 + 2 * pair_batched + with_lengths)
    init, pair, node = _problem(B, T, K, rng, pair_batched)
    lengths = np.array([2, T]) if with_lengths else None
    dev = torch.device("cuda")
    ti, tp, tn = (torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True) for x in (init, pair, node))
    assert torch.autograd.gradcheck(lambda i, p, n: hmm_logZ_perstep_differentiable((i, p, n), lengths=lengths),
                                    (ti, tp, tn), eps=1e-6, atol=1e-7, rtol=1e-6)
    g = torch.tensor([0.7, -1.3], dtype=torch.float64, device=dev)
    (hmm_logZ_perstep_differentiable((ti, tp, tn), lengths=lengths) * g).sum().backward()
    lz, (ei, et, es) = hmm_estep_perstep((init, pair, node), lengths=lengths)
    assert torch.equal(tn.grad, g[:, None, None] * es)
    assert torch.equal(ti.grad, (g[:, None] * ei).sum(0))
    d_pair = g[:, None, None, None] * et
    assert torch.equal(tp.grad, d_pair if pair_batched else d_pair.sum(0))
    if with_lengths:                                                     # exactly 0 from the length on
        assert (tn.grad[0, 2:] == 0).all() and (tn.grad[0, :2] != 0).all()
        if pair_batched:
            assert (tp.grad[0, 1:] == 0).all() and (tp.grad[0, :1] != 0).all()
    # the unbatched form
    ui, up, un = (torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True)
                  for x in (init, pair[0] if pair_batched else pair, node[0]))
    assert torch.autograd.gradcheck(lambda i, p, n: hmm_logZ_perstep_differentiable((i, p, n)), (ui, up, un),
                                    eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,with_lengths", [(8, False), (24, True), (64, False)])
def test_perstep_estep_captured_in_a_graph_replays_the_eager_result(K, with_lengths):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import _status_word
    lib = _lib.load()
    B, T = 5, 7
    rng = np.random.default_rng(80 + K)
    init, pair, node = _problem(B, T, K, rng, False, 1.5)
    dev = torch.device("cuda")
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)      # noqa: E731
    d_init, d_pair, d_node = t(init), t(pair), t(node)
    lens = torch.tensor([T, 1, 3, T - 1, 2], dtype=torch.int32, device=dev) if with_lengths else None
    word = _status_word(dev) if with_lengths else None
    wsb = int(lib.svae_hmm_perstep_workspace_bytes(B, T, K))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    logZ = torch.empty(B, dtype=torch.float64, device=dev)
    Ei, Et, Es = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((B, K), (B, T - 1, K, K), (B, T, K)))
    p = _lib.ptr

    def launch():
        rc = lib.svae_hmm_perstep_estep_f64(B, T, K, 0, p(d_init), p(d_pair), p(d_node), p(lens), p(logZ), p(Ei), p(Et),
                                            p(Es), p(word), p(ws), wsb, _lib.current_stream(dev))
        assert rc == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture: the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in (logZ, Ei, Et, Es)]
    _check(init, pair, node, (eager[0], eager[1:]), None if lens is None else _np(lens))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for x in (logZ, Ei, Et, Es, ws):
            x.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip((logZ, Ei, Et, Es), eager))
