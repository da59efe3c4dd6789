"""GPU tests of the derivative of the HMM E-step with per-step transition potentials (svae_hmm_perstep_estep_vjp_f64,
csrc/hmm_estep_perstep_vjp.hip; hmm_estep_perstep_vjp, hmm_estep_perstep_differentiable) against the log-space
restatement tests/_hmm_perstep_vjp_numpy.py (pinned to torch double-backward, to the covariance over all paths and to
tests/_hmm_vjp_numpy.py by tests/test_hmm_perstep_vjp_cpu.py), sequence by sequence.

Tolerance, relative to the size of phi, S = |g| + L max|cotangent| of the sequence: the kernel has ONE route, log space
throughout, so every comparison is  |got - want| <= 1e-7 |want| + 1e-9 S  (the log-space bound of
tests/test_hmm_estep_vjp_hip.py), with everything finite.
Worst measured (this file, MI355X), in units of S: the shape grid 3.7e-16 (K = 2); one cotangent alone 1.2e-15 (g, K = 17);
the range families 1.1e-13 (entries 800 nats deep, K = 24; per-step offsets 1.8e-14); lengths 2.4e-16 (K = 3)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_perstep_vjp_numpy as pvjp  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)
TS = (1, 2, 3, 7, 37)
BS = (1, 5, 9)
RTOL, ATOL = 1e-7, 1e-9
NAMES = ("g", "u0", "V", "W")


def _dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.float64, device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _potentials(B, T, K, rng, pair_batched, scale=1.0):
    """tests/test_hmm_perstep_hip.py::_problem: every step's matrix at its own offset"""
    init = np.log(rng.dirichlet(np.ones(K)))
    lead = (B, T - 1) if pair_batched else (T - 1,)
    pair = np.log(rng.dirichlet(np.ones(K), size=lead + (K,))) + 0.5 * rng.standard_normal(lead + (K, K))
    pair = pair + 3.0 * rng.standard_normal(lead + (1, 1))
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


def _cotangents(B, T, K, rng):
    return dict(g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, T - 1, K, K)),
                W=rng.standard_normal((B, T, K)))


@functools.lru_cache(maxsize=None)
def _problem(B, T, K, pair_batched, seed):
    """potentials and all four cotangents; read-only, shared among the tests"""
    rng = np.random.default_rng(seed)
    init, pair, node = _potentials(B, T, K, rng, pair_batched, 1.5)
    cot = _cotangents(B, T, K, rng)
    for x in (init, pair, node, *cot.values()):
        x.setflags(write=False)
    return init, pair, node, cot


@functools.lru_cache(maxsize=None)
def _reference(B, T, K, pair_batched, seed, which=NAMES):
    init, pair, node, cot = _problem(B, T, K, pair_batched, seed)
    return pvjp.estep_perstep_vjp_batch(init, pair, node, **{k: cot[k] for k in which})


def _scales(B, L, g=None, u0=None, V=None, W=None):
    return np.array([pvjp.scale(None if g is None else g[b], None if u0 is None else u0[b],
                                None if V is None else V[b, :L[b] - 1], None if W is None else W[b, :L[b]], L[b])
                     for b in range(B)])


def _run_t(init, pair, node, g=None, u0=None, V=None, W=None, **kw):
    from svae_amd.hmm import hmm_estep_perstep_vjp
    return hmm_estep_perstep_vjp((_dev(init), _dev(pair), _dev(node)), (_dev(g), (_dev(u0), _dev(V), _dev(W))), **kw)


def _run(*a, **kw):
    return tuple(None if x is None else _np(x) for x in _run_t(*a, **kw))


def _compare(got, want, scales, what):
    """every sequence within the bound, everything finite; returns the worst error in units of the sequence's scale"""
    w = 0.0
    for name, a, b in zip(("d_init", "d_pair", "d_node"), got, want):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert np.isfinite(a).all(), (what, name)
        for s in range(a.shape[0]):
            if a[s].size == 0:
                continue
            err = np.abs(a[s] - b[s])
            bound = RTOL * np.abs(b[s]) + ATOL * scales[s]
            assert (err <= bound).all(), (what, name, s, float(err.max()), float(scales[s]))
            w = max(w, float(err.max()) / max(scales[s], 1e-300))
    return w


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b) if x is not None and y is not None)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_all_four_cotangents_on_the_shape_grid(K):
    """T = 1 (no pair step at all) and both sides of the unroll-by-4 trip counts, B with partly filled wavefronts at
    8, 4, 2 and 1 sequences per wavefront, shared and per-sequence pair parameters"""
    worst = 0.0
    for T in TS:
        for B in BS:
            for pb in (False, True):
                seed = 100000 * K + 100 * T + 10 * B + pb
                init, pair, node, cot = _problem(B, T, K, pb, seed)
                got = _run(init, pair, node, **cot)
                w = _compare(got, _reference(B, T, K, pb, seed), _scales(B, [T] * B, **cot), (K, T, B, pb))
                worst = max(worst, w)
    print("K = %d: worst error %.2e of the scale" % (K, worst))


@pytest.mark.parametrize("K", (3, 17))
def test_unbatched_input_keeps_its_shapes(K):
    T = 7
    init, pair, node, cot = _problem(1, T, K, False, 5 + K)
    out = _run(init, pair, node[0], cot["g"][0], cot["u0"][0], cot["V"][0], cot["W"][0])
    assert [x.shape for x in out] == [(K,), (T - 1, K, K), (T, K)]
    _compare(tuple(x[None] for x in out), _reference(1, T, K, False, 5 + K), _scales(1, [T], **cot), K)
    lean = _run(init, pair, node[0], cot["g"][0], cot["u0"][0], cot["V"][0], cot["W"][0], want_pair=False)
    assert lean[1] is None and np.array_equal(lean[0], out[0]) and np.array_equal(lean[2], out[2])


# ---- 2. each cotangent alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 16, 17, 64))
@pytest.mark.parametrize("which", NAMES)
def test_each_cotangent_alone_and_none_equals_zero_bit_for_bit(K, which):
    B, T = 5, 7
    init, pair, node, cot = _problem(B, T, K, True, 77 + K)
    one = {which: cot[which]}
    got = _run_t(init, pair, node, **one)
    w = _compare(tuple(_np(x) for x in got), _reference(B, T, K, True, 77 + K, (which,)), _scales(B, [T] * B, **one),
                 (K, which))
    print("K = %d, %s alone: worst error %.2e of the scale" % (K, which, w))
    zeros = {k: (cot[k] if k == which else np.zeros_like(cot[k])) for k in cot}
    assert _same(got, _run_t(init, pair, node, **zeros))


# ---- 3. without d_pair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 8, 16, 17, 33, 64))
def test_without_d_pair_the_other_gradients_keep_their_bits(K):
    B, T = 5, 7
    for pb in (False, True):
        init, pair, node, cot = _problem(B, T, K, pb, 150 + K)
        full = _run_t(init, pair, node, **cot)
        lean = _run_t(init, pair, node, want_pair=False, **cot)
        assert lean[1] is None and torch.equal(lean[0], full[0]) and torch.equal(lean[2], full[2])
        noV = dict(cot, V=None)                                          # ... and without g_trans as well
        full = _run_t(init, pair, node, **noV)
        lean = _run_t(init, pair, node, want_pair=False, **noV)
        assert lean[1] is None and torch.equal(lean[0], full[0]) and torch.equal(lean[2], full[2])


# ---- 4. range -------------------------------------------------------------------------------------------------------------------
def _range_case(case, B, T, K, rng):
    """the four families of tests/test_hmm_perstep_hip.py::_range_case"""
    init, pair, node = _potentials(B, T, K, rng, True, 1.0)
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
def test_the_restatement_holds_over_the_whole_domain(case, K):
    B, T = 3, 9
    rng = np.random.default_rng(5000 + K)
    init, pair, node = _range_case(case, B, T, K, rng)
    cot = _cotangents(B, T, K, rng)
    got = _run(init, pair, node, **cot)
    w = _compare(got, pvjp.estep_perstep_vjp_batch(init, pair, node, **cot), _scales(B, [T] * B, **cot), (case, K))
    print("%s, K = %d: worst error %.2e of the scale" % (case, K, w))
    assert (got[1][~np.isfinite(pair)] == 0.0).all()                     # a -inf potential: exactly 0
    if case == "forbidden_stretch":
        assert (got[2][:, 2:6, K - 1] == 0.0).all() and got[2][1, 0, 0] == 0.0 and got[0][1, 0] == 0.0
    # a sequence's results do not depend on its neighbours: alone, bit for bit
    alone = _run(init, pair[1:2], node[1:2], **{k: v[1:2] for k, v in cot.items()})
    assert all(np.array_equal(a[0], x[1]) for a, x in zip(alone, got))


# ---- 5. constant matrices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 16, 17, 64))
def test_reduces_to_the_uniform_derivative_at_constant_matrices(K):
    from svae_amd.hmm import hmm_estep_vjp
    B, T = 5, 7
    rng = np.random.default_rng(4000 + K)
    init = np.log(rng.dirichlet(np.ones(K)))
    P = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    node = 1.5 * rng.standard_normal((B, T, K))
    g, u0, V, W = (rng.standard_normal(s) for s in ((B,), (B, K), (B, K, K), (B, T, K)))
    Vt = np.broadcast_to(V[:, None], (B, T - 1, K, K)).copy()
    di, dp, dn = _run(init, np.broadcast_to(P, (T - 1, K, K)).copy(), node, g, u0, Vt, W)
    ui, up, un = (_np(x) for x in hmm_estep_vjp((_dev(init), _dev(P), _dev(node)), (_dev(g), (_dev(u0), _dev(V), _dev(W)))))
    sc = _scales(B, [T] * B, g, u0, Vt, W)
    _compare((di, dp.sum(1), dn), (ui, up, un), sc, K)


# ---- 6. lengths -----------------------------------------------------------------------------------------------------------------
def _padded(x, lengths, off):
    """a copy with steps >= L - off replaced by NaN"""
    x = np.array(x)
    for b, L in enumerate(lengths):
        x[b, L - off:] = np.nan
    return x


@pytest.mark.parametrize("K", [3, 8, 16, 17, 33, 64])
def test_lengths_against_the_restatement_on_the_cut_sequences(K):
    from svae_amd.hmm.hmm_inference import check_lengths_status
    B, T = 9, 12
    try:
        check_lengths_status()                                           # start from a clean word
    except FloatingPointError:
        pass
    rng = np.random.default_rng(6000 + K)
    lengths = np.array([1, 2, T - 1, T] + list(rng.integers(1, T + 1, B - 4)))
    init, pair, node, cot = _problem(B, T, K, True, 6100 + K)
    pad = lambda L: (_padded(pair, L, 1), _padded(node, L, 0),           # noqa: E731
                     dict(cot, V=_padded(cot["V"], L, 1), W=_padded(cot["W"], L, 0)))
    n_pair, n_node, n_cot = pad(lengths)
    got = _run_t(init, n_pair, n_node, lengths=lengths, check=True, **n_cot)
    want = pvjp.estep_perstep_vjp_batch(init, pair, node, lengths=lengths, **cot)
    sc = _scales(B, lengths, **cot)
    gn = tuple(_np(x) for x in got)
    w = _compare(gn, want, sc, ("lengths", K))
    print("lengths, K = %d: worst error %.2e of the scale" % (K, w))
    for b, L in enumerate(lengths):                                      # the tails: exactly +0.0
        assert (gn[2][b, L:] == 0.0).all() and not np.signbit(gn[2][b, L:]).any()
        assert (gn[1][b, L - 1:] == 0.0).all() and not np.signbit(gn[1][b, L - 1:]).any()
    lean = _run_t(init, n_pair, n_node, lengths=torch.tensor(lengths), want_pair=False, **n_cot)
    assert lean[1] is None and torch.equal(lean[0], got[0]) and torch.equal(lean[2], got[2])
    # shared pair parameters (finite everywhere: another sequence may need the step), everything else NaN behind L
    shared = _run(init, pair[0], n_node, lengths=lengths, **n_cot)
    _compare(shared, pvjp.estep_perstep_vjp_batch(init, pair[0], node, lengths=lengths, **cot), sc, ("shared", K))
    # no sequence sees another's length: the other sequences' lengths permuted, sequence by sequence the same bits
    perm = rng.permutation(B)
    got_p = _run_t(init, n_pair[perm], n_node[perm], lengths=lengths[perm], **{k: v[perm] for k, v in n_cot.items()})
    idx = torch.as_tensor(perm, device="cuda")
    assert _same(got_p, tuple(x[idx] for x in got))
    other = lengths.copy()
    other[1:] = other[1:][::-1]                                          # sequence 0 keeps L = 1, its wavefront's lengths move
    o_pair, o_node, o_cot = pad(other)
    got_o = _run_t(init, o_pair, o_node, lengths=other, **o_cot)
    assert _same(tuple(x[:1] for x in got_o), tuple(x[:1] for x in got))
    # a length of 0 and a length of T + 3: clamped, and reported through check=True
    bad = lengths.copy()
    bad[0], bad[3] = 0, T + 3
    with pytest.raises(FloatingPointError):
        _run_t(init, n_pair, n_node, lengths=bad, check=True, **n_cot)
    got_b = _run_t(init, n_pair, n_node, lengths=bad, **n_cot)           # check=False: no synchronisation, no error
    with pytest.raises(FloatingPointError):
        check_lengths_status()
    assert _same(got_b, got)                                             # 0 -> 1 and T + 3 -> T are what sequences 0 and 3 had
    _run_t(init, n_pair, n_node, lengths=lengths, check=True, **n_cot)   # the word was cleared: a clean call stays clean


# ---- 7. the autograd function ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (5, 20))
def test_autograd_layer(K):
    """the forward is hmm_estep_perstep bit for bit; shared parameters receive the batch sum of the per-sequence
    gradients, per-sequence pair parameters their own block; without a pair gradient the others keep their bits"""
    from svae_amd.hmm import hmm_estep_perstep_differentiable
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep
    B, T = 5, 7
    for pb in (False, True):
        init, pair, node, cot = _problem(B, T, K, pb, 500 + K)
        lengths = None if pb else np.array([T, 1, 3, T - 1, 2])
        ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node))
        logZ, (Ei, Et, Es) = hmm_estep_perstep_differentiable((ti, tp, tn), lengths=lengths, check=True)
        lz0, (ei0, et0, es0) = hmm_estep_perstep((ti, tp, tn), lengths=lengths)
        assert torch.equal(logZ, lz0) and torch.equal(Ei, ei0) and torch.equal(Et, et0) and torch.equal(Es, es0)
        loss = lambda lz, ei, et, es: ((lz * _dev(cot["g"])).sum() + (ei * _dev(cot["u0"])).sum()          # noqa: E731
                                       + (et * _dev(cot["V"])).sum() + (es * _dev(cot["W"])).sum())
        loss(logZ, Ei, Et, Es).backward()
        di, dp, dn = _run_t(init, pair, node, lengths=lengths, **cot)
        assert tp.grad.shape == tp.shape and ti.grad.shape == ti.shape and tn.grad.shape == tn.shape
        assert torch.equal(tn.grad, dn) and torch.equal(ti.grad, di.sum(0))
        assert torch.equal(tp.grad, dp if pb else dp.sum(0))
        want = pvjp.estep_perstep_vjp_batch(init, pair, node, lengths=lengths, **cot)
        _compare((_np(di), _np(dp), _np(dn)), want, _scales(B, [T] * B if lengths is None else lengths, **cot), (K, pb))
        # the recognition-network case: the pair parameters need no gradient
        ui, un = (_dev(x).requires_grad_() for x in (init, node))
        up = _dev(pair)
        lz, (ei, et, es) = hmm_estep_perstep_differentiable((ui, up, un), lengths=lengths)
        loss(lz, ei, et, es).backward()
        assert up.grad is None and torch.equal(ui.grad, ti.grad) and torch.equal(un.grad, tn.grad)


def test_autograd_unbatched():
    from svae_amd.hmm import hmm_estep_perstep_differentiable
    K, T = 4, 6
    init, pair, node, cot = _problem(1, T, K, False, 600)
    ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node[0]))
    logZ, (Ei, Et, Es) = hmm_estep_perstep_differentiable((ti, tp, tn))
    assert logZ.dim() == 0 and Ei.shape == (K,) and Et.shape == (T - 1, K, K) and Es.shape == (T, K)
    (logZ * cot["g"][0] + (Ei * _dev(cot["u0"][0])).sum() + (Et * _dev(cot["V"][0])).sum()
     + (Es * _dev(cot["W"][0])).sum()).backward()
    want = _reference(1, T, K, False, 600)
    _compare(tuple(_np(x.grad)[None] for x in (ti, tp, tn)), want, _scales(1, [T], **cot), "unbatched")


@pytest.mark.parametrize("pair_batched", [False, True])
@pytest.mark.parametrize("with_lengths", [False, True])
def test_gradcheck(pair_batched, with_lengths):
    from svae_amd.hmm import hmm_estep_perstep_differentiable
    B, T, K = 2, 4, 3
    init, pair, node, cot = _problem(B, T, K, pair_batched, 700 + 2 * pair_batched + with_lengths)
    lengths = np.array([2, T]) if with_lengths else None
    mask = np.ones((B, T, 1))
    if with_lengths:
        mask[0, 2:] = 0.0                      # outputs behind a length are constants: the scalar weights them by 0
    g, u0, V, W = (_dev(x) for x in (cot["g"], cot["u0"], cot["V"] * mask[:, 1:, :, None], cot["W"] * mask))

    def f(i, p, n):
        logZ, (Ei, Et, Es) = hmm_estep_perstep_differentiable((i, p, n), lengths=lengths)
        return (logZ * g).sum() + (Ei * u0).sum() + (Et * V).sum() + (torch.sin(Es) * W).sum() + (Et * Et).sum()

    ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node))
    assert torch.autograd.gradcheck(f, (ti, tp, tn), eps=1e-6, atol=1e-7, rtol=1e-5)


# ---- 8. capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,with_lengths", [(8, False), (24, True), (64, False)])
def test_captured_in_a_graph_replays_the_eager_result(K, with_lengths):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import _status_word
    lib = _lib.load()
    B, T = 5, 7
    init, pair, node, cot = _problem(B, T, K, False, 80 + K)
    dev = torch.device("cuda")
    d_in = [_dev(x) for x in (init, pair, node, cot["g"], cot["u0"], cot["V"], cot["W"])]
    lens = torch.tensor([T, 1, 3, T - 1, 2], dtype=torch.int32, device=dev) if with_lengths else None
    word = _status_word(dev) if with_lengths else None
    wsb = int(lib.svae_hmm_perstep_estep_vjp_workspace_bytes(B, T, K))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    di, dp, dn = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((B, K), (B, T - 1, K, K), (B, T, K)))
    p = _lib.ptr

    def launch():
        rc = lib.svae_hmm_perstep_estep_vjp_f64(B, T, K, 0, p(d_in[0]), p(d_in[1]), p(d_in[2]), p(lens), p(d_in[3]),
                                                p(d_in[4]), p(d_in[5]), p(d_in[6]), p(di), p(dp), p(dn), p(word), p(ws),
                                                wsb, _lib.current_stream(dev))
        assert rc == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture: the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in (di, dp, dn)]
    L = [T] * B if lens is None else list(_np(lens))
    want = pvjp.estep_perstep_vjp_batch(init, pair, node, lengths=L, **cot)
    _compare(tuple(_np(x) for x in eager), want, _scales(B, L, **cot), ("eager", K))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for x in (di, dp, dn, ws):
            x.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip((di, dp, dn), eager))
