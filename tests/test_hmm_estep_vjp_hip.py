"""GPU tests of the HMM E-step's derivative (svae_hmm_estep_vjp_f64 / svae_hmm_ragged_estep_vjp_f64,
csrc/hmm_estep_vjp.hip; hmm_estep_differentiable) against the log-space restatement tests/_hmm_vjp_numpy.py (pinned to
torch double-backward and to the covariance over all paths by tests/test_hmm_estep_vjp_cpu.py), sequence by sequence.

Tolerances, relative to the size of phi, S = |g| + L max|cotangent| of the sequence:
  ordinary sequences           |got - want| <= 1e-8 |want| + 1e-11 S     (TOL_ORD of tests/test_hmm_range_hip.py, scaled)
  sequences flagged as redone  |got - want| <= 1e-7 |want| + 1e-9 S      (TOL_LOG of the same file, scaled)
Worst measured (this file, MI355X): ordinary 2.1e-15 S (the grid at K = 3); redone 8.7e-15 S (gap family, K = 8)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_range_numpy as rng_np  # noqa: E402
import _hmm_vjp_numpy as vjp  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)
TS = (1, 2, 3, 15, 16, 17, 33)
BS = (1, 4, 5, 9)
ORD = (1e-8, 1e-11)
LOG = (1e-7, 1e-9)


def _dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.float64, device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _problem(B, T, K, pair_batched, seed):
    """ordinary potentials (tests/test_hmm_hip.py::_problem) and all four cotangents; read-only, with its reference"""
    rng = np.random.default_rng(seed)
    init, pair, node = rng_np.ordinary(B, T, K, rng)
    if pair_batched:
        pair = np.stack([rng_np.ordinary(1, 1, K, rng)[1] for _ in range(B)])
    cot = dict(g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, K, K)),
               W=rng.standard_normal((B, T, K)))
    for x in (init, pair, node, *cot.values()):
        x.setflags(write=False)
    return init, pair, node, cot


@functools.lru_cache(maxsize=None)
def _reference(B, T, K, pair_batched, seed, which=("g", "u0", "V", "W")):
    init, pair, node, cot = _problem(B, T, K, pair_batched, seed)
    return vjp.estep_vjp_batch(init, pair, node, **{k: cot[k] for k in which})


def _scales(B, L, g=None, u0=None, V=None, W=None):
    return np.array([vjp.scale(None if g is None else g[b], None if u0 is None else u0[b], None if V is None else V[b],
                               None if W is None else W[b, :L[b]], L[b]) for b in range(B)])


def _run(init, pair, node, g=None, u0=None, V=None, W=None, lengths=None, check=False):
    """-> per-sequence (d_init, d_pair, d_node) as NumPy arrays, and the (B,) route flags"""
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_estep_vjp, vjp_redone_sequences
    B, T, K = node.shape
    ws = torch.empty(int(_lib.load().svae_hmm_estep_vjp_workspace_bytes(B, T, K)) // 8, dtype=torch.float64, device="cuda")
    out = hmm_estep_vjp((_dev(init), _dev(pair), _dev(node)), (_dev(g), (_dev(u0), _dev(V), _dev(W))), workspace=ws,
                        lengths=lengths, check=check)
    return tuple(_np(x) for x in out), _np(vjp_redone_sequences(ws, B, T, K))


def _compare(got, want, scales, redone, what, worst=None):
    """every sequence within its tolerance; returns the worst error in units of the sequence's scale"""
    w = 0.0
    for name, a, b in zip(("d_init", "d_pair", "d_node"), got, want):
        assert np.isfinite(a).all(), (what, name)
        for s in range(a.shape[0]):
            rt, at = LOG if redone[s] else ORD
            err = np.abs(a[s] - b[s])
            bound = rt * np.abs(b[s]) + at * scales[s]
            assert (err <= bound).all(), (what, name, s, bool(redone[s]), float(err.max()), float(scales[s]))
            w = max(w, float(err.max()) / max(scales[s], 1e-300))
    return w


@pytest.mark.parametrize("K", KS)
def test_all_four_cotangents_on_the_shape_grid(K):
    """every T (block and renormalisation edges), with B cycling through 1, 4, 5, 9 (a wavefront holds four rows) and the
    pair parameters alternating between shared and per-sequence"""
    worst = 0.0
    for i, T in enumerate(TS):
        for B, pb in ((BS[i % 4], i % 2 == 0), (BS[(i + 2) % 4], i % 2 == 1)):
            init, pair, node, cot = _problem(B, T, K, pb, 1000 * K + T)
            got, redone = _run(init, pair, node, **cot)
            assert not redone.any(), (K, T, B)                  # ordinary potentials stay on the scaled route
            w = _compare(got, _reference(B, T, K, pb, 1000 * K + T), _scales(B, [T] * B, **cot), redone, (K, T, B, pb))
            worst = max(worst, w)
    print("K = %d: worst error %.2e of the scale" % (K, worst))


@pytest.mark.parametrize("K", (3, 16, 17, 64))
@pytest.mark.parametrize("which", ("g", "u0", "V", "W"))
def test_each_cotangent_alone_and_null_equals_zero(K, which):
    B, T = 5, 17
    init, pair, node, cot = _problem(B, T, K, True, 77 + K)
    one = {which: cot[which]}
    got, redone = _run(init, pair, node, **one)
    _compare(got, _reference(B, T, K, True, 77 + K, (which,)), _scales(B, [T] * B, **one), redone, (K, which))
    # a NULL cotangent is a zero cotangent
    zeros = {k: (cot[k] if k == which else np.zeros_like(cot[k])) for k in cot}
    got0, _ = _run(init, pair, node, **zeros)
    sc = _scales(B, [T] * B, **one)
    for a, b in zip(got, got0):
        for s in range(B):
            assert (np.abs(a[s] - b[s]) <= 1e-8 * np.abs(b[s]) + 1e-11 * sc[s]).all()


@pytest.mark.parametrize("K", (3, 17))
def test_unbatched_input_keeps_its_shapes(K):
    from svae_amd.hmm.hmm_inference import hmm_estep_vjp
    T = 5
    init, pair, node, cot = _problem(1, T, K, False, 5 + K)
    out = hmm_estep_vjp((_dev(init), _dev(pair), _dev(node[0])),
                        (_dev(cot["g"][0]), (_dev(cot["u0"][0]), _dev(cot["V"][0]), _dev(cot["W"][0]))))
    assert [tuple(x.shape) for x in out] == [(K,), (K, K), (T, K)]
    want = _reference(1, T, K, False, 5 + K)
    _compare(tuple(_np(x)[None] for x in out), want, _scales(1, [T], **cot), [False], K)


def _left_to_right(K, T, B, seed):
    """the chain starts in state 0 and only ever stays or moves one state up: every other transition is -inf"""
    rng = np.random.default_rng(seed)
    init = np.full(K, -np.inf)
    init[0] = 0.0
    pair = np.full((K, K), -np.inf)
    for k in range(K):
        pair[k, k] = np.log(0.7)
        if k + 1 < K:
            pair[k, k + 1] = np.log(0.3)
    return init, pair, rng.standard_normal((B, T, K))


@pytest.mark.parametrize("K", (5, 20))
def test_left_to_right_chain_takes_the_log_space_route(K):
    B, T = 5, 17
    init, pair, node = _left_to_right(K, T, B, 40 + K)
    rng = np.random.default_rng(41 + K)
    cot = dict(g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, K, K)),
               W=rng.standard_normal((B, T, K)))
    got, redone = _run(init, pair, node, **cot)
    assert redone.all()
    _compare(got, vjp.estep_vjp_batch(init, pair, node, **cot), _scales(B, [T] * B, **cot), redone, K)
    d_init, d_pair, d_node = got
    assert (d_pair[:, ~np.isfinite(pair)] == 0).all() and (d_init[:, 1:] == 0).all()      # -inf potential: exactly 0
    assert (d_node[:, 0, 1:] == 0).all()               # finite cotangents at positions of probability 0: exactly 0


@pytest.mark.parametrize("K", (8, 17))
@pytest.mark.parametrize("family", ("gap", "ramp"))
def test_range_families_are_redone_in_log_space(K, family):
    keys = rng_np.gap_keys(K, 12, (745.0, 3000.0)) if family == "gap" else rng_np.ramp_keys(K)
    init, pair, node, _, _ = rng_np.stack(keys)
    B, T, _ = node.shape
    rng = np.random.default_rng(60 + K)
    cot = dict(g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, K, K)),
               W=rng.standard_normal((B, T, K)))
    got, redone = _run(init, pair, node, **cot)
    assert redone.all()
    w = _compare(got, vjp.estep_vjp_batch(init, pair, node, **cot), _scales(B, [T] * B, **cot), redone, (K, family))
    print("%s, K = %d: worst error %.2e of the scale" % (family, K, w))


@pytest.mark.parametrize("K", (5, 20))
def test_lengths(K):
    from svae_amd.hmm.hmm_inference import check_lengths_status
    B, T = 6, 9
    init, pair, node, cot = _problem(B, T, K, True, 90 + K)
    L = np.array([1, 2, T - 1, T, 3, T])
    node, W = node.copy(), cot["W"].copy()
    for b in range(B):
        node[b, L[b]:] = np.nan
        W[b, L[b]:] = np.nan
    cot = dict(cot, W=W)
    lens = torch.as_tensor(L, dtype=torch.int32, device="cuda")
    got, redone = _run(init, pair, node, lengths=lens, check=True, **cot)
    want = vjp.estep_vjp_batch(init, pair, node, lengths=L, **cot)
    sc = _scales(B, L, **cot)
    _compare(got, want, sc, redone, ("ragged", K))
    for b in range(B):
        assert (got[2][b, L[b]:] == 0).all()            # exactly 0 from the length on
        # ... and the sequence run alone, cut to its length
        alone, _ = _run(init, pair[b:b + 1], node[b:b + 1, :L[b]], g=cot["g"][b:b + 1], u0=cot["u0"][b:b + 1],
                        V=cot["V"][b:b + 1], W=W[b:b + 1, :L[b]])
        cutgot = (got[0][b:b + 1], got[1][b:b + 1], got[2][b:b + 1, :L[b]])
        _compare(cutgot, alone, sc[b:b + 1], [False], ("alone", K, b))
    # a length of 0 and of T + 1: clamped, raised by check=True, the other sequences right
    bad = L.copy()
    bad[0], bad[3] = 0, T + 1
    badlens = torch.as_tensor(bad, dtype=torch.int32, device="cuda")
    with pytest.raises(FloatingPointError):
        _run(init, pair, node, lengths=badlens, check=True, **cot)
    got2, redone2 = _run(init, pair, node, lengths=badlens, **cot)
    with pytest.raises(FloatingPointError):
        check_lengths_status()
    _compare(got2, want, sc, redone2, ("clamped", K))    # 0 -> 1 and T + 1 -> T are what sequences 0 and 3 had


@pytest.mark.parametrize("K", (4, 33))
def test_hessian_symmetry(K):
    """with g = 0 the map is the Hessian of log Z: <H v, w> = <H w, v>"""
    B, T = 4, 16
    init, pair, node, v = _problem(B, T, K, True, 300 + K)
    _, _, _, w = _problem(B, T, K, True, 301 + K)
    v, w = {k: v[k] for k in ("u0", "V", "W")}, {k: w[k] for k in ("u0", "V", "W")}
    (Hv, _), (Hw, _) = _run(init, pair, node, **v), _run(init, pair, node, **w)
    sv, sw = _scales(B, [T] * B, **v), _scales(B, [T] * B, **w)
    for b in range(B):
        lhs = sum(float((Hv[i][b] * w[k][b]).sum()) for i, k in enumerate(("u0", "V", "W")))
        rhs = sum(float((Hw[i][b] * v[k][b]).sum()) for i, k in enumerate(("u0", "V", "W")))
        tol = sum(float(((1e-8 * np.abs(Hv[i][b]) + 1e-11 * sv[b]) * np.abs(w[k][b])).sum()) +
                  float(((1e-8 * np.abs(Hw[i][b]) + 1e-11 * sw[b]) * np.abs(v[k][b])).sum())
                  for i, k in enumerate(("u0", "V", "W")))
        assert abs(lhs - rhs) <= tol, (b, lhs, rhs, tol)


@pytest.mark.parametrize("K", (3, 16, 17, 64))
def test_constant_cotangents_give_zero(K):
    """constant u0, V and W make phi the same for every path: no covariance with anything"""
    B, T = 5, 17
    init, pair, node, _ = _problem(B, T, K, False, 400 + K)
    cot = dict(u0=np.full((B, K), 0.7), V=np.full((B, K, K), -1.3), W=np.full((B, T, K), 2.1))
    got, redone = _run(init, pair, node, **cot)
    sc = _scales(B, [T] * B, **cot)
    for x in got:
        for b in range(B):
            assert (np.abs(x[b]) <= 1e-11 * sc[b]).all(), (K, b, float(np.abs(x[b]).max()), sc[b])


@pytest.mark.parametrize("K", (5, 20))
def test_autograd_layer(K):
    """hmm_estep_differentiable: the forward is hmm_estep bit for bit; g alone reproduces hmm_logZ_differentiable; shared
    parameters receive the batch sum, per-sequence pair parameters their own block"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_estep_differentiable, hmm_logZ_differentiable
    B, T = 5, 9
    for pb in (False, True):
        init, pair, node, cot = _problem(B, T, K, pb, 500 + K)
        ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node))
        logZ, (Ei, Et, Es) = hmm_estep_differentiable((ti, tp, tn))
        lz0, (ei0, et0, es0) = hmm_estep((ti, tp, tn))
        assert torch.equal(logZ, lz0) and torch.equal(Ei, ei0) and torch.equal(Et, et0) and torch.equal(Es, es0)
        loss = (logZ * _dev(cot["g"])).sum() + (Ei * _dev(cot["u0"])).sum() + (Et * _dev(cot["V"])).sum() \
            + (Es * _dev(cot["W"])).sum()
        loss.backward()
        wi, wp, wn = _reference(B, T, K, pb, 500 + K)
        sc = _scales(B, [T] * B, **cot)
        assert tp.grad.shape == tp.shape and ti.grad.shape == ti.shape and tn.grad.shape == tn.shape
        _compare((np.zeros((B, 1)), np.zeros((B, 1)), _np(tn.grad)), (np.zeros((B, 1)), np.zeros((B, 1)), wn), sc,
                 [False] * B, "node")
        bound = lambda want: 1e-8 * np.abs(want).sum(0) + 1e-11 * sc.sum()          # noqa: E731  (a sum of B terms)
        assert (np.abs(_np(ti.grad) - wi.sum(0)) <= bound(wi)).all()
        if pb:
            _compare((np.zeros((B, 1)), _np(tp.grad), np.zeros((B, 1))), (np.zeros((B, 1)), wp, np.zeros((B, 1))), sc,
                     [False] * B, "pair")
        else:
            assert (np.abs(_np(tp.grad) - wp.sum(0)) <= bound(wp)).all()
        # g alone: the node gradient of the existing first-order path
        tn2 = _dev(node).requires_grad_()
        (hmm_logZ_differentiable((_dev(init), _dev(pair), tn2)) * _dev(cot["g"])).sum().backward()
        tn3 = _dev(node).requires_grad_()
        (hmm_estep_differentiable((_dev(init), _dev(pair), tn3))[0] * _dev(cot["g"])).sum().backward()
        a, b = _np(tn3.grad), _np(tn2.grad)
        assert (np.abs(a - b) <= 1e-8 * np.abs(b) + 1e-11 * np.abs(cot["g"])[:, None, None]).all()


def test_autograd_unbatched_and_lengths():
    from svae_amd.hmm.hmm_inference import hmm_estep_differentiable
    K, T = 4, 6
    init, pair, node, cot = _problem(3, T, K, False, 600)
    ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node[0]))
    logZ, (Ei, Et, Es) = hmm_estep_differentiable((ti, tp, tn))
    assert logZ.dim() == 0 and Es.shape == (T, K)
    (logZ * cot["g"][0] + (Ei * _dev(cot["u0"][0])).sum() + (Et * _dev(cot["V"][0])).sum()
     + (Es * _dev(cot["W"][0])).sum()).backward()
    wi, wp, wn = vjp.estep_vjp(init, pair, node[0], cot["g"][0], cot["u0"][0], cot["V"][0], cot["W"][0])
    s = vjp.scale(cot["g"][0], cot["u0"][0], cot["V"][0], cot["W"][0], T)
    for got, want in ((ti.grad, wi), (tp.grad, wp), (tn.grad, wn)):
        assert got.shape == want.shape and (np.abs(_np(got) - want) <= 1e-8 * np.abs(want) + 1e-11 * s).all()
    # lengths=: the gradient of every sequence cut to its length, exactly 0 behind it
    L = np.array([6, 1, 4])
    tn = _dev(node).requires_grad_()
    logZ, (_, _, Es) = hmm_estep_differentiable((_dev(init), _dev(pair), tn), lengths=L, check=True)
    Wm = cot["W"].copy()
    for b in range(3):
        Wm[b, L[b]:] = 0.0
    ((Es * _dev(Wm)).sum() + logZ.sum()).backward()
    _, _, wn = vjp.estep_vjp_batch(init, pair, node, lengths=L, g=np.ones(3), W=cot["W"])
    sc = _scales(3, L, g=np.ones(3), W=cot["W"])
    _compare((np.zeros((3, 1)), np.zeros((3, 1)), _np(tn.grad)), (np.zeros((3, 1)), np.zeros((3, 1)), wn), sc, [False] * 3,
             "ragged node")
    for b in range(3):
        assert (_np(tn.grad)[b, L[b]:] == 0).all()


def test_gradcheck():
    from svae_amd.hmm.hmm_inference import hmm_estep_differentiable
    K, T, B = 3, 4, 2
    init, pair, node, _ = _problem(B, T, K, False, 700)

    def f(i, p, n):
        logZ, (Ei, Et, Es) = hmm_estep_differentiable((i, p, n))
        return logZ, Ei, Et, Es

    ti, tp, tn = (_dev(x).requires_grad_() for x in (init, pair, node))
    assert torch.autograd.gradcheck(f, (ti, tp, tn), eps=1e-6, atol=1e-7, rtol=1e-5)
    tpb = _dev(np.stack([pair, pair + 0.1])).requires_grad_()
    assert torch.autograd.gradcheck(f, (ti, tpb, tn), eps=1e-6, atol=1e-7, rtol=1e-5)
