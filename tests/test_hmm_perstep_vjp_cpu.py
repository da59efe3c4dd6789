"""CPU tests of the derivative of the HMM E-step with per-step transition potentials (svae_hmm_perstep_estep_vjp_f64,
hmm_estep_perstep_vjp, hmm_estep_perstep_differentiable).

The arithmetic: the NumPy restatement tests/_hmm_perstep_vjp_numpy.py -- the reference of the GPU file -- against torch
fp64 double-backward through the per-step logsumexp chain (finite potentials), against the covariance taken directly
over all K^T paths (K <= 3, T <= 5, -inf entries, an all -inf row and an all -inf column included: there enumeration is
the arbiter, torch returns NaN), against tests/_hmm_vjp_numpy.estep_vjp at constant P_t, V_t, and, with g = 1 alone,
against the statistics of tests/_hmm_perstep_numpy.hmm_estep_perstep.
Tolerance of all four: 1e-12 S, S = |g| + L max|cotangent|, the size of phi (scale(); the bound of
tests/test_hmm_estep_vjp_cpu.py).

The C ABI and the Python layer without a GPU: the symbols (ABI number still 15), the workspace formula, every argument
code (decided on the host before any HIP call) and the shape refusals (raised before anything is converted)."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_perstep_numpy as ps  # noqa: E402
import _hmm_perstep_vjp_numpy as pvjp  # noqa: E402
import _hmm_vjp_numpy as vjp  # noqa: E402

NAMES = ("svae_hmm_perstep_estep_vjp_workspace_bytes", "svae_hmm_perstep_estep_vjp_f64")


def _problem(K, T, seed, forbid=None):
    rng = np.random.default_rng(seed)
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=(T - 1, K))) + 0.3 * rng.standard_normal((T - 1, K, K))
    pair = pair + 3.0 * rng.standard_normal((T - 1, 1, 1))              # every step at its own offset
    node = rng.standard_normal((T, K))
    if T > 1 and K > 1:
        if forbid == "entry":
            pair[0, 0, K - 1] = -np.inf
            pair[T - 2, K - 1, 0] = -np.inf
        elif forbid == "row":                   # state 0 at step T-2 has no way on: gamma_{T-2}[0] = 0
            pair[T - 2, 0, :] = -np.inf
        elif forbid == "column":                # state K-1 at step 1 cannot be reached: gamma_1[K-1] = 0
            pair[0, :, K - 1] = -np.inf
        elif forbid == "node":
            node[T // 2, 0] = -np.inf
        elif forbid == "all":                   # an all -inf column, an all -inf row and a -inf node entry at once
            pair[0, :, K - 1] = -np.inf
            pair[T - 2, 0, :] = -np.inf
            node[T - 1, K - 1] = -np.inf
    cot = dict(g=float(rng.standard_normal()), u0=rng.standard_normal(K), V=rng.standard_normal((T - 1, K, K)),
               W=rng.standard_normal((T, K)))
    return init, pair, node, cot


def _check(got, want, tol, what):
    for name, a, b in zip(("init", "pair", "node"), got, want):
        assert np.isfinite(a).all(), (what, name)
        err = float(np.max(np.abs(a - b))) if a.size else 0.0
        assert err <= tol, (what, name, err, tol)


def _torch_double_backward(init, pair, node, g, u0, V, W):
    ti, tp, tn = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (init, pair, node))
    al = ti + tn[0]
    for t in range(1, node.shape[0]):
        al = torch.logsumexp(al[:, None] + tp[t - 1], 0) + tn[t]
    logZ = torch.logsumexp(al, 0)
    Ei, Et, Es = torch.autograd.grad(logZ, (ti, tp, tn), create_graph=True, allow_unused=True)
    loss = g * logZ + (torch.tensor(u0) * Ei).sum() + (torch.tensor(W) * Es).sum()
    if Et is not None:                       # (T = 1: log Z does not depend on the pair parameters)
        loss = loss + (torch.tensor(V) * Et).sum()
    gi, gp, gn = torch.autograd.grad(loss, (ti, tp, tn), allow_unused=True)
    gp = torch.zeros_like(tp) if gp is None else gp
    return gi.numpy(), gp.numpy(), gn.numpy()


@pytest.mark.parametrize("K,T", [(K, T) for K in (1, 2, 3, 5, 17) for T in (1, 2, 3, 7)])
def test_restatement_equals_torch_double_backward(K, T):
    init, pair, node, cot = _problem(K, T, 100 * K + T)
    want = _torch_double_backward(init, pair, node, **cot)
    got = pvjp.estep_perstep_vjp(init, pair, node, **cot)
    _check(got, want, 1e-12 * pvjp.scale(cot["g"], cot["u0"], cot["V"], cot["W"], T), (K, T))


def _brute_force(init, pair, node, g, u0, V, W):
    T, K = node.shape
    paths = list(itertools.product(range(K), repeat=T))
    score = np.array([init[z[0]] + sum(node[t, z[t]] for t in range(T)) + sum(pair[t, z[t], z[t + 1]] for t in range(T - 1))
                      for z in paths])
    p = np.exp(score - score.max())
    p /= p.sum()
    phi = np.array([u0[z[0]] + sum(W[t, z[t]] for t in range(T)) + sum(V[t, z[t], z[t + 1]] for t in range(T - 1))
                    for z in paths])
    c = p * (g + phi - p @ phi)              # E[f (g + phi - E phi)] = g E[f] + Cov(f, phi)
    gn, gp = np.zeros((T, K)), np.zeros((T - 1, K, K))
    for z, cz in zip(paths, c):
        for t in range(T):
            gn[t, z[t]] += cz
        for t in range(T - 1):
            gp[t, z[t], z[t + 1]] += cz
    return gn[0].copy(), gp, gn


@pytest.mark.parametrize("K,T,forbid", [(K, T, f) for K in (1, 2, 3) for T in (1, 2, 3, 4, 5)
                                        for f in (None, "entry", "row", "column", "node", "all")
                                        if f is None or (K > 1 and T > 1 and (f != "all" or K == 3))])
def test_restatement_equals_the_covariance_over_all_paths(K, T, forbid):
    """(the exclusions need K > 1 and T > 1; all three at once leave a path only at K = 3)"""
    init, pair, node, cot = _problem(K, T, 500 + 10 * K + T, forbid)
    with np.errstate(all="ignore"):
        want = _brute_force(init, pair, node, **cot)
    assert np.isfinite(want[2]).all()                                    # (the case leaves a path: log Z is finite)
    got = pvjp.estep_perstep_vjp(init, pair, node, **cot)
    _check(got, want, 1e-12 * pvjp.scale(cot["g"], cot["u0"], cot["V"], cot["W"], T), (K, T, forbid))
    assert (got[1][~np.isfinite(pair)] == 0.0).all()                     # a -inf potential has gradient exactly 0


@pytest.mark.parametrize("K,T", [(1, 4), (2, 2), (3, 9), (5, 6), (17, 5)])
@pytest.mark.parametrize("forbid", [False, True])
def test_restatement_reduces_to_the_uniform_one_at_constant_matrices(K, T, forbid):
    rng = np.random.default_rng(900 + 10 * K + T)
    init = np.log(rng.dirichlet(np.ones(K)))
    P = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    if forbid and K > 1:
        P[0, K - 1] = -np.inf
    node = rng.standard_normal((T, K))
    cot = dict(g=float(rng.standard_normal()), u0=rng.standard_normal(K), V=rng.standard_normal((K, K)),
               W=rng.standard_normal((T, K)))
    wi, wp, wn = vjp.estep_vjp(init, P, node, **cot)
    bc = lambda x: np.broadcast_to(x, (T - 1, K, K)).copy()              # noqa: E731
    gi, gp, gn = pvjp.estep_perstep_vjp(init, bc(P), node, **dict(cot, V=bc(cot["V"])))
    _check((gi, gp.sum(0), gn), (wi, wp, wn), 1e-12 * vjp.scale(cot["g"], cot["u0"], cot["V"], cot["W"], T), (K, T))


@pytest.mark.parametrize("K,T,forbid", [(1, 1, None), (1, 3, None), (2, 2, "entry"), (3, 5, "all"), (5, 7, None),
                                        (5, 7, "row"), (17, 4, "column")])
def test_g_alone_gives_the_statistics(K, T, forbid):
    init, pair, node, _ = _problem(K, T, 1300 + 10 * K + T, forbid)
    gi, gp, gn = pvjp.estep_perstep_vjp(init, pair, node, g=1.0)
    _, (Ei, Et, Es) = ps.hmm_estep_perstep((init, pair, node))
    _check((gi, gp, gn), (Ei, Et, Es), 1e-12, (K, T, forbid))            # S = |g| = 1


def test_batch_form_cuts_each_sequence_to_its_length():
    rng = np.random.default_rng(3)
    B, T, K = 3, 5, 3
    init = _problem(K, T, 9)[0]
    pair = np.stack([_problem(K, T, 10 + b)[1] for b in range(B)])
    node = rng.standard_normal((B, T, K))
    V, W = rng.standard_normal((B, T - 1, K, K)), rng.standard_normal((B, T, K))
    L = np.array([5, 1, 3])
    for b in range(B):
        node[b, L[b]:] = np.nan
        W[b, L[b]:] = np.nan
        pair[b, L[b] - 1:] = np.nan
        V[b, L[b] - 1:] = np.nan
    di, dp, dn = pvjp.estep_perstep_vjp_batch(init, pair, node, lengths=L, g=np.ones(B), V=V, W=W)
    assert np.isfinite(di).all() and np.isfinite(dp).all() and np.isfinite(dn).all()
    assert (dn[1, 1:] == 0).all() and (dn[2, 3:] == 0).all() and (dp[1] == 0).all() and (dp[2, 2:] == 0).all()
    one = pvjp.estep_perstep_vjp(init, pair[2, :2], node[2, :3], g=1.0, V=V[2, :2], W=W[2, :3])
    assert np.array_equal(one[2], dn[2, :3]) and np.array_equal(one[1], dp[2, :2]) and np.array_equal(one[0], di[2])
    shared = pvjp.estep_perstep_vjp_batch(init, pair[0], node, lengths=L, V=V, W=W)
    assert all(np.isfinite(x).all() for x in shared)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_symbols_are_declared_bound_and_exported_without_a_new_abi_number():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s


@pytest.mark.parametrize("K", [1, 3, 8, 16, 17, 33, 64])
def test_workspace_bytes_closed_form(K):
    """B T records of [la_t | r_t] = 2 K doubles, rounded up to 128 bytes"""
    _, lib = _lib()
    for B, T in ((1, 1), (3, 2), (5, 7), (1, 3), (7, 5), (2048, 500)):
        got = lib.svae_hmm_perstep_estep_vjp_workspace_bytes(B, T, K)
        assert got == -(-(B * T * 2 * K) * 8 // 128) * 128 and got % 16 == 0
        assert got >= 2 * (lib.svae_hmm_perstep_workspace_bytes(B, T, K) - 127)


def test_workspace_bytes_out_of_range_is_zero():
    _, lib = _lib()
    for B, T, K in ((0, 5, 3), (-1, 5, 3), (2, 0, 3), (2, -4, 3), (2, 5, 0), (2, 5, -1), (2, 5, 65), (2, 5, 1000)):
        assert lib.svae_hmm_perstep_estep_vjp_workspace_bytes(B, T, K) == 0


def test_vjp_rejects_bad_arguments_on_the_host_in_order():
    _, lib = _lib()
    raw = (ctypes.c_double * 4096)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    p = ctypes.c_void_p(base)                 # 16-byte aligned host address: must never be dereferenced
    need = lib.svae_hmm_perstep_estep_vjp_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, g0=None, g1=None, g2=None, g3=None, di=p, dp=p,
             dn=p, info=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_perstep_estep_vjp_f64(B, T, K, pb, init, pair, node, lengths, g0, g1, g2, g3, di, dp, dn, info,
                                                  ws, ws_bytes, None)

    bad = [dict(B=-1), dict(T=0), dict(K=0), dict(pb=2), dict(init=None), dict(pair=None), dict(node=None),
           dict(di=None), dict(dn=None), dict(info=None), dict(ws=None), dict(ws_bytes=need - 1),
           dict(ws=ctypes.c_void_p(base + 8))]
    for i, kw in enumerate(bad):
        assert call(**kw) == -(i + 1), kw
        merged = {}                           # the first failing check decides: every later argument bad as well
        for later in bad[i:]:
            merged = {**later, **merged}
        assert call(**merged) == -(i + 1), merged
    assert call(T=-3) == -2 and call(K=65) == -3 and call(pb=-1) == -4 and call(ws_bytes=0) == -12
    assert call(T=1, pair=None, init=None) == -5          # T = 1 reads no pair parameters: the next check decides
    assert call(T=1, pair=None, node=None) == -7
    # an empty batch returns 0 after the checks it shares with every batch
    n = (None,) * 4
    f = lib.svae_hmm_perstep_estep_vjp_f64
    assert f(0, 3, 5, 0, p, p, None, None, *n, None, None, None, None, None, 0, None) == 0
    assert f(0, 3, 5, 1, p, p, None, None, *n, None, None, None, None, None, 0, None) == 0
    assert f(0, 0, 5, 0, p, p, None, None, *n, None, None, None, None, None, 0, None) == -2
    assert f(0, 3, 5, 0, p, None, None, None, *n, None, None, None, None, None, 0, None) == -6


# ---- the Python layer's refusals (before anything is converted or launched: no GPU needed) ---------------------------------
def test_python_layer_refuses_wrong_shapes_before_any_launch():
    from svae_amd.hmm import hmm_estep_perstep_differentiable, hmm_estep_perstep_vjp
    B, T, K = 2, 4, 3
    z = np.zeros
    nat = (z(K), z((T - 1, K, K)), z((B, T, K)))
    none = (None, (None, None, None))
    for bad in ((z(K + 1), nat[1], nat[2]), (nat[0], z((K, K)), nat[2]), (nat[0], z((T, K, K)), nat[2]),
                (nat[0], z((B + 1, T - 1, K, K)), nat[2]), (nat[0], z((B, T - 1, K, K)), z((T, K))),
                (nat[0], nat[1], z((T, 0))), (z(65), z((T - 1, 65, 65)), z((B, T, 65))), (nat[0], nat[1], z(K))):
        with pytest.raises(ValueError):
            hmm_estep_perstep_vjp(bad, none)
    for cot in ((z(B + 1), (None, None, None)), (z(()), (None, None, None)), (None, (z(K), None, None)),
                (None, (None, z((B, K, K)), None)), (None, (None, z((T - 1, K, K)), None)),
                (None, (None, z((B, T, K, K)), None)), (None, (None, None, z((B, T - 1, K))))):
        with pytest.raises(ValueError):
            hmm_estep_perstep_vjp(nat, cot)
    one = (z(K), z((T - 1, K, K)), z((T, K)))                            # unbatched: cotangents without the leading axis
    for cot in ((z(1), (None, None, None)), (None, (z((1, K)), None, None)), (None, (None, z((1, T - 1, K, K)), None))):
        with pytest.raises(ValueError):
            hmm_estep_perstep_vjp(one, cot)
    with pytest.raises(ValueError):
        hmm_estep_perstep_vjp(nat, none, lengths=np.array([1, 2, 3]))
    with pytest.raises(ValueError):
        hmm_estep_perstep_vjp(nat, none, lengths=np.array([1.0, 2.0]))
    with pytest.raises(TypeError):
        hmm_estep_perstep_differentiable(nat)
    with pytest.raises(TypeError):
        hmm_estep_perstep_differentiable((torch.zeros(K), nat[1], torch.zeros(B, T, K)))
