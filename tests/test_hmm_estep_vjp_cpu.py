"""CPU tests of the arithmetic of the HMM E-step's derivative (svae_hmm_estep_vjp_f64): the NumPy restatement
tests/_hmm_vjp_numpy.py -- the reference of the GPU file -- against torch fp64 double-backward through a log-space
logsumexp chain, and against the covariance taken directly over all K^T paths.
Tolerance of both: 1e-12 (|g| + T max|cotangent|), the size of phi (tests/_hmm_vjp_numpy.scale)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_vjp_numpy as vjp  # noqa: E402


def _problem(K, T, seed, forbid):
    rng = np.random.default_rng(seed)
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    node = rng.standard_normal((T, K))
    if forbid:
        pair[0, K - 1] = -np.inf          # (K = 1: the only transition; the chain then has log Z = -inf unless T = 1)
    cot = dict(g=float(rng.standard_normal()), u0=rng.standard_normal(K), V=rng.standard_normal((K, K)),
               W=rng.standard_normal((T, K)))
    return init, pair, node, cot


def _torch_double_backward(init, pair, node, g, u0, V, W):
    ti, tp, tn = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (init, pair, node))
    al = ti + tn[0]
    for t in range(1, node.shape[0]):
        al = torch.logsumexp(al[:, None] + tp, 0) + tn[t]
    logZ = torch.logsumexp(al, 0)
    Ei, Et, Es = torch.autograd.grad(logZ, (ti, tp, tn), create_graph=True, allow_unused=True)
    loss = g * logZ + (torch.tensor(u0) * Ei).sum() + (torch.tensor(W) * Es).sum()
    if Et is not None:                       # (T = 1: log Z does not depend on the pair parameters)
        loss = loss + (torch.tensor(V) * Et).sum()
    gi, gp, gn = torch.autograd.grad(loss, (ti, tp, tn), allow_unused=True)
    gp = torch.zeros_like(tp) if gp is None else gp
    return gi.numpy(), gp.numpy(), gn.numpy()


CASES = [(K, T, forbid) for K in (1, 2, 3, 5, 17) for T in (1, 2, 9) for forbid in (False, True)
         if not (forbid and K == 1 and T > 1)]       # K = 1 with its transition forbidden: log Z = -inf, outside the contract


@pytest.mark.parametrize("K,T,forbid", CASES)
def test_restatement_equals_torch_double_backward(K, T, forbid):
    init, pair, node, cot = _problem(K, T, 100 * K + T, forbid)
    want = _torch_double_backward(init, pair, node, **cot)
    got = vjp.estep_vjp(init, pair, node, **cot)
    tol = 1e-12 * vjp.scale(cot["g"], cot["u0"], cot["V"], cot["W"], T)
    for name, a, b in zip(("init", "pair", "node"), got, want):
        assert np.isfinite(a).all(), name
        err = float(np.max(np.abs(a - b)))
        print(K, T, forbid, name, err, tol)
        assert err <= tol, (name, err, tol)
    if forbid and T > 1:
        assert got[1][0, K - 1] == 0.0       # a -inf potential has gradient exactly 0


def _brute_force(init, pair, node, g, u0, V, W):
    T, K = node.shape
    paths = list(itertools.product(range(K), repeat=T))
    score = np.array([init[z[0]] + sum(node[t, z[t]] for t in range(T)) + sum(pair[z[t], z[t + 1]] for t in range(T - 1))
                      for z in paths])
    p = np.exp(score - score.max())
    p /= p.sum()
    phi = np.array([u0[z[0]] + sum(W[t, z[t]] for t in range(T)) + sum(V[z[t], z[t + 1]] for t in range(T - 1))
                    for z in paths])
    c = p * (g + phi - p @ phi)              # E[f (g + phi - E phi)] = g E[f] + Cov(f, phi)
    gn, gp = np.zeros((T, K)), np.zeros((K, K))
    for z, cz in zip(paths, c):
        for t in range(T):
            gn[t, z[t]] += cz
        for t in range(T - 1):
            gp[z[t], z[t + 1]] += cz
    return gn[0].copy(), gp, gn


@pytest.mark.parametrize("K,T,forbid", [(K, T, f) for K in (1, 2, 3) for T in (1, 2, 3, 5) for f in (False, True)
                                        if not (f and K == 1 and T > 1)])
def test_restatement_equals_the_covariance_over_all_paths(K, T, forbid):
    init, pair, node, cot = _problem(K, T, 500 + 10 * K + T, forbid)
    with np.errstate(all="ignore"):
        want = _brute_force(init, pair, node, **cot)
    got = vjp.estep_vjp(init, pair, node, **cot)
    tol = 1e-12 * vjp.scale(cot["g"], cot["u0"], cot["V"], cot["W"], T)
    for name, a, b in zip(("init", "pair", "node"), got, want):
        err = float(np.max(np.abs(a - b)))
        assert err <= tol, (name, err, tol)


def test_batch_form_cuts_each_sequence_to_its_length():
    rng = np.random.default_rng(3)
    B, T, K = 3, 5, 3
    init, pair, _, _ = _problem(K, T, 9, False)
    node = rng.standard_normal((B, T, K))
    W = rng.standard_normal((B, T, K))
    L = np.array([5, 1, 3])
    node[1, 1:] = np.nan
    W[2, 3:] = np.nan
    gi, gp, gn = vjp.estep_vjp_batch(init, pair, node, lengths=L, W=W)
    assert np.isfinite(gi).all() and np.isfinite(gp).all() and np.isfinite(gn).all()
    assert (gn[1, 1:] == 0).all() and (gn[2, 3:] == 0).all()
    one = vjp.estep_vjp(init, pair, node[2, :3], W=W[2, :3])
    assert np.array_equal(one[2], gn[2, :3]) and np.array_equal(one[1], gp[2])
