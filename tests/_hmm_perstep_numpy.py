"""NumPy fp64 oracle of the HMM E-step with PER-STEP transition potentials.  TEST INFRASTRUCTURE.

    log p(z) ∝ init[z_0] + sum_{t<L-1} pair[t][z_t][z_{t+1}] + sum_{t<L} node[t][z_t]

hmm_estep_perstep: the plain log-space forward-backward on one sequence, cut to `length` steps; returns logZ, E_init,
the per-step E_trans (T-1,K,K) and E_states (T,K), both 0 from the length on.  brute_force: the same four by enumerating
all K^L paths (tiny K, T only).  Checked against each other, against oracle/hmm_numpy at constant P_t and by the marginal
identities in tests/test_hmm_perstep_oracle.py.
"""
import itertools

import numpy as np


def _lse(x, axis=None):
    """logsumexp with exp(-inf - (-inf)) read as 0: an all -inf slice gives -inf without a warning or a NaN"""
    x = np.asarray(x, np.float64)
    m = np.max(x, axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        out = np.log(np.sum(np.exp(x - ms), axis=axis, keepdims=True)) + ms
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def hmm_estep_perstep(natparam, length=None):
    init, pair, node = (np.asarray(x, np.float64) for x in natparam)
    T, K = node.shape
    assert init.shape == (K,) and pair.shape == (T - 1, K, K)
    L = T if length is None else int(length)
    assert 1 <= L <= T
    la = np.full((L, K), -np.inf)
    lb = np.zeros((L, K))
    la[0] = init + node[0]
    for t in range(1, L):
        la[t] = _lse(la[t - 1][:, None] + pair[t - 1], axis=0) + node[t]
    for t in range(L - 2, -1, -1):
        lb[t] = _lse(pair[t] + (node[t + 1] + lb[t + 1])[None, :], axis=1)
    logZ = float(_lse(la[L - 1]))
    E_states = np.zeros((T, K))
    E_trans = np.zeros((T - 1, K, K))
    E_states[:L] = np.exp(la + lb - logZ)
    for t in range(L - 1):
        E_trans[t] = np.exp(la[t][:, None] + pair[t] + (node[t + 1] + lb[t + 1])[None, :] - logZ)
    return logZ, (E_states[0].copy(), E_trans, E_states)


def brute_force(natparam, length=None):
    init, pair, node = (np.asarray(x, np.float64) for x in natparam)
    T, K = node.shape
    L = T if length is None else int(length)
    paths = list(itertools.product(range(K), repeat=L))
    score = np.array([init[z[0]] + sum(pair[t][z[t], z[t + 1]] for t in range(L - 1)) + sum(node[t][z[t]] for t in range(L))
                      for z in paths])
    logZ = float(_lse(score))
    w = np.exp(score - logZ)
    E_states = np.zeros((T, K))
    E_trans = np.zeros((T - 1, K, K))
    for z, p in zip(paths, w):
        for t in range(L):
            E_states[t, z[t]] += p
        for t in range(L - 1):
            E_trans[t, z[t], z[t + 1]] += p
    return logZ, (E_states[0].copy(), E_trans, E_states)
