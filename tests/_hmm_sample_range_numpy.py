"""The batches of tests/_hmm_range_numpy.py as SAMPLING problems (S = 4 uniforms per step, per-sequence transition
matrices) with the paths of the log-space oracle tests/_hmm_sample_numpy.py, shared by tests/test_hmm_sample_range_cpu.py
(margins, teeth) and tests/test_hmm_sample_range_hip.py (the kernels) so that each reference is computed once.

old_sample is what hmm_sample computed BEFORE its filter took the E-step's range contract: the scaled filter renormalised
every step, a step redone in log space only where its normaliser fell below 1e-200, and the draw with its own 1e-200 test.
Only here to show that the cases have teeth."""
import functools

import numpy as np
from scipy.special import logsumexp

import _hmm_range_numpy as R
import _hmm_sample_numpy as smp

S = 4
ALL_K = R.K_ROW + R.K_WIDE
FAMILY_K = (3, 8, 9, 16, 17, 32, 33, 64)
FAMILIES = ("surprise", "sparse", "ramp")
VARIANTS = ("shared", "shared4", "batched", "ragged")
TINY = 1e-200


def _freeze(d):
    for x in d.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return d


def _batch(keys, seed):
    init, pair, node, _, extreme = R.stack(keys)
    B, T, _ = node.shape
    u = np.random.default_rng(seed).random((B, S, T))
    states, logZ, margin = smp.sample_batch(init, pair, node, u)
    return _freeze(dict(init=init, pair=pair, node=node, u=u, lengths=None, states=states, logZ=logZ, margin=margin,
                        extreme=extreme))


@functools.lru_cache(maxsize=None)
def gap_batch(K, T):
    """every g of R.GAP_G at every event start of R.gap_t0(T): B = 88 (22 at T = 4); uniforms default_rng(1000 K + T)"""
    return _batch(R.gap_keys(K, T, R.GAP_G), 1000 * K + T)


@functools.lru_cache(maxsize=None)
def family_batch(name, K):
    """the surprise / sparse / ramp batch of K; uniforms default_rng(77 K + len(name))"""
    keys = {"surprise": R.surprise_keys, "sparse": R.sparse_keys, "ramp": R.ramp_keys}[name](K)
    return _batch(keys, 77 * K + len(name))


@functools.lru_cache(maxsize=None)
def ragged_gap_batch(K):
    """gap_batch(K, 37)'s potentials with R.ragged_lengths(B, 37, 500 + K) (lengths 1 and 2 included); uniforms
    default_rng(2000 K + 37); node potentials and uniforms NaN from each length on"""
    T = 37
    init, pair, node, _, extreme = R.stack(R.gap_keys(K, T, R.GAP_G))
    B = node.shape[0]
    lengths = np.array(R.ragged_lengths(B, T, 500 + K))
    u = np.random.default_rng(2000 * K + T).random((B, S, T))
    node = node.copy()
    for b, L in enumerate(lengths):
        node[b, L:] = np.nan
        u[b, :, L:] = np.nan
    states, logZ, margin = smp.sample_ragged(init, pair, node, u, lengths)
    return _freeze(dict(init=init, pair=pair, node=node, u=u, lengths=lengths, states=states, logZ=logZ, margin=margin,
                        extreme=extreme & (lengths == T)))


@functools.lru_cache(maxsize=None)
def mixed(K, variant):
    """R.mixed_batch(K, variant) with uniforms default_rng(3000 K + len(variant)) (NaN from a row's length on)"""
    m = R.mixed_batch(K, variant)
    B, T, _ = m["node"].shape
    u = np.random.default_rng(3000 * K + len(variant)).random((B, S, T))
    if m["lengths"] is None:
        states, logZ, margin = smp.sample_batch(m["init"], m["pair"], m["node"], u)
    else:
        for b, L in enumerate(m["lengths"]):
            u[b, :, L:] = np.nan
        states, logZ, margin = smp.sample_ragged(m["init"], m["pair"], m["node"], u, m["lengths"])
    ordinary = np.array([b for b in range(B) if b not in m["ext"]])
    return _freeze(dict(init=m["init"], pair=m["pair"], node=m["node"], u=u, lengths=m["lengths"], states=states,
                        logZ=logZ, margin=margin, extreme=m["extreme"], ordinary=ordinary))


def old_sample(init, pair, node, u):
    """one sequence in the sampler's arithmetic before the range contract: pair (K,K), node (T,K), u (S,T)
    -> states (S,T) int32, logZ"""
    init, pair, node, u = (np.asarray(x, float) for x in (init, pair, node, u))
    T, K = node.shape
    with np.errstate(all="ignore"):
        pmax = pair.max()
        P = np.exp(pair - pmax)
        a = np.empty((T, K))
        x = init + node[0]
        m = x.max()
        w = np.exp(x - m)
        cs = w.sum()
        a[0] = w / cs
        lz = m + np.log(cs)
        for t in range(1, T):
            m = node[t].max()
            w = (a[t - 1] @ P) * np.exp(node[t] - m)
            cs, shift = w.sum(), m + pmax
            if not cs > TINY:                                   # this step alone in log space
                la = np.where(a[t - 1] > 0, np.log(a[t - 1]), -np.inf)
                lal = logsumexp(la[:, None] + pair, axis=0) + node[t]
                shift = lal.max()
                w = np.exp(lal - shift) if shift > -np.inf else np.zeros(K)
                cs = w.sum()
            a[t] = w / cs
            lz += np.log(cs) + shift
        states = np.empty(u.shape, np.int32)
        for s in range(u.shape[0]):
            z = 0
            for t in range(T - 1, -1, -1):
                w = a[t] if t == T - 1 else a[t] * P[:, z]
                C = np.cumsum(w)
                if t < T - 1 and C[-1] < TINY:                  # this draw's weights in log space
                    lw = np.where(a[t] > 0, np.log(a[t]), -np.inf) + pair[:, z]
                    mx = lw.max()
                    C = np.cumsum(np.exp(lw - mx) if mx > -np.inf else np.zeros(K))
                uu = u[s, t] if u[s, t] > 0 else 0.0
                thr = min(uu, 1.0) * C[-1]
                z = int(((C <= thr) & (C < C[-1])).sum())
                states[s, t] = z
    return states, lz


def old_differs(batch):
    """does old_sample draw a path other than the oracle's on an extreme sequence of the batch? (stops at the first)"""
    for b in np.flatnonzero(batch["extreme"]):
        got, _ = old_sample(batch["init"], batch["pair"][b], batch["node"][b], batch["u"][b])
        if not np.array_equal(got, batch["states"][b]):
            return True
    return False
