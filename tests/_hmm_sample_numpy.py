"""NumPy oracle of HMM posterior sampling (svae_hmm_sample_f64, include/svae_hip.h), independent of the kernels' scaling:
a log-space forward filter (scipy's logsumexp), the draw's weights ALWAYS in the log-space form of the definition,
w[k] = exp(la_t[k] + pair[k][z_{t+1}] - max_k(..)), np.cumsum (sequential, hence index order), thr = u C[-1] and
z = min(#{k : C[k] <= thr}, K-1) -- which is the definition's rule wherever the margin below is positive.

Besides the states and log Z it returns the smallest MARGIN over all draws, min_k |C[k] - thr| / C[K-1]: the distance of
a draw from a decision boundary, relative to the total.  A kernel whose filtered sums agree with these to 1e-10 of the
total (the project's tolerance for log Z) cannot flip a draw whose margin is 1e-8: the GPU tests compare such cases
exactly, and tests/test_hmm_sample_cpu.py asserts the margins of every case they use.

The cases themselves (problem generator, seeds, shapes) live here so that the CPU and the GPU file share one computation
of each reference."""
import functools

import numpy as np
from scipy.special import logsumexp

MARGIN = 1e-8


def problem(B, T, K, S, rng, scale=1.0, batched_pair=False):
    """the generator of tests/test_hmm_viterbi_hip.py::_problem, then the uniforms (drawn last)"""
    init = np.log(rng.dirichlet(np.ones(K)))
    shape = (B, K, K) if batched_pair else (K, K)
    pair = np.log(rng.dirichlet(np.ones(K), size=shape[:-1])) + 0.3 * rng.standard_normal(shape)
    node = scale * rng.standard_normal((B, T, K))
    u = rng.random((B, S, T))
    return init, pair, node, u


def log_filter(init, pair, node):
    """la[b,t,k] = log p(z_t = k, node_{0..t}) (unnormalised), batched; pair (K,K) or (B,K,K)"""
    init, pair, node = (np.asarray(x, float) for x in (init, pair, node))
    B, T, K = node.shape
    pb = np.broadcast_to(pair, (B, K, K))
    la = np.empty((B, T, K))
    with np.errstate(invalid="ignore", divide="ignore"):
        la[:, 0] = init[None] + node[:, 0]
        for t in range(1, T):
            la[:, t] = logsumexp(la[:, t - 1][:, :, None] + pb, axis=1) + node[:, t]
    return la


def sample_batch(init, pair, node, u):
    """-> states (B,S,T) int32, logZ (B), the minimum margin over all draws"""
    init, pair, node, u = (np.asarray(x, float) for x in (init, pair, node, u))
    B, T, K = node.shape
    S = u.shape[1]
    assert u.shape == (B, S, T)
    pb = np.broadcast_to(pair, (B, K, K))
    la = log_filter(init, pair, node)
    states = np.empty((B, S, T), np.int32)
    margin = np.inf
    bi = np.arange(B)[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        logZ = logsumexp(la[:, T - 1], axis=1)
        z = None
        for t in range(T - 1, -1, -1):
            lw = np.broadcast_to(la[:, t][:, None, :], (B, S, K))
            if t < T - 1:
                lw = lw + pb[bi, :, z]                                # pair[b][k][z_{t+1}]: (B,S,K)
            m = lw.max(-1, keepdims=True)
            w = np.where(np.isfinite(m), np.exp(lw - np.where(np.isfinite(m), m, 0.0)), 0.0)
            C = np.cumsum(w, axis=-1)
            tot = C[..., -1]
            uu = np.clip(np.where(np.isnan(u[:, :, t]), 0.0, u[:, :, t]), 0.0, 1.0)
            thr = uu * tot
            z = np.minimum((C <= thr[..., None]).sum(-1), K - 1)
            states[:, :, t] = z
            mg = np.abs(C - thr[..., None]).min(-1) / tot
            margin = min(margin, float(np.nanmin(mg))) if np.isfinite(mg).any() else margin
    return states, logZ, margin


def sample_ragged(init, pair, node, u, lengths):
    """each sequence cut at its length and run alone; states[b, :, L:] = -1"""
    node, u = np.asarray(node, float), np.asarray(u, float)
    B, T, K = node.shape
    S = u.shape[1]
    pair = np.asarray(pair, float)
    states = np.full((B, S, T), -1, np.int32)
    logZ = np.empty(B)
    margin = np.inf
    for b in range(B):
        L = int(lengths[b])
        st, lz, mg = sample_batch(init, pair[b] if pair.ndim == 3 else pair, node[b:b + 1, :L], u[b:b + 1, :, :L])
        states[b, :, :L], logZ[b], margin = st[0], lz[0], min(margin, mg)
    return states, logZ, margin


# ---- the cases the GPU file compares exactly (tests/test_hmm_sample_cpu.py asserts their margins) ----------------------
GRID_K = (1, 2, 5, 8, 15, 16, 17, 31, 32, 33, 48, 64)
GRID_T = (1, 2, 7, 200)
GRID_B = (1, 3, 5, 64)
GRID_SCALE = (1.0, 50.0)
GRID_S = 3
PAIR_K = (3, 16, 20, 64)
LTR_K = (4, 16, 24, 64)


@functools.lru_cache(maxsize=None)
def grid_case(K, T, B, scale):
    rng = np.random.default_rng(100000 * K + 1000 * T + B + int(scale))
    init, pair, node, u = problem(B, T, K, GRID_S, rng, scale)
    return (init, pair, node, u) + sample_batch(init, pair, node, u)


@functools.lru_cache(maxsize=None)
def pair_case(K):
    """batched pair parameters: B = 9, T = 37, S = 2, scale 2, seed K"""
    rng = np.random.default_rng(K)
    init, pair, node, u = problem(9, 37, K, 2, rng, 2.0, batched_pair=True)
    return (init, pair, node, u) + sample_batch(init, pair, node, u)


@functools.lru_cache(maxsize=None)
def ragged_case(K):
    """the shapes of pair_case with lengths from rng.integers(1, T+1), L[0] = 1, L[1] = T, L[2] = 2; node and u NaN from
    L on (the oracle slices them away)"""
    rng = np.random.default_rng(K)
    B, T, S = 9, 37, 2
    init, pair, node, u = problem(B, T, K, S, rng, 2.0, batched_pair=True)
    L = rng.integers(1, T + 1, size=B)
    L[0], L[1], L[2] = 1, T, 2
    for b in range(B):
        node[b, L[b]:] = np.nan
        u[b, :, L[b]:] = np.nan
    return (init, pair, node, u, L) + sample_ragged(init, pair, node, u, L)


@functools.lru_cache(maxsize=None)
def ltr_case(K):
    """left-to-right chains: B = 7, T = 90, S = 3, scale 2, seed 11 K, the lower triangle of pair forbidden"""
    rng = np.random.default_rng(11 * K)
    init, pair, node, u = problem(7, 90, K, 3, rng, 2.0)
    pair = np.where(np.tril(np.ones((K, K)), -1) > 0, -np.inf, pair)
    return (init, pair, node, u) + sample_batch(init, pair, node, u)
