"""NumPy oracles of Viterbi decoding and posterior sampling with PER-STEP transition potentials
(svae_hmm_perstep_viterbi_f64, svae_hmm_perstep_sample_f64; include/svae_hip.h), and the cases the CPU and the GPU test
files share.  TEST INFRASTRUCTURE, written from the definitions.

  viterbi_perstep   delta_0[k] = init[k] + node[0][k];  delta_t[k] = (max_j (delta_{t-1}[j] + pair[t-1][j][k])) + node[t][k]
                    in fp64 with the additions in that order, running maximum with a strict `>` (lowest j keeps a tie),
                    on whole arrays in the style of _hmm_viterbi_numpy.viterbi_batch: labels and score bit for bit.
  path_score        the sum along a path in the recursion's order;  brute_force  all K^L paths.
  sample_perstep    the log-space filter of _hmm_perstep_numpy (its logsumexp), the draw's weights in the log-space form
                    of the definition, np.cumsum (sequential: index order), thr = u C[-1], z = min(#{C <= thr}, K-1);
                    returns states, log Z and the smallest margin as _hmm_sample_numpy.sample_batch defines it.
  *_ragged          each sequence cut at its length and run alone; labels -1 from the length on.
"""
import functools
import itertools

import numpy as np

import _hmm_perstep_numpy as ps

MARGIN = 1e-8


# ---- problems ---------------------------------------------------------------------------------------------------------------
def problem(B, T, K, S, rng, pair_batched, scale=1.0):
    """the generator of tests/test_hmm_perstep_hip.py::_problem, then the uniforms (drawn last)"""
    init = np.log(rng.dirichlet(np.ones(K)))
    lead = (B, T - 1) if pair_batched else (T - 1,)
    pair = np.log(rng.dirichlet(np.ones(K), size=lead + (K,))) + 0.5 * rng.standard_normal(lead + (K, K))
    pair = pair + 3.0 * rng.standard_normal(lead + (1, 1))              # every step at its own offset
    node = scale * rng.standard_normal((B, T, K))
    u = rng.random((B, S, T))
    return init, pair, node, u


def _pair_b(pair, B):
    pair = np.asarray(pair, np.float64)
    return np.broadcast_to(pair, (B,) + pair.shape[-3:])


# ---- Viterbi ----------------------------------------------------------------------------------------------------------------
def viterbi_perstep(init, pair, node):
    """init (K), pair (T-1,K,K) or (B,T-1,K,K), node (B,T,K), float64 -> (labels (B,T) int32, score (B))"""
    init, node = np.asarray(init, np.float64), np.asarray(node, np.float64)
    B, T, K = node.shape
    pair = _pair_b(pair, B)
    psi = np.zeros((T, B, K), np.int8)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        delta = init[None, :] + node[:, 0]
        for t in range(1, T):
            P = pair[:, t - 1]
            best = delta[:, 0, None] + P[:, 0]
            arg = np.zeros((B, K), np.int8)
            for j in range(1, K):
                v = delta[:, j, None] + P[:, j]
                w = v > best                              # strict: the first (lowest) j keeps a tie
                best = np.where(w, v, best)
                arg = np.where(w, np.int8(j), arg)
            psi[t] = arg
            delta = best + node[:, t]
        z = np.zeros(B, np.int64)
        score = delta[:, 0].copy()
        for k in range(1, K):
            w = delta[:, k] > score
            score = np.where(w, delta[:, k], score)
            z = np.where(w, k, z)
    labels = np.zeros((B, T), np.int32)
    labels[:, T - 1] = z
    for t in range(T - 1, 0, -1):
        labels[:, t - 1] = psi[t][rows, labels[:, t]]
    return labels, score


def path_score(init, pair, node, labels):
    """init (K), pair (T-1,K,K), node (T,K): the sum along `labels` in the recursion's order"""
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    with np.errstate(invalid="ignore"):
        s = init[labels[0]] + node[0][labels[0]]
        for t in range(1, len(labels)):
            s = (s + pair[t - 1][labels[t - 1]][labels[t]]) + node[t][labels[t]]
    return np.float64(s)


def brute_force(init, pair, node):
    """all K^T paths of one sequence, each scored by path_score -> (best score, the paths attaining it)"""
    T, K = np.asarray(node).shape
    best, paths = None, []
    for p in itertools.product(range(K), repeat=T):
        s = path_score(init, pair, node, p)
        if best is None or s > best:
            best, paths = s, [p]
        elif s == best:
            paths.append(p)
    return best, paths


def viterbi_ragged(init, pair, node, lengths):
    node = np.asarray(node, np.float64)
    B, T, K = node.shape
    pair = np.asarray(pair, np.float64)
    labels = np.full((B, T), -1, np.int32)
    score = np.empty(B)
    for b in range(B):
        L = int(lengths[b])
        pb = pair[b] if pair.ndim == 4 else pair
        lab, sc = viterbi_perstep(init, pb[:L - 1], node[b:b + 1, :L])
        labels[b, :L], score[b] = lab[0], sc[0]
    return labels, score


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def log_filter(init, pair, node):
    """la[b,t,k], unnormalised, with the logsumexp of _hmm_perstep_numpy"""
    init, node = np.asarray(init, np.float64), np.asarray(node, np.float64)
    B, T, K = node.shape
    pair = _pair_b(pair, B)
    la = np.empty((B, T, K))
    with np.errstate(invalid="ignore", divide="ignore"):
        la[:, 0] = init[None] + node[:, 0]
        for t in range(1, T):
            la[:, t] = ps._lse(la[:, t - 1][:, :, None] + pair[:, t - 1], axis=1) + node[:, t]
    return la


def sample_perstep(init, pair, node, u):
    """-> states (B,S,T) int32, logZ (B), the minimum margin over all draws (min_k |C[k] - thr| / C[K-1])"""
    node, u = np.asarray(node, np.float64), np.asarray(u, np.float64)
    B, T, K = node.shape
    S = u.shape[1]
    assert u.shape == (B, S, T)
    pair = _pair_b(pair, B)
    la = log_filter(init, pair, node)
    states = np.empty((B, S, T), np.int32)
    margin = np.inf
    bi = np.arange(B)[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        logZ = ps._lse(la[:, T - 1], axis=1)
        z = None
        for t in range(T - 1, -1, -1):
            lw = np.broadcast_to(la[:, t][:, None, :], (B, S, K))
            if t < T - 1:
                lw = lw + pair[:, t][bi, :, z]                         # pair[b][t][k][z_{t+1}]: (B,S,K)
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
    node, u = np.asarray(node, np.float64), np.asarray(u, np.float64)
    B, T, K = node.shape
    S = u.shape[1]
    pair = np.asarray(pair, np.float64)
    states = np.full((B, S, T), -1, np.int32)
    logZ = np.empty(B)
    margin = np.inf
    for b in range(B):
        L = int(lengths[b])
        pb = pair[b] if pair.ndim == 4 else pair
        st, lz, mg = sample_perstep(init, pb[:L - 1], node[b:b + 1, :L], u[b:b + 1, :, :L])
        states[b, :, :L], logZ[b], margin = st[0], lz[0], min(margin, mg)
    return states, logZ, margin


def extreme_draws(init, pair, node):
    """what u = 0 and u = 1 draw under the definition: backwards from the last step, the lowest resp. the highest state
    whose weight w[k] is positive (allowed: reachable, and its transition into the state drawn after it not forbidden).
    -> (lowest (B,T), highest (B,T), the smallest w[highest] / C[K-1] met).  u = 1 takes the lowest k with C[k] = C[K-1],
    which is that highest state as long as its weight is not lost in the rounding of the total: the last figure says by
    how much (tests/test_hmm_perstep_decode_cpu.py asserts it >= MARGIN for the cases compared)."""
    node = np.asarray(node, np.float64)
    B, T, K = node.shape
    pair = _pair_b(pair, B)
    la = log_filter(init, pair, node)
    out = np.zeros((2, B, T), np.int32)
    rel = np.inf
    for i, pick in enumerate((np.min, np.max)):
        for b in range(B):
            nxt = None
            for t in range(T - 1, -1, -1):
                lw = la[b, t] if t == T - 1 else la[b, t] + pair[b, t][:, nxt]
                w = np.exp(lw - lw.max())
                nxt = int(pick(np.nonzero(w > 0)[0]))
                out[i, b, t] = nxt
                if i == 1:
                    rel = min(rel, float(w[nxt] / np.cumsum(w)[-1]))
    return out[0], out[1], rel


def statistics_within_5_sigma(states, natparam):
    """states (N,T) draws of ONE sequence: every state marginal and every per-step transition count within 5 sigma
    (binomial, per cell) of the enumeration of all paths; a cell of probability 0 must stay empty.  Returns the worst
    deviation in sigmas."""
    states = np.asarray(states)
    N, T = states.shape
    _, (_, Et, Es) = ps.brute_force(natparam)
    K = Es.shape[1]
    worst = 0.0

    def cell(count, p):
        nonlocal worst
        sd = np.sqrt(N * p * (1.0 - p))
        if sd == 0.0:
            assert count == round(N * p), (count, p)
            return
        dev = abs(count - N * p) / sd
        worst = max(worst, dev)
        assert dev <= 5.0, (count, N * p, sd)

    for t in range(T):
        for k in range(K):
            cell(int((states[:, t] == k).sum()), float(Es[t, k]))
    for t in range(T - 1):
        for j in range(K):
            for k in range(K):
                cell(int(((states[:, t] == j) & (states[:, t + 1] == k)).sum()), float(Et[t, j, k]))
    return worst


# ---- the cases the GPU file compares exactly (tests/test_hmm_perstep_decode_cpu.py asserts the sampling margins) -------------
GRID_K = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)
GRID_T = (1, 2, 3, 7, 37)
GRID_B = (1, 5, 9)
GRID_S = 3
LONG_K = (3, 16, 17, 64)
LONG_T = (17, 65, 130)           # across the backtrace's block sizes (8, 16, 32, 64 steps)
LTR_K = (4, 16, 24, 64)
TIE_K = (3, 16, 17, 64)
PAIR_K = (3, 16, 20, 64)


class Case:
    """one problem with its oracle results: init, pair, node, u; labels, score (Viterbi); states, logZ, margin (sampling)"""

    def __init__(self, init, pair, node, u=None):
        self.init, self.pair, self.node, self.u = init, pair, node, u
        self.labels, self.score = viterbi_perstep(init, pair, node)
        if u is not None:
            self.states, self.logZ, self.margin = sample_perstep(init, pair, node, u)

    @property
    def natparam(self):
        return self.init, self.pair, self.node


@functools.lru_cache(maxsize=None)
def grid_cases(K):
    """T x B x {shared, per-sequence} in that order from one generator, S = 3, scale 1.5, seed 5000 + K"""
    rng = np.random.default_rng(5000 + K)
    out = []
    for T in GRID_T:
        for B in GRID_B:
            for pair_batched in (False, True):
                out.append(Case(*problem(B, T, K, GRID_S, rng, pair_batched, 1.5)))
    return out


@functools.lru_cache(maxsize=None)
def long_cases(K):
    """Viterbi only: T across the backtrace's block sizes, B = 5, per-sequence pair parameters, seed 5100 + K"""
    rng = np.random.default_rng(5100 + K)
    return [Case(*problem(5, T, K, 1, rng, True, 1.5)[:3]) for T in LONG_T]


@functools.lru_cache(maxsize=None)
def ltr_case(K):
    """left-to-right chains: the lower triangle of every step's matrix forbidden; B = 7, T = 40, S = 3, seed 11 K"""
    rng = np.random.default_rng(11 * K)
    init, pair, node, u = problem(7, 40, K, 3, rng, False, 2.0)
    pair = np.where(np.tril(np.ones((K, K)), -1) > 0, -np.inf, pair)
    return Case(init, pair, node, u)


def tie_problem(B, T, K, rng, pair_batched=True):
    """integer-valued potentials drawn from {-2, -1, 0, -inf}: sums are exact, so equal path scores are exact ties"""
    vals = np.array([-2.0, -1.0, 0.0, -np.inf])
    lead = (B, T - 1) if pair_batched else (T - 1,)
    init = rng.choice(vals[:3], size=K)
    pair = rng.choice(vals, size=lead + (K, K), p=[0.3, 0.3, 0.3, 0.1])
    node = rng.choice(vals, size=(B, T, K), p=[0.3, 0.3, 0.3, 0.1])
    return init, pair, node


@functools.lru_cache(maxsize=None)
def tie_case(K):
    """B = 5, T = 37, per-sequence pair parameters, seed 700 + K"""
    return Case(*tie_problem(5, 37, K, np.random.default_rng(700 + K)))


@functools.lru_cache(maxsize=None)
def dead_step_case(K):
    """one step whose transition potentials are all -inf: score -inf, labels by the lowest-index rule"""
    rng = np.random.default_rng(900 + K)
    init, pair, node, _ = problem(3, 9, K, 1, rng, True, 1.5)
    pair[:, 4] = -np.inf
    return Case(init, pair, node)


@functools.lru_cache(maxsize=None)
def ragged_case(K):
    """B = 9, T = 37, S = 2, per-sequence pair parameters, scale 1.5, seed 6100 + K; L = rng.integers(1, T+1) with
    L[0] = 1, L[1] = T, L[2] = 2.  Returns the clean problem, the lengths, and the oracle on the cut sequences."""
    rng = np.random.default_rng(6100 + K)
    B, T, S = 9, 37, 2
    init, pair, node, u = problem(B, T, K, S, rng, True, 1.5)
    L = rng.integers(1, T + 1, size=B)
    L[0], L[1], L[2] = 1, T, 2
    labels, score = viterbi_ragged(init, pair, node, L)
    states, logZ, margin = sample_ragged(init, pair, node, u, L)
    shared = (viterbi_ragged(init, pair[0], node, L), sample_ragged(init, pair[0], node, u, L))
    return dict(init=init, pair=pair, node=node, u=u, L=L, labels=labels, score=score, states=states, logZ=logZ,
                margin=margin, shared=shared)


def padded(pair, node, u, lengths):
    """copies with node steps >= L, pair steps >= L - 1 (pair per sequence) and u steps >= L replaced by NaN"""
    node, pair, u = np.array(node), np.array(pair), np.array(u)
    for b, L in enumerate(lengths):
        node[b, L:] = np.nan
        if pair.ndim == 4:
            pair[b, L - 1:] = np.nan
        u[b, :, L:] = np.nan
    return pair, node, u
