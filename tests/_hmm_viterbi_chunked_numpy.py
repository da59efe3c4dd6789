"""NumPy restatement of the time-chunked Viterbi decoder (svae_amd/csrc/hmm_viterbi_chunked.hip), in the arithmetic that
include/svae_hip.h defines for svae_hmm_chunked_viterbi_f64: fp64 adds and strict-`>` running maxima in the stated order,
so labels and score are the library's bit for bit.  Vectorised over sequences, chunks and start states.  TEST INFRASTRUCTURE.

  step(d, t)[k] = (max_j (d[j] + pair[j][k])) + node[t][k]      running maximum in j order, the lowest j on ties
  stage 1  row j of M_c (c >= 1) starts as pair[j][:] + node[t0][:] and takes `step` over t0+1 .. t1-1; chunk 0 is the
           recursion from init + node[0], its end vector D_0
  stage 2  D_c[k] = max_j (D_{c-1}[j] + M_c[j][k])
  stage 3  every chunk entered with D_{c-1} (chunk 0: init + node[0]) and decoded: psi, then z_{T-1} and the score from the
           last chunk, then the chase from all K end states: cand[t][k], f_c[k]
  stage 4  e_{C-1} = z_{T-1}; e_{c-1} = f_c[e_c]
  stage 5  states[t] = cand[t][e_{c(t)}]
"""
import numpy as np

import _hmm_viterbi_numpy as V


def workspace_bytes(B, T, K, chunk):
    """the closed form of svae_hmm_chunked_viterbi_workspace_bytes (include/svae_hip.h)"""
    if B <= 0 or T <= 0 or K <= 0 or K > 16 or chunk < 2:
        return 0
    C = 1 if chunk >= T else -(-T // chunk)
    return 32 * B * T + 16 * B * C + 16 * (-(-B * C // 16)) + 8 * B * C * K * (K + 1)


def default_chunk(B, T, K):
    """svae_hmm_chunked_viterbi_default_chunk's rule: serial (T) for K > 16, T < 500 or B > 256, else
    2^round(log2(1.2 sqrt(T))), doubled from 128 sequences up"""
    if B < 1 or T < 1 or K < 1 or K > 16 or T < 500 or B > 256:
        return T
    L = 2
    while 200 * L * L <= 144 * T:
        L *= 2
    if B >= 128:
        L *= 2
    return min(L, T)


def _maxplus(d, M, want_arg=False):
    """best[..., k] = max_j (d[..., j] + M[..., j, k]) as a running maximum in j order (and the lowest j attaining it)"""
    K = d.shape[-1]
    best = d[..., 0, None] + M[..., 0, :]
    arg = np.zeros(best.shape, np.int8)
    for j in range(1, K):
        v = d[..., j, None] + M[..., j, :]
        w = v > best                                   # strict: the first (lowest) j keeps a tie
        best = np.where(w, v, best)
        if want_arg:
            arg = np.where(w, np.int8(j), arg)
    return (best, arg) if want_arg else best


def _chunks(node, L):
    """node (B,T,K) -> node padded to whole chunks (B,C,L,K), the chunks' step counts n (C)"""
    B, T, K = node.shape
    C = -(-T // L)
    pad = np.zeros((B, C * L, K))
    pad[:, :T] = node
    return pad.reshape(B, C, L, K), np.minimum(L, T - L * np.arange(C))


def chunk_operators(init, pair, node, L):
    """stage 1 -> (M (B,C,K,K) with M[:, 0] unused, D0 (B,K))"""
    B, T, K = node.shape
    nd, n = _chunks(node, L)
    pr = pair[:, None, None]                           # (B,1,1,K,K): the same matrix for every chunk and start state
    with np.errstate(invalid="ignore"):
        d = pair[:, None] + nd[:, :, 0, None, :]       # [b,c,j,k] = pair[b,j,k] + node[b,t0,k]
        d0 = init[None] + node[:, 0]
        for i in range(1, L):
            dn = _maxplus(d, pr) + nd[:, :, i, None, :]
            d = np.where((i < n)[None, :, None, None], dn, d)
            d0 = _maxplus(d0, pair) + node[:, i]       # (chunk 0 is a whole chunk: C >= 2)
    return d, d0


def boundary_scan(M, D0):
    """stage 2 -> D (B,C,K)"""
    B, C, K, _ = M.shape
    D = np.zeros((B, C, K))
    D[:, 0] = D0
    with np.errstate(invalid="ignore"):
        for c in range(1, C):
            D[:, c] = _maxplus(D[:, c - 1], M[:, c])
    return D


def decode_chunks(init, pair, node, L, D):
    """stage 3 -> (cand (B,C,L,K) int, f (B,C,K) int, zT (B) int, score (B))"""
    B, T, K = node.shape
    nd, n = _chunks(node, L)
    C = len(n)
    psi = np.zeros((B, C, L, K), np.int8)
    head = (np.arange(C) == 0)[None, :, None]
    with np.errstate(invalid="ignore"):
        d = np.concatenate([(init[None] + node[:, 0])[:, None], D[:, :-1]], axis=1)       # (B,C,K)
        for i in range(L):
            best, arg = _maxplus(d, pair[:, None], want_arg=True)
            act = (i < n)[None, :, None] & ~(head & (i == 0))
            d = np.where(act, best + nd[:, :, i], d)
            psi[:, :, i] = np.where(act, arg, 0)
        last = d[:, C - 1]
        zT = np.zeros(B, np.int64)
        score = last[:, 0].copy()
        for k in range(1, K):
            w = last[:, k] > score
            score = np.where(w, last[:, k], score)
            zT = np.where(w, k, zT)
    cand = np.zeros((B, C, L, K), np.int64)
    z = np.broadcast_to(np.arange(K), (B, C, K)).copy()
    for i in range(L - 1, -1, -1):
        live = (i < n)[None, :, None]
        cand[:, :, i] = z
        z = np.where(live, np.take_along_axis(psi[:, :, i].astype(np.int64), z, axis=-1), z)
    return cand, z, zT, score


def chunked_viterbi_batch(init, pair, node, chunk):
    """init (K), pair (K,K) or (B,K,K), node (B,T,K), 2 <= chunk < T -> (labels (B,T) int32, score (B))"""
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    B, T, K = node.shape
    assert 2 <= chunk < T
    pair = np.broadcast_to(pair, (B, K, K))
    M, D0 = chunk_operators(init, pair, node, chunk)
    D = boundary_scan(M, D0)
    cand, f, zT, score = decode_chunks(init, pair, node, chunk, D)
    C = M.shape[1]
    rows = np.arange(B)
    e = np.zeros((B, C), np.int64)
    e[:, C - 1] = zT
    for c in range(C - 1, 0, -1):
        e[:, c - 1] = f[rows, c, e[:, c]]
    t = np.arange(T)
    labels = cand[rows[:, None], (t // chunk)[None], (t % chunk)[None], e[:, t // chunk]]
    return labels.astype(np.int32), score


def chunked_viterbi(init, pair, node, chunk):
    """one sequence: node (T,K) -> (labels (T,) int32, score float64)"""
    labels, score = chunked_viterbi_batch(init, pair, np.asarray(node, np.float64)[None], chunk)
    return labels[0], np.float64(score[0])


def score_bound(init, pair, node):
    """bound (c) of include/svae_hip.h for ONE sequence, node (T,K): 4 T 2^-53 A,
    A = max|init| + sum_t max_k |node_t| + (T-1) max|pair| over the finite entries"""
    def fmax(x, axis=None):
        x = np.abs(np.where(np.isfinite(x), x, 0.0))
        return x.max(axis=axis)
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    T = node.shape[0]
    A = fmax(init) + fmax(node, axis=-1).sum() + (T - 1) * fmax(pair)
    return 4.0 * T * 2.0 ** -53 * A


def count_ties(init, pair, node):
    """how many (step, state) maxima of the serial recursion of ONE sequence are attained by more than one j with a
    finite value, plus 1 if the final maximum over k is"""
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    ties = 0
    with np.errstate(invalid="ignore"):
        d = init + node[0]
        for t in range(1, node.shape[0]):
            v = d[:, None] + pair
            best = v.max(axis=0)
            ties += int((((v == best[None]) & np.isfinite(v)).sum(axis=0) > 1).sum())
            d = best + node[t]
        ties += int(((d == d.max()) & np.isfinite(d)).sum() > 1)
    return ties


def dyadic_problem(seed):
    """-> (init (K), pair (K,K) or (B,K,K), node (B,T,K), chunk): K in 1..16, T in 3..70, 2 <= chunk < T, B in 1..3;
    potentials multiples of 1/4 in [-3/4, 0], so every add of the recursion is exact.  Every third seed carries -inf
    transitions and node entries (never a whole row of `pair`, never all of `init`); every ninth also a chain whose node
    potentials are all -inf at one step."""
    rng = np.random.default_rng(1000 + seed)
    K = int(rng.integers(1, 17))
    T = int(rng.integers(3, 71))
    chunk = int(rng.integers(2, T))
    B = int(rng.integers(1, 4))
    q = lambda *s: -0.25 * rng.integers(0, 4, size=s)              # noqa: E731
    init, node = q(K), q(B, T, K)
    pair = q(B, K, K) if seed % 2 else q(K, K)
    if seed % 3 == 0:
        pair = np.where(rng.random(pair.shape) < 0.25, -np.inf, pair)
        idx = np.arange(K)
        pair[..., idx, idx] = np.where(np.isinf(pair[..., idx, idx]), -0.5, pair[..., idx, idx])   # self-transitions stay
        node = np.where(rng.random(node.shape) < 0.1, -np.inf, node)
        if seed % 9 == 0:
            node[B - 1, int(rng.integers(1, T))] = -np.inf
    return init, pair, node, chunk


DYADIC_SEEDS = range(60)
bits = V.bits
