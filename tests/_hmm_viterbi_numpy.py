"""NumPy restatement of the Viterbi arithmetic that include/svae_hip.h defines for svae_hmm_viterbi_f64, and a
brute-force enumerator over all K^T paths.  Written from the definition (checker only):

  delta_0[k] = init[k] + node[0][k]
  delta_t[k] = (max_j (delta_{t-1}[j] + pair[j][k])) + node[t][k]        fp64, additions in that order
  psi_t[k]   = the LOWEST j attaining the maximum (running maximum, strict `>`)
  z_{T-1}    = the lowest k attaining max_k delta_{T-1}[k];   z_t = psi_{t+1}[z_{t+1}];   score = delta_{T-1}[z_{T-1}]
"""
import itertools

import numpy as np


def viterbi_batch(init, pair, node):
    """init (K), pair (K,K) [j][k] = j -> k or (B,K,K), node (B,T,K), float64 -> (labels (B,T) int32, score (B)).
    The same scalar operations in the same order for every sequence and state, carried out on whole arrays."""
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    B, T, K = node.shape
    pair = np.broadcast_to(pair, (B, K, K))
    psi = np.zeros((T, B, K), np.int8)
    rows = np.arange(B)
    with np.errstate(invalid="ignore"):
        delta = init[None, :] + node[:, 0]
        for t in range(1, T):
            best = delta[:, 0, None] + pair[:, 0]
            arg = np.zeros((B, K), np.int8)
            for j in range(1, K):
                v = delta[:, j, None] + pair[:, j]
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


def viterbi(init, pair, node):
    """init (K), pair (K,K), node (T,K) -> (labels (T,) int32, score float64)."""
    labels, score = viterbi_batch(init, pair, np.asarray(node, np.float64)[None])
    return labels[0], np.float64(score[0])


def path_score(init, pair, node, labels):
    """The sum along `labels` in the recursion's order: ((init + node_0) + pair) + node_1, ..."""
    init, pair, node = (np.asarray(x, np.float64) for x in (init, pair, node))
    s = init[labels[0]] + node[0][labels[0]]
    for t in range(1, len(labels)):
        s = (s + pair[labels[t - 1]][labels[t]]) + node[t][labels[t]]
    return np.float64(s)


def brute_force(init, pair, node):
    """All K^T paths, each scored by path_score -> (best score, the paths attaining it)."""
    T, K = np.asarray(node).shape
    best, paths = None, []
    for p in itertools.product(range(K), repeat=T):
        s = path_score(init, pair, node, p)
        if best is None or s > best:
            best, paths = s, [p]
        elif s == best:
            paths.append(p)
    return best, paths


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)
