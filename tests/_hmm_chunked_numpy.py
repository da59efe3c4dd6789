"""NumPy restatement of the time-chunked HMM E-step (svae_amd/csrc/hmm_estep_chunked.hip): its three stages and its
range criterion, one sequence at a time, in the kernels' own scaled arithmetic.  TEST INFRASTRUCTURE.

  stage 1  chunk c >= 1: the operator M_c = prod_{t in chunk} P diag(e_t) as K independently scaled rows (row j = the
           scaled filter from delta_j, renormalised every NORM-th step and at the end; log scale s_c[j]);  chunk 0: the
           filter from `init`
  stage 2  forward over the chunks: u = (a^_{c-1} o exp(s_c - max s_c)) M^_c, a^_c = u / sum u, log Z accumulates
           log sum u + max s_c;  backward: b^_{C-1} = 1, b_{c-1} = exp(s_c - max) o (M^_c b^_c), renormalised
  stage 3  per chunk the scaled forward-backward entered with a^_{c-1} and left with b^_c; the chunk adds the transition
           term of the step that enters it; E_trans = the chunks' counts summed in chunk order
  range    flagged (-> the serial route) if a live component falls below LOW or a normaliser to TINY or below

chunked_estep returns (logZ, (E_init, E_trans, E_states), flagged); what a flagged sequence returns is NOT what the
library returns for it (the library recomputes it with the serial kernels)."""
import numpy as np

LOW = 1e-250      # csrc/hmm_args.hpp HMM_LOW
TINY = 1e-200
NORM = 4          # stage 1 renormalises at chunk steps i with i % NORM == NORM - 1


def chunks_of(T, chunk):
    """[(first step, number of steps)] of the C = ceil(T / chunk) chunks"""
    return [(t0, min(chunk, T - t0)) for t0 in range(0, T, chunk)]


def workspace_doubles(B, T, K, chunk):
    """the closed form of svae_hmm_chunked_workspace_bytes / 8 (include/svae_hip.h)"""
    C = 1 if chunk >= T else -(-T // chunk)
    return B * (1 + T * (50 + K) + K * K + K + C * (2 * K * K + 3 * K))


def _scaled(pair, node):
    pmax = pair.max()
    with np.errstate(under="ignore"):
        P = np.exp(pair - pmax)
        m = node.max(axis=-1)
        e = np.exp(node - m[:, None])
    return P, pmax, e, m


def chunk_operators(init, pair, node, chunk):
    """stage 1 -> (ops (C,K,K), scale (C,K), flagged): ops[c][j] sums to 1 and M_c[j] = exp(scale[c][j]) ops[c][j];
    chunk 0 holds its filtered message and log scale in row 0"""
    T, K = node.shape
    P, pmax, _, _ = _scaled(pair, node)
    cks = chunks_of(T, chunk)
    ops, scale, bad = np.zeros((len(cks), K, K)), np.zeros((len(cks), K)), False
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        for c, (t0, n) in enumerate(cks):
            for j in range(K if c else 1):
                alpha = np.eye(K)[j] if c else None
                ls = 0.0
                for i in range(n):
                    nd = node[t0 + i] + (init if (c == 0 and i == 0) else 0.0)
                    m = nd.max()
                    e = np.exp(nd - m)
                    al = e.copy() if (c == 0 and i == 0) else (alpha @ P) * e
                    ls += m + (0.0 if (c == 0 and i == 0) else pmax)
                    if (c == 0 or i > 0) and not (al >= LOW).all():
                        bad = True
                    if i % NORM == NORM - 1:
                        cs = al.sum()
                        bad = bad or not cs > TINY
                        al, ls = al / cs, ls + np.log(cs)
                    alpha = al
                fs = alpha.sum()
                bad = bad or not fs > TINY
                ops[c, j], scale[c, j] = alpha / fs, ls + np.log(fs)
    return ops, scale, bad


def boundary_scan(ops, scale, backward=True):
    """stage 2 -> (logZ, ahat (C,K), bhat (C,K) or None, flagged)"""
    C, K, _ = ops.shape
    ahat, bad = np.zeros((C, K)), False
    ahat[0], logZ = ops[0, 0], scale[0, 0]
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        for c in range(1, C):
            smax = scale[c].max()
            w = ahat[c - 1] * np.exp(scale[c] - smax)
            u = w @ ops[c]
            su = u.sum()
            bad = bad or not (w >= LOW).all() or not (u >= LOW).all() or not su > TINY
            ahat[c], logZ = u / su, logZ + np.log(su) + smax
        bhat = None
        if backward:
            bhat = np.ones((C, K))
            for c in range(C - 1, 0, -1):
                bw = (ops[c] @ bhat[c]) * np.exp(scale[c] - scale[c].max())
                sb = bw.sum()
                bad = bad or not (bw >= LOW).all() or not sb > TINY
                bhat[c - 1] = bw / sb
    return logZ, ahat, bhat, bad


def chunk_esteps(init, pair, node, chunk, ahat, bhat):
    """stage 3 and the combine -> ((E_init, E_trans, E_states), flagged)"""
    T, K = node.shape
    P, _, _, _ = _scaled(pair, node)
    E_states, E_trans, bad = np.zeros((T, K)), np.zeros((K, K)), False
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        for c, (t0, n) in enumerate(chunks_of(T, chunk)):
            al_rec, u_rec = np.zeros((n, K)), np.zeros((n, K))
            alpha = ahat[c - 1] if c else None
            for i in range(n):
                nd = node[t0 + i] + (init if (c == 0 and i == 0) else 0.0)
                e = np.exp(nd - nd.max())
                al = e.copy() if (c == 0 and i == 0) else (alpha @ P) * e
                cs = al.sum()
                bad = bad or not (al >= LOW).all() or not cs > TINY
                alpha = al / cs
                al_rec[i], u_rec[i] = alpha, e / cs
            z = (alpha * bhat[c]).sum()
            bad = bad or not z > TINY
            beta = bhat[c] / z
            E_states[t0 + n - 1] = alpha * beta
            acc = np.zeros((K, K))
            for i in range(n - 2, -1, -1):
                w = u_rec[i + 1] * beta
                acc += np.outer(al_rec[i], w)
                beta = P @ w
                E_states[t0 + i] = al_rec[i] * beta
            if c:
                acc += np.outer(ahat[c - 1], u_rec[0] * beta)        # the transition into the chunk
            E_trans += acc * P                                       # (chunk order)
    return (E_states[0].copy(), E_trans, E_states), bad


def chunked_estep(natparam, chunk, want_stats=True):
    """(logZ, (E_init, E_trans, E_states) or None, flagged) of ONE sequence: init (K), pair (K,K), node (T,K), 2 <= chunk < T"""
    init, pair, node = (np.asarray(x, float) for x in natparam)
    assert 2 <= chunk < node.shape[0]
    ops, scale, bad1 = chunk_operators(init, pair, node, chunk)
    logZ, ahat, bhat, bad2 = boundary_scan(ops, scale, backward=want_stats)
    if not want_stats:
        return logZ, None, bad1 or bad2
    stats, bad3 = chunk_esteps(init, pair, node, chunk, ahat, bhat)
    return logZ, stats, bad1 or bad2 or bad3


def default_chunk(B, T, K):
    """svae_hmm_chunked_default_chunk's rule: serial (T) for K > 16, T < 500 or B > 128, else 2^round(log2(1.2 sqrt(T)))"""
    if B < 1 or T < 1 or K < 1 or K > 16 or T < 500 or B > 128:
        return T
    L = 2
    while 200 * L * L <= 144 * T:
        L *= 2
    return min(L, T)


# ---- the shapes and problems of the tests ------------------------------------------------------------------------------------
# (B, T, K, chunk): T = C L exactly, a one-step last chunk, C = 2, K = 1, B C not a multiple of the four rows of a wavefront
PARITY_SHAPES = [(1, 7, 3, 2), (5, 9, 2, 3), (3, 8, 8, 4), (2, 65, 2, 64), (9, 50, 8, 7), (4, 33, 16, 8), (13, 17, 9, 5),
                 (1, 12, 1, 4), (2, 500, 8, 32)]
PARITY_SCALE = 3.0


def problem(B, T, K, rng, scale=1.0):
    """tests/test_hmm_hip.py::_problem"""
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


def parity_problem(B, T, K, chunk, pair_batched):
    rng = np.random.default_rng(B * 100 + T + K + 1000 * chunk)
    init, pair, node = problem(B, T, K, rng, PARITY_SCALE)
    if pair_batched:
        pair = np.stack([problem(1, 1, K, rng)[1] for _ in range(B)])
    return init, pair, node


def range_batch():
    """K = 2, T = 40, chunk = 8, (B,K,K) pair parameters: the even-indexed sequences carry a -inf transition, a -800
    transition (the K = 2, T = 4 case of DESIGN 4.5 -- the only way into state 1 costs 800 nats and the evidence then
    pays for it -- embedded at steps 18 .. 21) or node potentials at 400 sigma; the odd-indexed ones are benign.
    -> init, pair (B,2,2), node (B,T,2), hostile (B) bool"""
    rng = np.random.default_rng(7)
    B, T, K = 6, 40, 2
    init = np.log(np.array([0.6, 0.4]))
    base = np.log(np.array([[0.7, 0.3], [0.2, 0.8]]))
    pair = np.stack([base] * B)
    node = rng.standard_normal((B, T, K))
    hostile = np.zeros(B, bool)
    hostile[0::2] = True
    pair[0, 1, 0] = -np.inf                         # state 1 absorbs
    pair[2] = np.array([[0.0, -800.0], [-800.0, 0.0]])
    node[2] = 0.1 * rng.standard_normal((T, K))
    node[2, :19, 1] -= 5.0                          # state 0 until step 18 ...
    node[2, 19:, 0] -= 1000.0                       # ... then the evidence pays for the -800 transition
    node[4] = 400.0 * rng.standard_normal((T, K))
    return init, pair, node, hostile
