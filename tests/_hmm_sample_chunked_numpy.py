"""NumPy restatement of time-chunked HMM posterior sampling (svae_amd/csrc/hmm_sample_chunked.hip,
svae_hmm_chunked_sample_f64 in include/svae_hip.h), on top of tests/_hmm_chunked_numpy.py (operators, forward scan,
flags), and the cases of its tests.  TEST INFRASTRUCTURE.

  stage 1, 2  C.chunk_operators, C.boundary_scan(backward=False): a^_c, log Z, flags
  stage 3     per chunk the scaled filter entered with a^_{c-1} (chunk 0: init): records a_t, flags
  stage 4     per chain and step t >= 1 the map psi_t[k] = the state drawn at t-1 given z_t = k, from a_{t-1}, column k of
              exp(pair - M) and u[t-1]; z_{T-1} from a_{T-1} and u[T-1]; a flagged sequence: log-space records and weights
  stage 5     per chunk, from all K end states: cand[t][k], f_c[k]
  stage 6, 7  e_{C-1} = z_{T-1}, e_{c-1} = f_c[e_c];  states[t] = cand[t][e_{c(t)}]

The truth for labels is tests/_hmm_sample_numpy.sample_batch (the log-space oracle with its draw margins); for the long
cases long_truth below, a per-step-normalised log filter in np.longdouble (the fp64 oracle's unnormalised magnitudes grow
with T)."""
import functools

import numpy as np
from scipy.special import logsumexp

import _hmm_chunked_numpy as C
import _hmm_sample_numpy as smp

LOW, TINY = C.LOW, C.TINY

# (B, T, K, S, chunk, batched pair)
CASES = [(1, 5, 2, 1, 2, 0),            # one-step last chunk
         (1, 141, 3, 3, 2, 0),          # 71 chunks
         (2, 33, 4, 2, 4, 1),           # batched pair
         (3, 67, 5, 2, 16, 0),          # short last chunk
         (2, 100, 8, 3, 32, 1),         # batched pair
         (5, 130, 16, 2, 16, 0),        # more rows than a wavefront; K = 16
         (2, 131, 16, 3, 17, 1),        # chunk off the 16-step chase block
         (1, 1100, 8, 17, 32, 0),       # 35 chunks; S = 17 crosses wavefronts
         (3, 40, 1, 2, 8, 0),           # K = 1
         (7, 530, 7, 5, 33, 1),         # batched pair
         (1, 4401, 2, 2, 2, 0),         # 2201 chunks
         (130, 64, 8, 1, 8, 0)]         # beyond one ballot block
# (B, T, K, S): one long sequence; chunk None (the library's pick) and 256 (90 chunks, a one-step last chunk)
LONG_CASES = [(1, 22785, 8, 2), (1, 22785, 16, 2)]
LONG_CHUNKS = (None, 256)


def _freeze(*xs):
    for x in xs:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return xs


def _problem(B, T, K, S, pb):
    rng = np.random.default_rng(1000003 * K + 1009 * T + 17 * B + S)
    return smp.problem(B, T, K, S, rng, 1.0, batched_pair=bool(pb))


@functools.lru_cache(maxsize=None)
def case(B, T, K, S, chunk, pb):
    """-> init, pair, node, u, states, logZ, margin: the problem and the oracle's answer (computed once, read-only)"""
    init, pair, node, u = _problem(B, T, K, S, pb)
    return _freeze(init, pair, node, u, *smp.sample_batch(init, pair, node, u))


def r16(x):
    return (x + 15) // 16 * 16


def layout(B, T, K, S, chunk):
    """csrc/hmm_args.hpp hmm_chunked_sample_layout: byte offsets of the workspace's parts, and `total`"""
    Cn = 1 if chunk >= T else -(-T // chunk)
    R = B * S
    off, o = {}, 0
    for name, size in (("rec", 128 * B * T), ("lz", r16(8 * B)), ("route", r16(4 * B)), ("ops", r16(8 * B * Cn * K * K)),
                       ("scale", r16(8 * B * Cn * K)), ("ahat", r16(8 * B * Cn * K)), ("maps", 16 * R * T),
                       ("cand", 16 * R * T), ("fmap", 16 * R * Cn), ("ends", r16(R * Cn))):
        off[name], o = o, o + size
    off["total"], off["C"] = o, Cn
    return off


def workspace_bytes(B, T, K, S, chunk):
    """the closed form of svae_hmm_chunked_sample_workspace_bytes (include/svae_hip.h)"""
    if B <= 0 or T <= 0 or K <= 0 or K > 16 or S <= 0 or chunk < 2:
        return 0
    Cn = 1 if chunk >= T else -(-T // chunk)
    R = B * S
    return (128 * B * T + r16(8 * B) + r16(4 * B) + r16(8 * B * Cn * K * K) + 2 * r16(8 * B * Cn * K) + 32 * R * T + 16 * R * Cn
            + r16(R * Cn))


def default_chunk(B, T, K, S):
    """svae_hmm_chunked_sample_default_chunk's rule: the chunked E-step's applied to B; T for what the entry refuses"""
    if S < 1 or B < 1 or T < 1 or B * S * T >= 2 ** 31:
        return T
    return C.default_chunk(B, T, K)


def chunk_filter(init, pair, node, chunk, ahat):
    """stage 3 -> (records (T,K), flagged)"""
    T, K = node.shape
    with np.errstate(under="ignore"):
        P = np.exp(pair - pair.max())
    rec, bad = np.zeros((T, K)), False
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        for c, (t0, n) in enumerate(C.chunks_of(T, chunk)):
            alpha = ahat[c - 1] if c else None
            for i in range(n):
                nd = node[t0 + i] + (init if (c == 0 and i == 0) else 0.0)
                e = np.exp(nd - nd.max())
                al = e.copy() if (c == 0 and i == 0) else (alpha @ P) * e
                cs = al.sum()
                bad = bad or not (al >= LOW).all() or not cs > TINY
                alpha = al / cs
                rec[t0 + i] = alpha
    return rec, bad


def _count(w, uu):
    """the selection rule on weights w (..., K): #{j : C[j] <= thr and C[j] < C[K-1]}"""
    Cs = np.cumsum(w, axis=-1)
    tot = Cs[..., -1:]
    thr = uu * tot
    return ((Cs <= thr) & (Cs < tot)).sum(-1)


def state_maps(pair, rec, u, is_log):
    """stage 4 for one chain -> (psi (T,K) uint8 with psi[0] = 0, z_last): psi[t][k] from rec[t-1], column k, u[t-1]"""
    T, K = rec.shape
    uu = np.clip(np.where(np.isnan(u), 0.0, u), 0.0, 1.0)
    psi = np.zeros((T, K), np.uint8)
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        E = np.exp(pair - pair.max())                        # E[j][k]
        la = rec if is_log else np.where(rec > 0, np.log(np.where(rec > 0, rec, 1.0)), -np.inf)

        def logw(x):                                         # x (..., K) over j
            m = x.max(-1, keepdims=True)
            return np.where(m > -np.inf, np.exp(x - np.where(m > -np.inf, m, 0.0)), 0.0)

        for t in range(1, T):
            w = rec[t - 1][None, :] * E.T                    # [k][j] = a[j] E[j][k]
            tot = np.cumsum(w, -1)[:, -1]
            under = ~(tot >= TINY)
            z = _count(w, uu[t - 1])
            if under.any():
                z = np.where(under, _count(logw(la[t - 1][None, :] + pair.T), uu[t - 1]), z)
            psi[t] = z
        w = rec[T - 1]
        tot = np.cumsum(w)[-1]
        z_last = int(_count(w, uu[T - 1])) if tot >= TINY else int(_count(logw(la[T - 1]), uu[T - 1]))
    return psi, z_last


def chase_resolve_gather(psi, z_last, chunk):
    """stages 5 - 7 for one chain -> states (T) int32"""
    T, K = psi.shape
    cks = C.chunks_of(T, chunk)
    cand, fmap = np.zeros((T, K), np.uint8), np.zeros((len(cks), K), np.uint8)
    for c, (t0, n) in enumerate(cks):
        z = np.arange(K)
        for i in range(n - 1, -1, -1):
            cand[t0 + i] = z
            z = psi[t0 + i][z]
        fmap[c] = z
    ends = np.zeros(len(cks), np.int64)
    ends[-1] = z_last
    for c in range(len(cks) - 1, 0, -1):
        ends[c - 1] = fmap[c][ends[c]]
    return np.array([cand[t][ends[t // chunk]] for t in range(T)], np.int32)


def chunked_sample(init, pair, node, u, chunk):
    """ONE sequence: init (K), pair (K,K), node (T,K), u (S,T), 2 <= chunk < T -> (states (S,T) int32, logZ, flagged).  A
    flagged sequence takes the log-space records (scipy's filter) and the log-space weights, as the library's does."""
    init, pair, node, u = (np.asarray(x, float) for x in (init, pair, node, u))
    T, K = node.shape
    assert 2 <= chunk < T
    ops, scale, bad1 = C.chunk_operators(init, pair, node, chunk)
    logZ, ahat, _, bad2 = C.boundary_scan(ops, scale, backward=False)
    rec, bad3 = chunk_filter(init, pair, node, chunk, ahat)
    flagged = bool(bad1 or bad2 or bad3)
    if flagged:
        with np.errstate(invalid="ignore", divide="ignore"):
            la = smp.log_filter(init, pair, node[None])[0]
            c = logsumexp(la, axis=1, keepdims=True)
            rec = np.minimum(la - c, 0.0)
            logZ = float(c[-1, 0])
    states = np.empty((u.shape[0], T), np.int32)
    for s in range(u.shape[0]):
        psi, z_last = state_maps(pair, rec, u[s], flagged)
        states[s] = chase_resolve_gather(psi, z_last, chunk)
    return states, logZ, flagged


def chunked_sample_batch(init, pair, node, u, chunk):
    """-> states (B,S,T), logZ (B), flagged (B)"""
    B = node.shape[0]
    pair = np.asarray(pair, float)
    out = [chunked_sample(init, pair[b] if pair.ndim == 3 else pair, node[b], u[b], chunk) for b in range(B)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ---- long sequences: the truth in np.longdouble ------------------------------------------------------------------------------
def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    mm = np.where(np.isfinite(m), m, 0)
    with np.errstate(divide="ignore"):
        return np.squeeze(mm, axis) + np.log(np.exp(x - mm).sum(axis=axis))


def long_truth(init, pair, node, u):
    """ONE sequence, per-step-normalised log filter and log-space draw in np.longdouble: pair (K,K), node (T,K), u (S,T)
    -> states (S,T) int32, logZ (float), the minimum draw margin (as smp.sample_batch defines it)"""
    ld = np.longdouble
    init, pair, node, u = (np.asarray(x, ld) for x in (init, pair, node, u))
    T, K = node.shape
    S = u.shape[0]
    la = np.empty((T, K), ld)
    logZ = ld(0)
    x = init + node[0]
    for t in range(T):
        if t:
            x = _lse(la[t - 1][:, None] + pair, 0) + node[t]
        c = _lse(x, 0)
        la[t], logZ = x - c, logZ + c
    states = np.empty((S, T), np.int32)
    margin = np.inf
    z = None
    for t in range(T - 1, -1, -1):
        lw = np.broadcast_to(la[t][None, :], (S, K))
        if t < T - 1:
            lw = lw + pair[:, z].T                                   # pair[k][z_{t+1}]: (S,K)
        w = np.exp(lw - lw.max(-1, keepdims=True))
        Cs = np.cumsum(w, axis=-1)
        tot = Cs[:, -1]
        thr = np.clip(u[:, t], 0, 1) * tot
        z = np.minimum((Cs <= thr[:, None]).sum(-1), K - 1)
        states[:, t] = z
        margin = min(margin, float((np.abs(Cs - thr[:, None]).min(-1) / tot).min()))
    return states, float(logZ), margin


@functools.lru_cache(maxsize=None)
def long_case(B, T, K, S):
    """-> init, pair, node, u, states (B,S,T), logZ (B), margin from long_truth (computed once, read-only)"""
    init, pair, node, u = _problem(B, T, K, S, 0)
    out = [long_truth(init, pair, node[b], u[b]) for b in range(B)]
    return _freeze(init, pair, node, u, np.stack([o[0] for o in out]), np.array([o[1] for o in out]),
                   min(o[2] for o in out))
