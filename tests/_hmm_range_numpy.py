"""HMM problems on which a SCALED forward-backward loses mass without its normaliser noticing, and their log-space
references (oracle/hmm_numpy.hmm_estep).  A scaled recursion exponentiates shifted log-potentials: an entry more than
745 nats below the maximum is exactly 0, a message component below 1e-308 of the step's total is flushed, and a component
lost is never rebuilt -- the chain stays in the wrong state while every normaliser looks ordinary.

Every family has its "story" in states 0 and 1 (sparse_case: in the states the evidence visits); the states beyond them
carry ordinary random potentials and hold mass.  node[0] = 0 in every case (the fused SLDS route builds node[0] from
other inputs).  The cases (generators, seeds, shapes) and their lru_cache'd references live here so that
tests/test_hmm_range_cpu.py and tests/test_hmm_range_hip.py share one computation of each.

  gap_case       the only way into state 1 is a transition of -g; from step t0 on every other state loses g/2 per step
  surprise_case  gap_case with r steps before the event whose observed state (2) has predicted mass e^-s: a message that
                 is renormalised every 4th step only shrinks by e^-(r s) on top of the e^-g of state 1   (K >= 3: a
                 surprise needs a third state to be surprised by)
  sparse_case    transitions E[log pi] of a sparse Dirichlet row (psi(conc) - psi(50) ~ -1/conc); evidence hops to the next
                 state every `seg` steps (and stays on the last one: with K = 2 a way back would cost a second transition)
  ramp_case      gap_case whose evidence for state 1 arrives at ev nats per step over n steps
  mixed_batch    sparse_case rows among ordinary sequences, 0 / 1 / 2 / 4 of them in a block of four rows
"""
import functools

import numpy as np
from scipy.special import digamma

from oracle import hmm_numpy

DEEP = 745.0            # exp(-745.2) is the last fp64 denormal: a potential this far below the maximum is (nearly) 0
K_ROW = (2, 3, 8, 9, 16)          # DPP-row kernels
K_WIDE = (17, 32, 33, 64)         # one wavefront per sequence
GAP_G = (100.0, 200.0, 300.0, 400.0, 460.0, 600.0, 700.0, 745.0, 800.0, 1200.0, 3000.0)
GAP_T = (4, 12, 13, 37)
SURPRISE_G, SURPRISE_S, SURPRISE_R, SURPRISE_T0 = (460.0, 600.0), (60.0, 140.0), (1, 2, 3), (9, 10, 11, 12)
SPARSE = ((1e-2, 20.0, 8), (2e-3, 100.0, 8), (1e-3, 200.0, 8), (5e-4, 400.0, 8))     # (conc, ev, seg): ev seg = 1.6 / conc
RAMP = ((600.0, 50.0, 18), (800.0, 50.0, 24), (1200.0, 50.0, 36), (800.0, 200.0, 6))  # (g, ev, n): ev n = 1.5 g


def gap_t0(T):
    """the event starts of gap_case at length T: eight consecutive steps (every ring position and both renormalisation
    phases of a kernel that works in rounds of eight), inside the steady loop for T = 12 / 13, across the tail for T = 37;
    T = 4 has room for two"""
    return {4: (1, 2), 12: tuple(range(2, 10)), 13: tuple(range(3, 11)), 37: tuple(range(27, 35))}[T]


@functools.lru_cache(maxsize=None)
def _base(K):
    """ordinary potentials of the states beyond the story: init (K), pair (K,K), a (64, K) block of node noise"""
    rng = np.random.default_rng(7000 + K)
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    noise = 0.5 * rng.standard_normal((64, K))
    init[0] = 0.0
    pair[0, 0] = 0.0
    noise[:, :2] = 0.0
    return init, pair, noise


def _gate(K, g):
    """init and pair of the gap / surprise / ramp families: state 1 starts forbidden, every way into it costs g, it
    stays (0) or leaves at -5"""
    init, pair, noise = (x.copy() for x in _base(K))
    init[1] = -1e4
    pair[:, 1] = -g
    pair[1, :] = -5.0
    pair[1, 1] = 0.0
    return init, pair, noise


def gap_case(K, g, t0, T):
    assert K >= 2 and 1 <= t0 and T - t0 >= 2
    init, pair, noise = _gate(K, g)
    node = noise[:T].copy()
    node[0] = 0.0
    others = np.arange(K) != 1
    node[t0:, others] -= g / 2
    return init, pair, node


def surprise_case(K, g, s, r, t0=10, T=16):
    assert K >= 3 and t0 - r >= 1 and T - t0 >= 3
    init, pair, noise = _gate(K, g)
    pair[:, 2] = -s                      # state 2 always has predicted mass e^-s ...
    pair[1, 2] = -5.0 - s
    pair[:, 1] = -g
    pair[1, 1] = 0.0
    node = noise[:T].copy()
    node[:, 2] = 0.0
    node[0] = 0.0
    node[t0 - r:t0, np.arange(K) != 2] -= s          # ... and is what the r steps before the event observe
    node[t0:, np.arange(K) != 1] -= g / 2
    return init, pair, node


def sparse_pair(K, conc):
    a = conc + 50.0 * np.eye(K)
    return digamma(a) - digamma(a.sum(1, keepdims=True))


def sparse_case(K, conc, ev, seg, T=24, seed=0):
    rng = np.random.default_rng(9000 + 10 * K + seed)
    init = np.full(K, -np.log(K))
    node = 0.5 * rng.standard_normal((T, K))
    for t in range(T):
        node[t, min(t // seg, K - 1)] += ev
    node[0] = 0.0
    return init, sparse_pair(K, conc), node


def ramp_case(K, g, ev, n, t0=3, T=None):
    T = t0 + n + 3 if T is None else T
    assert K >= 2 and T >= t0 + n
    init, pair, noise = _gate(K, g)
    node = noise[:T].copy()
    node[0] = 0.0
    node[t0:t0 + n, 1] += ev
    return init, pair, node


def ordinary(B, T, K, rng, scale=1.0):
    """tests/test_hmm_hip.py::_problem"""
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


FAMILIES = {"gap": gap_case, "surprise": surprise_case, "sparse": sparse_case, "ramp": ramp_case}


@functools.lru_cache(maxsize=None)
def case(family, *args):
    """-> (init, pair, node) of one sequence, read-only"""
    out = FAMILIES[family](*args)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(family, *args):
    """-> logZ, (E_init, E_trans, E_states) of oracle/hmm_numpy.hmm_estep"""
    return _oracle(*case(family, *args))


def _oracle(init, pair, node):
    with np.errstate(all="ignore"):
        return hmm_numpy.hmm_estep((init, pair, node))


def deep_mass(pair, E_trans):
    """posterior mass (expected number of transitions) on entries >= DEEP below the matrix' maximum"""
    return float(E_trans[pair - pair.max() <= -DEEP].sum())


def by_construction_extreme(family, *args):
    """is the case beyond a scaled recursion that renormalises EVERY step?  gap / ramp / sparse: the story goes through a
    transition >= DEEP below the maximum; surprise: state 1's component e^-g meets a likelihood e^-s in the surprise
    steps, g + s > 700 nats below the step's best (no deep transition)"""
    if family in ("gap", "ramp"):
        return args[1] >= DEEP
    if family == "sparse":
        return args[1] <= 1e-3
    return args[1] + args[2] > 700.0


# tolerances of the GPU file for sequences the kernels may have redone in log space
LZ_REL, ST_RTOL, ST_ATOL, TR_ATOL = 1e-9, 1e-7, 1e-10, 1e-9


def off(got, want, factor):
    """is a scaled result (scaled_emulation) non-finite, or further than `factor` x the GPU tolerances from the oracle's?"""
    lz, (_, et, es), _ = got
    wz, (_, wt, ws) = want
    if not (np.isfinite(lz) and np.isfinite(es).all() and np.isfinite(et).all()):
        return True
    return bool(abs(lz - wz) > factor * LZ_REL * abs(wz) or (np.abs(es - ws) > factor * (ST_ATOL + ST_RTOL * np.abs(ws))).any()
                or (np.abs(et - wt) > factor * (TR_ATOL + ST_RTOL * np.abs(wt))).any())


def beyond_range(init, pair, node, want):
    """must a kernel with scaled recursions have left them for this sequence?  Yes if the oracle's posterior uses a deep
    transition (deep_mass > 0.1) or the per-step scaled recursion is more than 100x the GPU tolerances off"""
    return deep_mass(pair, want[1][1]) > 0.1 or off(scaled_emulation(init, pair, node), want, 100.0)


def four_step_off(init, pair, node, want):
    """is log Z of the two-ended kernel's schedule (renormalisation every fourth step) more than 100x the tolerance off?"""
    lz4 = scaled_logZ(init, pair, node)
    return bool(not np.isfinite(lz4) or abs(lz4 - want[0]) > 100 * LZ_REL * abs(want[0]))


def deterministic(E_states):
    return bool((E_states.max(-1) > 1 - 1e-9).all())


# ---- batches ------------------------------------------------------------------------------------------------------------
def stack(keys):
    """sequences of one K, one T and one init as a batch with per-sequence transition matrices:
    -> init (K), pair (B,K,K), node (B,T,K), refs [(logZ, (E_init, E_trans, E_states))], extreme (B) bool"""
    cs = [case(*k) for k in keys]
    assert all(np.array_equal(c[0], cs[0][0]) and c[2].shape == cs[0][2].shape for c in cs)
    return (cs[0][0], np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), [reference(*k) for k in keys],
            np.array([by_construction_extreme(*k) for k in keys]))


def gap_keys(K, T, g_set):
    return [("gap", K, g, t0, T) for g in g_set for t0 in gap_t0(T)]


def surprise_keys(K):
    return [("surprise", K, g, s, r, t0) for g in SURPRISE_G for s in SURPRISE_S for r in SURPRISE_R for t0 in SURPRISE_T0]


def sparse_keys(K):
    return [("sparse", K, conc, ev, seg, 24, seed) for conc, ev, seg in SPARSE for seed in (0, 1)]


def ramp_keys(K):
    """one T per batch: the shorter ramps are padded to the longest (quiet steps after the ramp)"""
    T = max(3 + n + 3 for _, _, n in RAMP)
    return [("ramp", K, g, ev, n, t0, T) for g, ev, n in RAMP for t0 in (3, 4, 5, 6)]


def cut(init, pair, node, L):
    """a sequence cut at length L, as its own problem"""
    return init, pair, node[:L]


@functools.lru_cache(maxsize=None)
def ragged_lengths(B, T, seed):
    """lengths for a batch of B sequences of T steps: T, 1, 2, random ones, and T for the last (every batch of keys ends
    with its most extreme case: it stays whole)"""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, T + 1, size=B)
    L[0] = T
    if B > 1:
        L[1] = 1
    if B > 2:
        L[2] = 2
    if B > 3:
        L[B - 1] = T
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def mixed_batch(K, variant):
    """Extreme rows (T = 24) among ordinary sequences (`ordinary`, scale 1); B = 11 for K <= 16 (blocks of four rows: the
    DPP-row kernels' wavefronts), 5 for K >= 17.  The init potential is shared and uniform, so the gap / ramp / surprise
    rows of the per-sequence-matrix variants carry their forbidden start of state 1 in node[0] instead.
      "shared"   one transition matrix (the sparse one: ordinary rows are ordinary in their node potentials), blocks with
                 0, 1 and 2 extreme rows
      "shared4"  the same, blocks with 4, 0 and 1 extreme rows
      "batched"  per-sequence matrices; the extreme rows are sparse (1e-3), gap (g = 800, event at t0 = 8), ramp (g = 800,
                 200 nats over 6 steps), surprise (g = 600, s = 140, r = 3; K = 2: a second gap, t0 = 13) and sparse (5e-4)
                 -- K >= 17: sparse, gap, surprise --, `ordinary` matrices for the others (4, 0, 1)
      "ragged"   "batched" with lengths: the sparse row cut before its first hop (L = 8), the gap row two steps after its
                 event (L = 10), others 1, 2 and T; node potentials NaN from a row's length on
    -> dict(init, pair, node, lengths or None, refs, extreme (B) bool: beyond_range of the sequence cut to its length)"""
    T, seg = 24, 8
    B = 11 if K <= 16 else 5
    rng = np.random.default_rng(31000 + K)
    _, opair0, onode = ordinary(B, T, K, rng)
    init = np.full(K, -np.log(K))
    if K <= 16:
        ext = (5, 8, 10) if variant == "shared" else (0, 1, 2, 3, 9)
    else:
        ext = (1, 3) if variant in ("shared", "shared4") else (0, 1, 4)
    concs = (1e-3, 5e-4) if variant in ("batched", "ragged") else (1e-3,)
    node = onode.copy()
    node[:, 0] = 0.0
    pairs = np.stack([ordinary(1, 1, K, rng)[1] for _ in range(B)])
    if variant in ("batched", "ragged"):
        third = ("surprise", K, 600.0, 140.0, 3, 10, T) if K >= 3 else ("gap", K, 800.0, 13, T)
        fam = [None, ("gap", K, 800.0, 8, T), ("ramp", K, 800.0, 200.0, 6, 4, T), third, None]
        fam = fam if K <= 16 else [None, fam[1], third]
    else:
        fam = [None] * len(ext)
    n_sparse = 0
    for i, b in enumerate(ext):
        if fam[i] is None:
            conc = concs[n_sparse % len(concs)]
            n_sparse += 1
            node[b] = sparse_case(K, conc, 0.2 / conc, seg, T, seed=10 + i)[2]
            pairs[b] = sparse_pair(K, conc)
        else:
            _, pairs[b], nd = FAMILIES[fam[i][0]](*fam[i][1:])
            node[b] = nd
            node[b, 0, 1] = -1e4
    pair = pairs if variant in ("batched", "ragged") else sparse_pair(K, 1e-3)
    lengths = None
    if variant == "ragged":
        lengths = np.full(B, T)
        lengths[ext[0]] = seg                # cut before the event
        lengths[ext[1]] = seg + 2            # ... just after it
        free = [b for b in range(B) if b not in ext]
        lengths[free[0]], lengths[free[1]] = 1, 2
        for b in range(B):
            node[b, lengths[b]:] = np.nan
    refs, extreme = [], []
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        pb = pair[b] if pair.ndim == 3 else pair
        r = _oracle(init, pb, node[b, :L])
        refs.append(r)
        extreme.append(beyond_range(init, pb, node[b, :L], r))
    for x in (init, pair, node):
        x.setflags(write=False)
    return dict(init=init, pair=pair, node=node, lengths=lengths, refs=refs, extreme=np.array(extreme), ext=ext)


# ---- what a scaled recursion makes of a case ----------------------------------------------------------------------------
def scaled_emulation(init, pair, node):
    """The plain scaled forward-backward: shift by the maximum, exponentiate, renormalise EVERY step, divide by the stored
    normalisers -> logZ, (E_init, E_trans, E_states), the smallest normaliser.  Only here to show that the cases have teeth."""
    init, pair, node = (np.asarray(x, float) for x in (init, pair, node))
    T, K = node.shape
    with np.errstate(all="ignore"):
        pmax = pair.max()
        P = np.exp(pair - pmax)
        x = node.copy()
        x[0] = x[0] + init
        m = x.max(1)
        e = np.exp(x - m[:, None])
        alpha, c = np.empty((T, K)), np.empty(T)
        al = e[0]
        c[0] = al.sum()
        alpha[0] = al / c[0]
        for t in range(1, T):
            al = (alpha[t - 1] @ P) * e[t]
            c[t] = al.sum()
            alpha[t] = al / c[t]
        logZ = np.log(c).sum() + m.sum() + (T - 1) * pmax
        beta = np.ones(K)
        E_states = np.empty((T, K))
        E_states[T - 1] = alpha[T - 1]
        E_trans = np.zeros((K, K))
        for t in range(T - 2, -1, -1):
            w = e[t + 1] * beta / c[t + 1]
            E_trans += alpha[t][:, None] * P * w[None, :]
            beta = P @ w
            E_states[t] = alpha[t] * beta
    return logZ, (E_states[0], E_trans, E_states), float(c.min())


def scaled_logZ(init, pair, node, every=4, rounds=8):
    """log Z of a scaled forward pass that renormalises only at steps t with (t % rounds) % every == every - 1 (and once
    at the end) -- the two-ended kernel's schedule"""
    init, pair, node = (np.asarray(x, float) for x in (init, pair, node))
    T, K = node.shape
    with np.errstate(all="ignore"):
        pmax = pair.max()
        P = np.exp(pair - pmax)
        x = node.copy()
        x[0] = x[0] + init
        m = x.max(1)
        e = np.exp(x - m[:, None])
        al, lz = e[0], 0.0
        for t in range(T):
            if t > 0:
                al = (al @ P) * e[t]
            if (t % rounds) % every == every - 1 or t == T - 1:
                c = al.sum()
                lz += np.log(c)
                al = al / c
        return lz + m.sum() + (T - 1) * pmax
