"""Helpers of the ragged SLDS / per-step ragged LDS tests (tests/test_slds_ragged_cpu.py, test_lds_ragged_perstep_hip.py,
test_slds_ragged_hip.py), on oracle/lds_numpy.py and oracle/slds_numpy.py, which they import and leave as they are:

  * the construction behind svae_lds_ragged_perstep_*: a chain of T steps whose pairs t <= L-2 carry the caller's per-step
    pair parameters and whose pairs t >= L-1 carry the decoupling set Q = (0, 0, -1/2 I, 0), zero node potentials from
    step L on, the init potential passed whole;
  * the SLDS's own inputs: `slds_globals` / `slds_nodes` (the recipe of tests/test_slds_hip.py) and per-step pair
    parameters that are convex mixtures (Dirichlet weights per step) of K parameter sets;
  * the oracle's coordinate ascent on every sequence cut at its length, with the condition that makes equal sweep counts
    meaningful: the count must not move when the tolerance moves by 1e-3 relative.
"""
import numpy as np

from oracle import expfam_numpy as ef, lds_numpy, slds_numpy

try:        # the oracle works on n x n blocks: a BLAS thread pool only costs there
    from threadpoolctl import threadpool_limits
except ImportError:
    import contextlib
    threadpool_limits = lambda limits: contextlib.nullcontext()


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0


def slds_globals(K, n, rng):
    dir_nat = rng.random(K) * 2.
    mdir_nat = rng.random((K, K)) * 2. + 3. * np.eye(K)
    lds = []
    for k in range(K):
        nu, S = n + 1. + rng.random(), 2. * (n + 1) * np.eye(n)
        mu, kappa = 0.3 * rng.standard_normal(n), 0.5
        th = 0.4 * (k + 1)
        M = 0.95 * np.eye(n)
        if n >= 2:
            M[:2, :2] = 0.95 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        else:
            M[0, 0] = 0.95 * np.cos(th)
        Kmat = 0.2 * np.eye(n)
        lds.append((ef.niw_standard_to_natural(S, mu, np.array(kappa), np.array(nu)),
                    ef.mniw_standard_to_natural(nu, S, M, Kmat)))
    return (dir_nat, mdir_nat), lds


def slds_nodes(B, T, n, rng):
    J = -0.5 * (0.5 + rng.random((B, T, n)))
    h = rng.standard_normal((B, T, n)) * 2.
    return J, h


def mixed_lds_params(n, T, rng, lead=(), K=3):
    """The SLDS's own use of the per-step LDS: init potential (J, h, logZ) and per-step pair parameters (J11, J12, J22, logZ)
    as convex mixtures of K parameter sets (slds_globals), Dirichlet weights per (sequence,) step.  lead = () or (B,)."""
    _, lds = slds_globals(K, n, rng)
    inits, pairs = slds_numpy.get_all_lds_local_natparams(lds)
    w = rng.dirichlet(np.ones(K), size=tuple(lead) + (T,))                    # (..., T, K)
    mix = lambda ws, sets, i: np.tensordot(ws, np.stack([np.asarray(s[i], float) for s in sets]), axes=1)
    init = (mix(w[..., 0, :], inits, 0), mix(w[..., 0, :], inits, 1), mix(w[..., 0, :], inits, 2) + mix(w[..., 0, :], inits, 3))
    pair = tuple(mix(w[..., 1:, :], pairs, i) for i in range(4))
    return init, pair


def decoupled_pair_params(pair, T, L):
    """(T-1,..) per-step pair parameters of the padded chain: the caller's at t <= L-2, Q = (0, 0, -1/2 I, 0) at t >= L-1"""
    J11, J12, J22, logZ = (np.array(x, dtype=float, copy=True) for x in pair)
    n = J11.shape[-1]
    J11[L - 1:] = 0.0
    J12[L - 1:] = 0.0
    J22[L - 1:] = -0.5 * np.eye(n)
    logZ[L - 1:] = 0.0
    return J11, J12, J22, logZ


def padded_perstep_run(init, pair, node, L, eps=None):
    """E-step (and sampler) of the padded chain of T steps -> (lognorm, (E_init, E_pair, E_node), samples | None)"""
    T = np.asarray(node[1]).shape[0]
    nodes = tuple(np.array(x, dtype=float, copy=True) for x in node)
    for x in nodes:
        x[L:] = 0.0
    pp = decoupled_pair_params(pair, T, L)
    lognorm, stats = lds_numpy.natural_lds_estep_general((init, pp), nodes)
    samples = None
    if eps is not None:
        messages, _ = lds_numpy.natural_filter_forward_general(init, pp, lds_numpy._canonical_node_params(nodes))
        samples = lds_numpy.natural_sample_backward_general(messages, pp, eps)
    return lognorm, stats, samples


def cut_perstep_run(init, pair, node, L, eps=None):
    """The same on the sequence cut at L: pair parameters [:L-1], node potentials [:L], the init potential whole.
    E_pair: 3 arrays (L-1,n,n) (none for L = 1: the oracle's per-step path has no empty form; shared zero blocks stand in)."""
    nodes = tuple(np.asarray(x, float)[:L] for x in node)
    n = nodes[1].shape[1]
    if L > 1:
        pp = tuple(np.asarray(x, float)[:L - 1] for x in pair)
    else:
        pp = (np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n)), 0.0)
    lognorm, (Ei, Ep, En) = lds_numpy.natural_lds_estep_general((init, pp), nodes)
    if L == 1:
        Ep = tuple(np.zeros((0, n, n)) for _ in range(3))
    samples = None
    if eps is not None:
        messages, _ = lds_numpy.natural_filter_forward_general(init, pp, lds_numpy._canonical_node_params(nodes))
        samples = lds_numpy.natural_sample_backward_general(messages, pp, eps[:L])
    return lognorm, (Ei, Ep, En), samples


def slds_cut_ascent(glob, J, h, init_eps, lengths, compat=True, tol=1e-2, check_margin=True):
    """oracle.slds_numpy.optimize_local_meanfield on every sequence cut at its length -> list of result dicts.
    check_margin: the sweep count must be the same at tol (1 - 1e-3) and tol (1 + 1e-3) -- where the reference's own
    stopping test is marginal, equal counts say nothing about the code under test (asserted from the oracle alone)."""
    with threadpool_limits(limits=1):
        return _slds_cut_ascent(glob, J, h, init_eps, lengths, compat, tol, check_margin)


def _slds_cut_ascent(glob, J, h, init_eps, lengths, compat, tol, check_margin):
    out = []
    for b, L in enumerate(lengths):
        L = int(L)
        run = lambda t: slds_numpy.optimize_local_meanfield(glob, (J[b, :L], h[b, :L]), init_eps[b, :L], tol=t,
                                                            cython_init_logZ=compat)
        ref = run(tol)
        if check_margin:
            lo, hi = run(tol * (1 - 1e-3)), run(tol * (1 + 1e-3))
            assert lo["iters"] == ref["iters"] == hi["iters"], \
                "sequence %d (L = %d): the oracle's stopping test is marginal (%d / %d / %d sweeps)" % (
                    b, L, lo["iters"], ref["iters"], hi["iters"])
        out.append(ref)
    return out


def slds_global_stats_sum(refs):
    """sum over the sequences of the oracle's get_global_stats on the cut sequences -> ((Ei, Et), (g_init, g_pair))"""
    tot = None
    for ref in refs:
        (Ei, Et), (gi, gp) = slds_numpy.get_global_stats(ref["hmm_stats"], ref["init_stats"], ref["pair_stats"])
        cur = [Ei, Et, list(gi), list(gp)]
        if tot is None:
            tot = cur
        else:
            tot = [tot[0] + Ei, tot[1] + Et, [x + y for x, y in zip(tot[2], gi)], [x + y for x, y in zip(tot[3], gp)]]
    return (tot[0], tot[1]), (tuple(tot[2]), tuple(tot[3]))


def slds_lengths(T, B, rng):
    """2, T, 3 and T-1 first (as many as fit -- the SLDS has no one-step sequence), the remainder drawn in [2, T]; shuffled"""
    must = list(dict.fromkeys([2, T, min(3, T), max(T - 1, 2)]))[:B]
    rest = rng.integers(2, T + 1, size=B - len(must)).tolist()
    L = np.array(must + rest, dtype=np.int64)
    return L[rng.permutation(B)]


def slds_case(K, n, T, B, seed, S=2):
    """global parameters, node potentials, the two noise arrays and the lengths of one ragged SLDS batch"""
    rng = np.random.default_rng(seed)
    glob = slds_globals(K, n, rng)
    J, h = slds_nodes(B, T, n, rng)
    init_eps, eps = rng.standard_normal((B, T, 1, n)), rng.standard_normal((B, T, S, n))
    return dict(K=K, n=n, T=T, B=B, S=S, glob=glob, J=J, h=h, init_eps=init_eps, eps=eps, L=slds_lengths(T, B, rng))
