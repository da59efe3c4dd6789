"""The draws, fixtures and judge shared by tests/golden/make_golden_lds_mfma_truth.py, tests/test_lds_mfma_truth_cpu.py
and tests/test_lds_mfma_truth_hip.py: the MFMA LDS paths (tile kernels n = 16 .. 64, XL kernel n = 65 .. 128) against the
50-digit oracle oracle/lds_mp.py, precomputed into tests/golden/lds_mfma_truth_<n>_<form>_<draw>.npz.

Metric and rule are tests/test_lds_truth_hip.py's (imported, not restated): normwise distance per output array, and
HIP-vs-truth <= max(3 x comparator-vs-truth, 1e-11)."""
import hashlib
import os

import numpy as np

try:        # rand_lds_natparam's products and inverses at n >= 97 round differently with the number of BLAS threads: the
    from threadpoolctl import threadpool_limits         # fixtures' inputs (and their hash) are the one-thread ones
except ImportError:
    import contextlib
    threadpool_limits = lambda limits: contextlib.nullcontext()

from test_lds_truth_hip import FLOOR, _cond_eps_rule, _dist, _distances, _stats_arrays, _sym_blocks, _symmetric_model  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# latent dimension -> NB = ceil(n / 16), the launch_tile<NB> / XL instance: a full and a padded size per instance
TILE_N, TILE_T, TILE_PERSTEP = (17, 32, 33, 48, 63, 64), 4, (33, 64)
XL_N, XL_T, XL_PERSTEP = (65, 96, 97, 128), 3, (65, 128)
DRAW_KINDS = ("ill", "median")
NUM_SAMPLES = 2
RESTATEMENT_BOUND = 1e-9        # an ill draw keeps the fp64 restatement within this of the truth on every statistics array
# A median draw is one "where the 1e-11 floor binds": 3 x an fp64 evaluation's distance to the truth stays below the floor,
# so the fp64 restatement has to be within FLOOR / 3 on every statistics array.  cond(J22) alone does not see to that: at
# n = 128 per-step the seed of median cond(J22) (90) has an ill-conditioned INIT block (cond(J0) 3.2e8, |h_0| 1.4e5 against
# |E[x_0]| 5.6) and the restatement is at 1.2e-10 there.  The generator takes the seed nearest the median that meets the
# condition; seed 90 stays as a fixture of its own (EXTRA_DRAWS), because the XL kernel misses the rule on it.
MEDIAN_BOUND = FLOOR / 3
# n64_perstep_illinit is the tile path's counterpart of seed 90: the seed of largest cond(J0) (draw kind "illinit") that
# meets the ill draws' condition, RESTATEMENT_BOUND.
EXTRA_DRAWS = (("n64_perstep_illinit", "tile", 64, 4, "perstep", "illinit"),
               ("n128_perstep_s90", "xl", 128, 3, "perstep", "seed90"))
GAP_FACTOR, GAP_FLOOR = 30.0, 1e-10


def fixture_names(path=None):
    """[(name, path kind, n, T, form, draw kind)] of every fixture, tile ones first; draw kind "ill", "median", or
    "seed<k>" for a fixed seed, "illinit" (EXTRA_DRAWS)"""
    out = []
    for kind, ns, T, perstep in (("tile", TILE_N, TILE_T, TILE_PERSTEP), ("xl", XL_N, XL_T, XL_PERSTEP)):
        if path in (None, kind):
            for n in ns:
                for form in ("homog", "perstep") if n in perstep else ("homog",):
                    out += [("n%d_%s_%s" % (n, form, d), kind, n, T, form, d) for d in DRAW_KINDS]
    return out + [f for f in EXTRA_DRAWS if path in (None, f[1])]


def fixture_path(name):
    return os.path.join(GOLDEN, "lds_mfma_truth_%s.npz" % name)


def model(n, T, seed, form):
    """(init, pair), node of one sequence: rand_lds_natparam + rand_node_potentials((T, n), with_logZ=True) from
    default_rng(seed), J0 / J11 / J22 exactly symmetric; form "perstep": step t takes the t % 3-th of three draws' pair
    blocks (tests/test_oracle.py's _mp_model)"""
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    rng = np.random.default_rng(seed)
    with threadpool_limits(limits=1):
        init, pair = rand_lds_natparam(n, rng)
        draws = [pair] + [rand_lds_natparam(n, rng)[1] for _ in range(2)] if form == "perstep" else None
    if form == "perstep":
        steps = [draws[t % 3] for t in range(T - 1)]
        pair = tuple(np.stack([s[k] for s in steps]) for k in range(3)) + (np.array([float(s[3]) for s in steps]),)
    else:
        assert form == "homog"
    init, pair = _symmetric_model(init, pair)
    init = (init[0], np.asarray(init[1], float), float(init[2]))
    node = rand_node_potentials((T, n), rng, with_logZ=True)
    return (init, pair), node


def cond_J22(pair):
    """cond(J22); per-step pair parameters: the worst step's"""
    return float(np.max(np.linalg.cond(np.asarray(pair[2], float))))


def input_hash(natparam, node):
    """SHA-256 over the bytes of init J, h, logZ, pair J11, J12, J22, logZ and node J, h, logZ as contiguous float64"""
    h = hashlib.sha256()
    for a in tuple(natparam[0]) + tuple(natparam[1]) + tuple(node):
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def noise(seed, T, n):
    """the sampler's noise of a tile fixture: (T, NUM_SAMPLES, n), eps[t] the draw applied at time t"""
    return np.random.default_rng(seed + 1).standard_normal((T, NUM_SAMPLES, n))


def cotangents(seed, T, n):
    """g_l, g_d (T,n), g_x (T,n), g_s (T,S,n) and two dense directions (2,T,n) on the node J"""
    rng = np.random.default_rng(seed + 2)
    return (float(rng.standard_normal()), rng.standard_normal((T, n)), rng.standard_normal((T, n)),
            rng.standard_normal((T, NUM_SAMPLES, n)), rng.standard_normal((2, T, n)))


def load(name):
    """the fixture as a dict, its model regenerated from the seed and checked against the stored hash"""
    with np.load(fixture_path(name)) as z:
        fx = {k: z[k] for k in z.files}
    for k in ("n", "T", "seed"):
        fx[k] = int(fx[k])
    fx["form"], fx["sha256"], fx["cond"] = str(fx["form"]), str(fx["sha256"]), float(fx["cond"])
    fx["natparam"], fx["node"] = model(fx["n"], fx["T"], fx["seed"], fx["form"])
    got = input_hash(fx["natparam"], fx["node"])
    assert got == fx["sha256"], ("the inputs of %s no longer regenerate to the stored hash (other NumPy / BLAS build? at n >= 97 "
                                 "also: threadpoolctl missing, so that the draw did not run on one BLAS thread)" % name,
                                 got, fx["sha256"])
    return fx


STATS_KEYS = ("lognorm", "ExxT0", "Ex0", "Epair_xx", "Epair_xxn", "Epair_xnxn", "Enode_diagxx", "Enode_x")


def truth_arrays(fx):
    return {k: fx[k] for k in STATS_KEYS}


def fp64_distances(fx):
    return {k: float(fx["fp64_" + k]) for k in STATS_KEYS}


def judge(hip, want, what, gaps=()):
    """per output array HIP-vs-truth <= max(3 x comparator-vs-truth, 1e-11); an array named in `gaps` (an open gap, listed
    with its measurement by the caller) <= max(30 x comparator-vs-truth, 1e-10) instead -- never a multiple of the
    kernel's own figure"""
    for k in hip:
        if k in gaps:
            assert hip[k] <= max(GAP_FACTOR * want[k], GAP_FLOOR), (what, k, hip[k], want[k], "open gap bound")
        else:
            _cond_eps_rule({k: hip[k]}, {k: want[k]}, what)


# ---------------------------------------------------------------------------------------------- gradient directions (fp64)
def autograd_node_grads(natparam, node, eps, cot, sampler=True):
    """node-J / node-h gradients (T,n) of L = g_l lognorm + <g_d, diag E[xx']> + <g_x, E[x]> [+ <g_s, samples>] by fp64 CPU
    autograd of tests/_lds_large_torch.torch_estep"""
    import torch
    import _lds_large_torch as lt
    (init, pair), (g_l, g_d, g_x, g_s) = natparam, cot[:4]
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64)
    params = (t(init[0]), t(init[1]), t(init[2]).reshape(1), t(pair[0]), t(pair[1]), t(pair[2]), t(pair[3]).reshape(-1))
    nJ, nh = t(node[0])[None].requires_grad_(True), t(node[1])[None].requires_grad_(True)
    ln, dxx, x, smp = lt.torch_estep(params, nJ, nh, eps=t(eps)[None] if sampler else None)[:4]
    loss = (ln * g_l).sum() + (dxx[0] * t(g_d)).sum() + (x[0] * t(g_x)).sum()
    if sampler:
        loss = loss + (smp[0] * t(g_s)).sum()
    loss.backward()
    return nJ.grad[0].numpy(), nh.grad[0].numpy()


def directions(gJ, dense):
    """(K,T,n), K <= 6: unit directions at the largest |gJ| entry, its largest in the last real row (latent index n - 1),
    at t = 0 and at t = T - 1 (duplicates dropped), then the two dense ones"""
    T, n = gJ.shape
    a = np.abs(gJ)
    coords = [np.unravel_index(int(np.argmax(a)), a.shape), (int(np.argmax(a[:, n - 1])), n - 1),
              (0, int(np.argmax(a[0]))), (T - 1, int(np.argmax(a[T - 1])))]
    dirs = []
    for c in sorted(set((int(t), int(i)) for t, i in coords)):
        v = np.zeros((T, n))
        v[c] = 1.0
        dirs.append(v)
    return np.stack(dirs + list(dense))


def direction_distance(gJ, dirs, truth, scale):
    """worst over the directions of |<gJ, v> - truth_v| / (scale |v|_1): a coordinate direction gives |a_k - truth_k| /
    scale, a dense one a lower bound of the normwise distance (tests/test_lds_truth_hip.py's fused_vjp_case)"""
    gJ = np.asarray(gJ, float)
    return max(abs(float(np.sum(gJ * v)) - float(t)) / (scale * float(np.abs(v).sum())) for v, t in zip(dirs, truth))
