"""Inputs, truths and error measures shared by tests/test_gmm_mp_cpu.py and tests/test_gmm_truth_hip.py (test
infrastructure): the GMM local step -- mean-field fixed point, sampler, derived adjoint -- away from the one family the
older tests use (Psi = (N + 10) I, means ~ 2, uniform-random label_init).

gaussian_globals are written down in closed form from (Lambda_k, m_k, kappa_k, nu_k) -- the expected statistics of a
NIW whose scale matrix is Lambda_k^-1, WITHOUT niw_expectedstats' absolute 1e-8 on the diagonal, which is not scale-free:

    A = -1/2 nu Lambda,  b = nu Lambda m,  c = -1/2 (nu m' Lambda m + N / kappa),  d = 1/2 E log|J|

Node potentials are (-1/2 prec, prec x) with x drawn around the component means.  A family is a one-line change of that
picture (FAMILIES below); `case(family, N, K, T)` is deterministic in its arguments.

Measures: per output array the normwise error max|a - truth| / max|truth| (the dense-packed arrays split into their
E[x x'] / -1/2 J block and their E[x] / h column: the packing's constant 1 entries would otherwise set the scale); `kl` on
the scale sum|terms| the oracle returns.  The rule, per output, is tests/_global_step_families.py's:

    e_kernel <= FACTOR max(e_ref, FLOOR),   FACTOR = 16, FLOOR = 64 eps

with e_ref the error of oracle/gmm_numpy.py on the same input and sweep count under the same measure."""
import functools
import os

import numpy as np
from scipy.special import digamma

from oracle import expfam_numpy as ef, gmm_mp, gmm_numpy

FACTOR = 16.0
FLOOR = 64 * np.finfo(float).eps
TOL = 1e-3                         # the stopping cases' tolerance (the library's default)

# name -> what it stresses
FAMILIES = {
    "plain": "today's regime: anchors the rule's floor",
    "far": "means 40 sigma apart: responsibilities underflow to exact 0, exp arguments below -746",
    "offset-1e4": "every mean and point shifted by 1e4 sigma: the natural parametrisation cancels (e_ref ~ 4e-9)",
    "tie": "components in identical pairs, uniform label_init: responsibilities tie exactly",
    "tie-all": "all components identical, uniform label_init: the KL is the same bits every sweep",
    "empty": "one component 60 sigma from every point: its responsibility column is 0 or denormal",
    "K1": "K = 1: softmax trivially 1, label KL 0",
    "sharp-node": "node precision 1e8 x the component's: the point is pinned by its own potential",
    "flat-node": "node precision 1e-8 x the component's: the node potential is ignored",
    "aniso": "Lambda_k of condition 1e8 in a random rotation: LDL' without pivoting, the reciprocal's Newton steps",
}
# scale-<s>: every length multiplied by s


def _rotation(N, rng):
    Q, R = np.linalg.qr(rng.standard_normal((N, N)))
    return Q * np.sign(np.diag(R))


def _seed(family, N, K, T, salt=0):
    return [sum(ord(c) * (i + 1) for i, c in enumerate(family)), N, K, T, salt]


def globals_closed_form(Lam, m, kappa, nu):
    """(Lambda (K,N,N), m (K,N), kappa (K), nu (K)) -> gaussian_globals (K, N+2, N+2)"""
    K, N = m.shape
    Lm = np.einsum("kij,kj->ki", Lam, m)
    A = -0.5 * nu[:, None, None] * Lam
    b = nu[:, None] * Lm
    c = -0.5 * (nu * np.einsum("ki,ki->k", m, Lm) + N / kappa)
    d = 0.5 * (digamma((nu[:, None] - np.arange(N)[None, :]) / 2.).sum(-1) + N * np.log(2.) + np.linalg.slogdet(Lam)[1])
    return ef.pack_dense((A + np.swapaxes(A, -1, -2)) / 2, b, c, d)


def case(family, N, K, T, salt=0):
    """-> dict(label_global (K), gaussian_globals (K,N+2,N+2), node_J (T,N), node_h (T,N), label_init (T,K),
    max_iters): deterministic in (family, N, K, T, salt)"""
    if family == "K1":
        K = 1
    rng = np.random.default_rng(_seed(family, N, K, T, salt))
    s = float(family[6:]) if family.startswith("scale-") else 1.0
    nu = N + 3.0 + 4.0 * rng.random(K)
    kappa = 1.0 + 4.0 * rng.random(K)
    m = 2.0 * rng.standard_normal((K, N))
    lam = np.exp(0.5 * rng.standard_normal((K, N)))                     # eigenvalues of Lambda_k, O(1)
    if family == "aniso":
        lam = np.stack([np.logspace(0, 8, N) if N > 1 else np.ones(1)] * K) * (1.0 + rng.random((K, 1)))
    rot = np.stack([_rotation(N, rng) for _ in range(K)])
    if family == "aniso":                        # one rotation, means a few sigma apart along every axis: soft labels
        rot = np.stack([rot[0]] * K)
        m = np.einsum("kia,ka->ki", rot, 1.5 * rng.standard_normal((K, N)) / np.sqrt(lam * nu[:, None]))
    if family == "far":
        m = 0.3 * rng.standard_normal((K, N))
        m[:, 0] += 40.0 * np.arange(K) / np.sqrt(lam.min())
    if family == "offset-1e4":
        lam, rot = np.ones((K, N)), np.stack([np.eye(N)] * K)           # unit covariances
    if family in ("tie", "tie-all"):
        twin = (np.arange(K) // 2) * 2 if family == "tie" else np.zeros(K, int)
        nu, kappa, m, lam, rot = nu[twin], kappa[twin], m[twin], lam[twin], rot[twin]
    if family == "empty" and K > 1:
        m[K // 2] = 0.0
        m[K // 2, 0] = 60.0 / np.sqrt(lam.min()) + 3.0 * np.abs(m).max()
    Lam = np.einsum("kia,ka,kja->kij", rot, lam, rot)
    alpha = 0.5 + 2.0 * rng.random(K)
    if family in ("tie", "tie-all"):
        alpha = alpha[twin]
    label_global = digamma(alpha) - digamma(alpha.sum())
    # points around the means of the components that own them (never the empty one)
    owners = np.array([k for k in range(K) if not (family == "empty" and K > 1 and k == K // 2)])
    z = owners[rng.integers(0, len(owners), T)]
    x = m[z] + np.einsum("tia,ta->ti", rot[z], rng.standard_normal((T, N)) / np.sqrt(lam[z] * nu[z, None]))
    node_factor = {"sharp-node": 1e8, "flat-node": 1e-8}.get(family, 1.0)
    prec = node_factor * nu[z, None] * np.exp(0.5 * rng.standard_normal((T, N))) * np.exp(np.log(lam[z]).mean(-1))[:, None]
    if family == "offset-1e4":
        m, x = m + 1e4, x + 1e4
    # all lengths x s
    Lam, m, x, prec = Lam / s ** 2, m * s, x * s, prec / s ** 2
    gg = globals_closed_form(Lam, m, kappa, nu)
    if family in ("tie", "tie-all"):
        gg, label_global = gg[twin], label_global[twin]                 # identical BITS, whatever the rounding above did
    init = rng.random((T, K)) + 0.05
    init = init / init.sum(-1, keepdims=True)
    if family in ("tie", "tie-all"):
        init = np.full((T, K), 1.0 / K)
    return dict(label_global=label_global, gaussian_globals=gg, node_J=-0.5 * prec, node_h=prec * x, label_init=init,
                max_iters=(0, 1, 3))


# --- the case lists (the table at the top of tests/test_gmm_truth_hip.py is written from these) -----------------------
# Workgroup boundaries, read from the sources: the persistent kernel and the per-sweep launches have 256 points per
# workgroup (GMM_MW_BLOCK), the one-workgroup kernel 1024 / 512 / 256 threads for N <= 3 / <= 5 / <= 8 (gmm_block<N>()),
# the wide kernels 16 points per workgroup (WBLOCK / 16).  A wavefront holds 64 points (N <= 8) or 4 (wide).
# (family, N, K, T, sweeps)
PLAIN = [
    ("plain", 1, 5, 63, 0), ("plain", 1, 5, 63, 1), ("plain", 1, 5, 63, 3),
    ("plain", 1, 2, 1025, 1),                                   # one point over the one-workgroup kernel's 1024 lanes
    ("plain", 2, 5, 257, 1), ("plain", 2, 8, 64, 3), ("plain", 2, 9, 65, 1), ("plain", 2, 64, 17, 1),
    ("plain", 3, 16, 255, 1), ("plain", 3, 17, 256, 0),
    ("plain", 4, 16, 65, 3), ("plain", 4, 3, 513, 1),           # (512 lanes at N = 4)
    ("plain", 5, 5, 64, 1), ("plain", 5, 9, 1, 3),
    ("plain", 8, 9, 257, 1), ("plain", 8, 3, 1, 3),
    ("plain", 9, 5, 15, 3), ("plain", 12, 17, 16, 1),
    ("plain", 16, 5, 17, 0), ("plain", 16, 5, 17, 1), ("plain", 16, 5, 17, 3), ("plain", 16, 64, 5, 1),
]
_FOUR = [(2, 5, 65, 0), (2, 5, 65, 3), (4, 16, 33, 1), (8, 5, 17, 3), (16, 9, 17, 1)]
OTHERS = [(f, N, K, T, m) for f in ("far", "offset-1e4", "tie", "empty", "K1", "sharp-node", "flat-node", "aniso")
          for (N, K, T, m) in _FOUR]
SCALES = [("scale-%s" % s, N, 3, 17, 1) for s in ("1e-3", "1e3") for N in (1, 2, 3, 4, 5, 8, 9, 12, 16)]
# the scales at which prod_j d_j leaves the fp64 range while every pivot is an ordinary number (pivot ~ 30 / s^2):
# pivots of 3e+43 / 3e-41 at N = 8, of 3e+23 / 3e-21 at N = 16 (tests/test_gmm_mp_cpu.py asserts both halves)
OVERFLOW = [("scale-%s" % s, N, 5, 17, m) for N, ss in ((8, ("1e-21", "1e21")), (16, ("1e-11", "1e11"))) for s in ss
            for m in (1, 3)]
ACCURACY = PLAIN + OTHERS + SCALES + OVERFLOW

# stopping decision at tol = 1e-3, max_iter = 100: (family, N, K, T, salt) -- the salts are chosen so that every case is
# admissible (tests/test_gmm_mp_cpu.py asserts it; nothing is skipped at run time)
# (offset-1e4: the restatement's KL is off by ~ 3e-7 T N there, absolutely, so only a handful of points can clear
#  1e3 a < tol at all; salts 5 and 11 are the widest of 40: margin 5.0 x and 3.2 x the condition)
STOPPING = [("plain", 2, 5, 65, 0), ("plain", 9, 5, 17, 0), ("far", 2, 5, 65, 0), ("far", 8, 3, 17, 0),
            ("offset-1e4", 1, 5, 3, 5), ("offset-1e4", 9, 3, 1, 11)]
TIE_STOP = [("tie-all", 2, 4, 65, 0), ("tie-all", 9, 5, 17, 0)]

TAIL_FAMILIES = ("plain", "offset-1e4", "aniso", "sharp-node", "scale-1e-3", "scale-1e3")
TAIL = [(f, N, 5, 65, S) for f in TAIL_FAMILIES for N in (1, 4, 8, 9, 16) for S in (1, 3)]


def routes(N):
    """{route name: (keyword arguments of meanfield_from_globals, the out["path"] it must report)}"""
    if N > 8:
        return {"wide_sweeps": (dict(), "wide_sweeps")}
    return {"single_wg": (dict(multi_wg=False), "single_wg"), "persistent": (dict(), "persistent"),
            "sweeps": (dict(multi_wg=True, persistent=False), "sweeps"), "wide": (dict(wide=True), "wide_sweeps")}


# --- measures --------------------------------------------------------------------------------------------------------

def e_block(got, truth):
    got, truth = np.asarray(got, float), np.asarray(truth, float)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - truth)) / np.max(np.abs(truth)))


def errors(out, truth):
    """{output: error} of one evaluation (a dict with local_meanfield_mp's keys, float64) against the oracle's"""
    N = truth["gaussian_stats"].shape[-1] - 2
    e = {"label_stats": e_block(out["label_stats"], truth["label_stats"]),
         "label_fixed": e_block(out["label_fixed"], truth["label_fixed"]),
         "label_natparam": e_block(out["label_natparam"], truth["label_natparam"]),
         "dirichlet_stats": e_block(out["dirichlet_stats"], truth["dirichlet_stats"])}
    for name, a, b in (("gaussian_stats", "ExxT", "Ex"), ("gaussian_natparam", "J", "h"), ("niw_stats", "ExxT", "Ex")):
        g, t = np.asarray(out[name], float), truth[name]
        e["%s.%s" % (name, a)] = e_block(g[..., :N, :N], t[..., :N, :N])
        e["%s.%s" % (name, b)] = e_block(g[..., :N, N], t[..., :N, N])
    for name in ("gaussian_natparam", "niw_stats"):            # the two trailing diagonal entries (c, d / the counts)
        g, t = np.asarray(out[name], float), truth[name]
        e["%s.cd" % name] = e_block(np.stack([g[..., N, N], g[..., N + 1, N + 1]]),
                                    np.stack([t[..., N, N], t[..., N + 1, N + 1]]))
    kl = float(np.asarray(out["kl"]).reshape(-1)[0])
    e["kl"] = abs(kl - truth["kl"]) / truth["kl_scale"] if np.isfinite(kl) else float("inf")
    return e


def reference(c, tol, max_iter):
    """oracle/gmm_numpy.py on a case -> a dict with the oracle's keys"""
    trace = {}
    (ls, gs), (ds, ns), (ln, gn), kl, iters = gmm_numpy.local_meanfield(
        c["label_global"], c["gaussian_globals"], (c["node_J"], c["node_h"]), c["label_init"], tol, max_iter, trace=trace)
    return dict(label_stats=ls, label_fixed=trace["label_fixed"], label_natparam=ln, gaussian_stats=gs,
                gaussian_natparam=gn, dirichlet_stats=ds, niw_stats=ns, kl=float(kl), iters=iters,
                kl_hist=trace["kl_hist"])


@functools.lru_cache(maxsize=None)
def truth(family, N, K, T, max_iter, tol=0.0, salt=0):
    """-> (case, oracle dict, reference dict, e_ref); computed once per process and shared, never modified"""
    c = case(family, N, K, T, salt)
    tr = gmm_mp.local_meanfield_mp(c["label_global"], c["gaussian_globals"], (c["node_J"], c["node_h"]), c["label_init"],
                                   tol, max_iter)
    ref = reference(c, tol, max_iter)
    return c, tr, ref, errors(ref, tr)


def expected_assign(tr, e_ref):
    """-> (argmax of the oracle's responsibilities, first maximum; mask of the points held to it): a point is exempt when
    its top two responsibilities are closer than 1e3 e_ref(label_stats) -- but not when they are EQUAL (the tie families:
    the lowest index is then required)"""
    ls = tr["label_stats"]
    want = np.argmax(ls, -1)
    if ls.shape[1] == 1:
        return want, np.ones(len(ls), bool)
    top = np.sort(ls, -1)
    gap = top[:, -1] - top[:, -2]
    return want, (gap > 1e3 * max(e_ref["label_stats"], FLOOR)) | (gap == 0.0)


def admissible(tr, ref, tol=TOL):
    """the stopping case's condition: every |d_i - tol| up to and including the first d_i < tol exceeds 1e3 x the largest
    absolute error of the restatement's kl_hist.  -> (bool, margin min|d_i - tol|, that error a)"""
    h, hr = tr["kl_hist"], ref["kl_hist"]
    n = min(len(h), len(hr))
    a = float(np.max(np.abs(h[:n] - hr[:n])))
    d = np.abs(np.diff(h))                              # (d_0 = |kl_0 - inf| never stops)
    margin = float(np.min(np.abs(d - tol))) if len(d) else float("inf")
    return len(h) == len(hr) and margin > 1e3 * a, margin, a


def check(errs, e_ref, what, exceptions=None):
    """print every figure (`GMMTRUTH` lines), then require e <= FACTOR max(e_ref, FLOOR) per output; a named exception
    (what, output) -> its own pinned bound instead.  -> the failures as text lines"""
    bad = []
    for q in sorted(errs):
        yard = max(e_ref[q], FLOOR)
        print("GMMTRUTH %-56s %-22s e %.3e  e_ref %.3e  ratio %8.2f" % (what, q, errs[q], e_ref[q], errs[q] / yard))
        bound = FACTOR * yard
        if exceptions and (what, q) in exceptions:
            bound = exceptions[(what, q)]
        if not np.isfinite(e_ref[q]):
            bad.append("%s %s: e_ref is not finite (not a valid comparison)" % (what, q))
        if not errs[q] <= bound:
            bad.append("%s %s: e %.3e > bound %.3e (e_ref %.3e)" % (what, q, errs[q], bound, e_ref[q]))
    return bad


# --- the taped tail: sampler and adjoint -----------------------------------------------------------------------------
# One problem per (family, N) at K = 5, T = 65 with S = 3 noise draws (S = 1 takes the first); the responsibilities that
# enter the pass are the restatement's after one sweep, rounded to float64: an INPUT from here on, the same bits for the
# kernel, torch and the oracle.
MODES = ("kl", "samples", "both")
TAIL_K, TAIL_T, TAIL_S = 5, 65, 3


GOLDEN_TAIL_N = 16         # the oracle's derivatives along the random directions take 10 s per family there: stored
_TAIL_INPUTS = ("label_global", "gaussian_globals", "node_J", "node_h", "label_init", "label_fixed", "natparam", "eps",
                "g_samples", "g_kl", "dir0_J", "dir0_h", "dir1_J", "dir1_h")


def golden_tail_path(family, N):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_truth_tail_%s_N%d.npz" % (family, N))


def make_tail_case(family, N):
    c = dict(case(family, N, TAIL_K, TAIL_T))
    ref = reference(c, 0.0, 1)
    rng = np.random.default_rng(_seed(family, N, TAIL_K, TAIL_T, 99))
    c.update(label_fixed=np.ascontiguousarray(ref["label_fixed"]), natparam=np.ascontiguousarray(ref["gaussian_natparam"]),
             eps=rng.standard_normal((TAIL_T, TAIL_S, N)), g_samples=rng.standard_normal((TAIL_T, TAIL_S, N)),
             g_kl=float(rng.standard_normal()),
             dirs=[(rng.standard_normal((TAIL_T, N)), rng.standard_normal((TAIL_T, N))) for _ in range(2)])
    return c


@functools.lru_cache(maxsize=None)
def tail_case(family, N):
    """N = 16: inputs AND truth from tests/golden/gmm_truth_tail_<family>_N16.npz (make_golden_gmm_truth.py), so that the
    stored truth belongs to the inputs bit for bit; otherwise generated"""
    if N != GOLDEN_TAIL_N:
        return make_tail_case(family, N)
    g = np.load(golden_tail_path(family, N))
    c = {k: g[k] for k in _TAIL_INPUTS[:-4]}
    c.update(g_kl=float(g["g_kl"]), dirs=[(g["dir0_J"], g["dir0_h"]), (g["dir1_J"], g["dir1_h"])], max_iters=(0, 1, 3))
    return c


def _t64(x):
    import torch
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64)


def tail_torch(c, S, nJ, nh):
    """tests/_gmm_torch.py on the CPU -> (samples (T, S, N), local_kl), on the autograd tape of nJ, nh"""
    from _gmm_torch import final_pass_torch, sample_torch
    from svae_amd.distributions import expfam
    _, (_, natp), kl = final_pass_torch(_t64(c["label_global"]), _t64(c["gaussian_globals"]), expfam.pack_dense(nJ, nh),
                                        _t64(c["label_fixed"]))
    return sample_torch(natp, _t64(c["eps"][:, :S])), kl


def cotangent(c, S, mode):
    """-> (g_samples (T, S, N), g_kl) with zeros where the mode has none"""
    return (c["g_samples"][:, :S] * (mode != "kl"), c["g_kl"] * (mode != "samples"))


@functools.lru_cache(maxsize=None)
def tail_want(family, N, S, mode):
    """torch-CPU autograd of the tail: the e_ref of the gradients -> (g_node_J, g_node_h)"""
    import torch
    c = tail_case(family, N)
    nJ, nh = _t64(c["node_J"]).requires_grad_(True), _t64(c["node_h"]).requires_grad_(True)
    x, kl = tail_torch(c, S, nJ, nh)
    gs, gk = cotangent(c, S, mode)
    gJ, gh = torch.autograd.grad((_t64(gs) * x).sum() + gk * kl, [nJ, nh])
    return gJ.numpy(), gh.numpy()


def make_tail_truth(c):
    from _gmm_torch import sample_torch
    args = (c["label_global"], c["gaussian_globals"], (c["node_J"], c["node_h"]), c["label_fixed"], c["eps"])
    return dict(samples=gmm_mp.sample_mp(c["natparam"], c["eps"]),
                samples_ref=sample_torch(_t64(c["natparam"]), _t64(c["eps"])).numpy(),
                jvp=[gmm_mp.local_tail_jvp_mp(*args, direction=d) for d in c["dirs"]])


@functools.lru_cache(maxsize=None)
def tail_truth(family, N):
    """-> dict(samples: sample_mp of the case's natural parameters (T, 3, N); samples_ref: _gmm_torch.sample_torch's on the
    CPU; jvp: [(d samples, d kl)] along the case's two random directions)"""
    if N != GOLDEN_TAIL_N:
        return make_tail_truth(tail_case(family, N))
    g = np.load(golden_tail_path(family, N))
    return dict(samples=g["samples"], samples_ref=g["samples_ref"],
                jvp=[(g["jvp0_samples"], float(g["jvp0_kl"])), (g["jvp1_samples"], float(g["jvp1_kl"]))])


@functools.lru_cache(maxsize=None)
def _point_jvp(family, N, t, which, i):
    """d (samples_t, kl) / d node_{J or h}[t, i]: a point's potentials reach only that point's samples and KL term"""
    c = tail_case(family, N)
    N = c["node_h"].shape[1]
    d = [np.zeros((1, N)), np.zeros((1, N))]
    d[which][0, i] = 1.0
    return gmm_mp.local_tail_jvp_mp(c["label_global"], c["gaussian_globals"], (c["node_J"][t:t + 1], c["node_h"][t:t + 1]),
                                    c["label_fixed"][t:t + 1], c["eps"][t:t + 1], direction=tuple(d))


def grad_errors(family, N, S, mode, got):
    """(e_got, e_ref) of gradient arrays (g_node_J, g_node_h) through <VJP(g), v> = <g, J v>, J v from the oracle
    (tests/test_lds_truth_hip.py::_grad_truth's scheme).  Directions: the two coordinates where `got` and torch-CPU autograd
    disagree most (relative to their array's scale), the largest coordinate, and two random directions over both arrays.
    A coordinate gives |a_k - truth_k| / max|array|; a random direction a lower bound of the normwise distance."""
    c = tail_case(family, N)
    want = tail_want(family, N, S, mode)
    got = [np.asarray(a, float) for a in got]
    gs, gk = cotangent(c, S, mode)
    scale = [max(float(np.max(np.abs(w))), 1e-300) for w in want]
    if not all(np.all(np.isfinite(a)) for a in got):
        return float("inf"), 0.0
    cand = sorted(((abs(got[a][idx] - want[a][idx]) / scale[a], a) + idx for a in range(2) for idx in np.ndindex(want[a].shape)),
                  reverse=True)[:2]
    big = max(((abs(want[a][idx]) / scale[a], a) + idx for a in range(2) for idx in np.ndindex(want[a].shape)))
    e_got = e_ref = 0.0
    for _, a, t, i in cand + [big]:
        ds, dkl = _point_jvp(family, N, int(t), int(a), int(i))
        truth = float(np.sum(gs[t] * ds[0, :S])) + gk * dkl
        e_got = max(e_got, abs(got[a][t, i] - truth) / scale[a])
        e_ref = max(e_ref, abs(want[a][t, i] - truth) / scale[a])
    for d, (ds, dkl) in zip(c["dirs"], tail_truth(family, N)["jvp"]):
        truth = float(np.sum(gs * ds[:, :S])) + gk * dkl
        norm = sum(sc * float(np.abs(v).sum()) for sc, v in zip(scale, d))
        dot = lambda G: sum(float(np.sum(g * v)) for g, v in zip(G, d))
        e_got, e_ref = max(e_got, abs(dot(got) - truth) / norm), max(e_ref, abs(dot(want) - truth) / norm)
    return e_got, e_ref
