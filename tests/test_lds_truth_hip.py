"""The LDS kernels against the TRUTH: oracle/lds_mp.py evaluates the same operation in 50-60 digits, so on an
ill-conditioned model it says which of the HIP kernel and the reference's compiled function carries the error.

Metric: normwise, max|a - truth| / max|truth| per output array.  A path meant to be accurate to cond * eps must meet
    HIP-vs-truth <= max(3 x reference-vs-truth, 1e-11)
with the reference's compiled function of the same name evaluated here on the same input (`_cond_eps_rule`).  Paths known
to be cond^2 * eps on ill-conditioned draws (the lean [P^-1 | c] records of the two-ended smoothers) are
pinned at about 3x their measured distance (LEAN_PINS); so are, per output array, the few cond * eps outputs on which
the HIP kernel is still more than 3x further from the truth than the reference (GAP_PINS: open).
Every model is handed over with exactly symmetric J0, J11, J22 (_symmetric_model).  Gradients are checked through
<VJP(g), v> = <g, J v>: J v by
oracle.lds_mp.jvp_mp (a central difference inside mp) at the coordinates where the fp64 sides disagree most and along a
random direction; the node-h gradient of the E-step has a closed form (one more solve).  The gradients w.r.t. the init and
pair natural parameters (natparam_grad=True) have no compiled reference: their comparator is the fp64 CPU autograd of
tests/_lds_large_torch.torch_estep (test_param_gradients_against_truth)."""
import functools

import numpy as np
import pytest
import torch

from oracle import lds_mp, lds_numpy, ref

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

# the conditioning ladder: (n, T, seed) of rand_lds_natparam + rand_node_potentials((1, T, n)); cond(J22) by np.linalg.cond
DRAWS = {"n7_s0": (7, 45, 0),         # 1.2e3
         "n7_s1": (7, 45, 1),         # 2.6e5
         "n7_s262": (7, 45, 262),     # 7.8e7
         "n8_s116": (8, 45, 116),     # 2.2e9
         "n10_s25": (10, 200, 25)}    # 2.3e7, the worst of seeds 0..299 at n = 10
TILE_DRAWS = {"n16_s207": (16, 10, 207),    # 3.9e6, the worst of seeds 0..299 at n = 16
              "n24_s219": (24, 10, 219)}    # 3.3e8, the worst of seeds 0..299 at n = 24
VARIANTS = ("twoend", "twoend_full", "twoend_seq", "twoend_rpc", "split", "packed")
FLOOR = 1e-11

# Pins: measured HIP-vs-truth on MI355X x 3, rounded up.  Case keys: ("estep", draw, variant) -- B-independent: the
# replicated draw at B = 513 / 1100 measures as B = 1 --, ("inference", B, accurate), ("tile", draw), ("host", entry),
# ("vjp", draw, accurate, sampler), ("prim", kind, n, form), ("prim262", kind), ("pgrad", draw, layout).
# cond^2 * eps BY DESIGN (the lean [P^-1 | c] records), worst output array of the case: the
# two-ended lean E-step variants from cond(J22) 2.6e5 on, the training forward below 1025 sequences, the default-mode VJP.
LEAN_PINS = {
    ("estep", "n7_s1", "twoend"): 2.3e-9, ("estep", "n7_s1", "twoend_seq"): 2.3e-9, ("estep", "n7_s1", "twoend_rpc"): 2.3e-9,
    ("estep", "n7_s262", "twoend"): 4e-4, ("estep", "n7_s262", "twoend_seq"): 4e-4, ("estep", "n7_s262", "twoend_rpc"): 4e-4,
    ("estep", "n8_s116", "twoend"): 0.085, ("estep", "n8_s116", "twoend_seq"): 0.085,
    ("estep", "n8_s116", "twoend_rpc"): 0.085,
    ("estep", "n10_s25", "twoend"): 3e-5, ("estep", "n10_s25", "twoend_seq"): 3e-5, ("estep", "n10_s25", "twoend_rpc"): 3e-5,
    ("inference", 1, False): 4e-4, ("inference", 513, False): 4e-4,
    ("vjp", "n7_s262", False, False): 3.4e-4, ("vjp", "n7_s262", False, True): 3.4e-4,
    ("vjp", "n8_s116", False, False): 0.07, ("vjp", "n8_s116", False, True): 0.07,
}
# Output arrays of cond * eps paths that miss `<= max(3 x reference, 1e-11)`, pinned per array (every other array of the
# case still meets the rule).  Open gaps, all but the ("pgrad", ..) ones within 3e-10 of the truth: the lognorm of the accurate E-step at
# cond(J22) = 2.2e9 (4.7x the reference's 3.8e-11), E_pair xx / xnxn at n = 10, T = 200 (3.5-6x the reference's 1.4e-11),
# the n = 16 tile E-step (E[x] 4.9e-11 against 2.0e-12 .. 9.3e-12), two sampler-VJP cases at 1.1e-11 / 1.3e-11 (the
# reference 1.5e-12 / 2.0e-12).  DESIGN sections 2 and 4.2b.
GAP_PINS = {
    ("estep", "n8_s116", "twoend_full"): {"lognorm": 5.5e-10},
    ("estep", "n8_s116", "split"): {"lognorm": 4.3e-10},
    ("estep", "n8_s116", "packed"): {"lognorm": 4.3e-10},
    ("estep", "n10_s25", "twoend_full"): {"lognorm": 6e-11, "Epair_xx": 2.6e-10, "Epair_xxn": 5.1e-10, "Epair_xnxn": 2.6e-10},
    ("estep", "n10_s25", "split"): {"Epair_xx": 1.5e-10, "Epair_xnxn": 1.5e-10},
    ("estep", "n10_s25", "packed"): {"Epair_xx": 1.5e-10, "Epair_xnxn": 1.5e-10},
    ("tile", "n16_s207"): {"ExxT0": 1.4e-10, "Ex0": 1.5e-10, "Epair_xxn": 2e-10, "Enode_x": 1.5e-10, "sample0": 1.5e-10},
    ("prim", "sampler", 10, "inhomog"): {"grad": 3.3e-11},
    ("prim", "sampler", 15, "batched"): {"grad": 3.9e-11},
    # The parameter gradients (natparam_grad=True; key ("pgrad", draw, layout)) run on the FULL per-step records in either
    # mode -- a plan made for them has the [chol(P)^-T | c] records of set_accurate_smoother switched off, and only the packed
    # sweep 2 on full records writes their blocks -- so from cond(J22) 2.6e5 on they are where the default-mode node gradients
    # are (LEAN_PINS ("vjp", ..)): cond^2 * eps.  Open; the comparator (fp64 CPU autograd) is at 2e-13 .. 3e-13 on n7_s1,
    # 8e-11 .. 9e-10 on n7_s262, 1e-9 .. 6e-9 on n8_s116 ("Parameter gradients: routes, edges, truth").
    ("pgrad", "n7_s1", "homog"): {"J11": 2.2e-10, "J12": 6.9e-10, "J22": 2.2e-10},
    ("pgrad", "n7_s262", "homog"): {"init_J": 5.5e-4, "init_h": 1.2e-4, "J11": 4e-4, "J12": 4e-4, "J22": 3.7e-4,
                                    "random": 2.3e-5},
    ("pgrad", "n8_s116", "homog"): {"init_J": 0.07, "init_h": 0.044, "J11": 0.073, "J12": 0.096, "J22": 0.07,
                                    "random": 2.2e-3},
    ("pgrad", "n7_s262", "homog_zero_noise"): {"init_J": 3.7e-4, "init_h": 9.2e-5, "J11": 3.3e-4, "J12": 3.7e-4,
                                               "J22": 3.1e-4, "random": 2e-5},
}


def _sym_blocks(x):
    """(M + M') / 2 over the last two axes: exactly symmetric in fp64"""
    x = np.asarray(x, float)
    return (x + np.swapaxes(x, -1, -2)) / 2


def _symmetric_model(init, pair):
    """J0, J11, J22 made exactly symmetric.  rand_lds_natparam's blocks are symmetric only to ~7e-16 (products and inverses
    in fp64); the reference's Cholesky reads their lower triangle, and so does the oracle's, while a kernel is free to read the other.
    At cond(J22) = 7.8e7 the two triangles define models whose E[x] differ by 1.8e-9 -- the size of the distances measured
    here -- so the arbitration hands every side the same, exactly symmetric, model."""
    return ((_sym_blocks(init[0]),) + tuple(init[1:]),
            (_sym_blocks(pair[0]), np.asarray(pair[1], float), _sym_blocks(pair[2])) + tuple(pair[3:]))


def _draw(n, T, seed):
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    rng = np.random.default_rng(seed)
    init, pair = _symmetric_model(*rand_lds_natparam(n, rng))
    node = rand_node_potentials((1, T, n), rng, with_logZ=True)
    return init, pair, node


@functools.lru_cache(maxsize=None)
def _truth_estep(key):
    init, pair, node = _draw(*(DRAWS.get(key) or TILE_DRAWS[key]))
    return lds_mp.estep_mp((init, pair), tuple(x[0] for x in node))


@functools.lru_cache(maxsize=None)
def _ref_estep(key):
    init, pair, node = _draw(*(DRAWS.get(key) or TILE_DRAWS[key]))
    return ref.estep((init, pair), tuple(x[0] for x in node))


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, float)


def _dist(a, truth):
    """normwise distance; `a` may carry a leading batch axis (worst sequence)"""
    a, t = _np(a), np.asarray(truth, float)
    scale = max(float(np.max(np.abs(t))), 1e-300) if t.size else 1.0
    if t.ndim == 0:
        scale = max(abs(float(t)), 1.0)
    return float(np.max(np.abs(a - t)) / scale) if t.size else 0.0


def _stats_arrays(lognorm, stats):
    (Ei, Ep, En) = stats
    return {"lognorm": lognorm, "ExxT0": Ei[0], "Ex0": Ei[1], "Epair_xx": Ep[0], "Epair_xxn": Ep[1],
            "Epair_xnxn": Ep[2], "Enode_diagxx": En[0], "Enode_x": En[1]}


def _distances(got, truth):
    return {k: _dist(got[k], truth[k]) for k in truth}


def _cond_eps_rule(hip, want, what):
    """HIP-vs-truth <= max(3 x reference-vs-truth, 1e-11), per output array"""
    for k in hip:
        assert hip[k] <= max(3 * want[k], FLOOR), (what, k, hip[k], want[k])


def _judge(key, hip, want):
    """a lean case stays within its pin; otherwise every output array meets the cond * eps rule or, if it is listed in
    GAP_PINS, its pin"""
    if key in LEAN_PINS:
        worst = max(hip.values())
        assert worst <= LEAN_PINS[key], (key, worst, LEAN_PINS[key])
        return
    gaps = GAP_PINS.get(key, {})
    for k in hip:
        if k in gaps:
            assert hip[k] <= gaps[k], (key, k, hip[k], gaps[k])
        else:
            _cond_eps_rule({k: hip[k]}, {k: want[k]}, key)


def _dev_model(init, pair, node, B=1):
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda")
    nodes = tuple(t(np.repeat(x, B, axis=0)) for x in node)
    return (tuple(t(x) for x in init), tuple(t(x) for x in pair)), nodes


def _hip_estep(key, variant, B=1):
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    n, T, seed = DRAWS.get(key) or TILE_DRAWS[key]
    init, pair, node = _draw(n, T, seed)
    nat, nodes = _dev_model(init, pair, node, B)
    plan = LDSEStepPlan(B, T, n, "cuda", options=_lib.KERNEL_OPTIONS[variant])
    with torch.no_grad():
        lognorm, stats = natural_lds_estep_general(nat, nodes, plan=plan, check=True)
        return _stats_arrays(lognorm, stats)


def estep_case(key, variant, B=1):
    """(HIP-vs-truth, reference-vs-truth) per output array of the E-step through `variant`'s options word"""
    ln, st = _truth_estep(key)
    truth = _stats_arrays(ln, st)
    return _distances(_hip_estep(key, variant, B), truth), _distances(_stats_arrays(*_ref_estep(key)), truth)


@needs_ref
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("key", list(DRAWS))
def test_estep_all_outputs_against_truth(key, variant):
    hip, want = estep_case(key, variant)
    _judge(("estep", key, variant), hip, want)


@needs_ref
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B", [1, 513, 1100])
def test_estep_replicated_ill_draw_against_truth(B, variant):
    """seed 262 replicated to B sequences: above 512 the two-ended kernels run two sequences per wavefront"""
    hip, want = estep_case("n7_s262", variant, B)
    _judge(("estep", "n7_s262", variant), hip, want)


def inference_case(key, accurate, B=1):
    """E[x], diag E[xx'] and lognorm of lds_inference_differentiable (the training forward: svae_lds_inference_f64 on
    full, lean or [chol(P)^-T | c] records by batch size and mode) with zero noise; the sample is E[x] too"""
    from svae_amd.lds import lds_inference as li
    n, T, seed = DRAWS[key]
    init, pair, node = _draw(n, T, seed)
    nat, nodes = _dev_model(init, pair, node, B)
    old = li.set_accurate_smoother(accurate)
    try:
        with torch.no_grad():
            ln, (dxx, x), smp, _ = li.lds_inference_differentiable(
                nat, nodes, eps=torch.zeros((B, T, 1, n), dtype=torch.float64, device="cuda"))
    finally:
        li.set_default_options(old)
    tl, (_, _, tn) = _truth_estep(key)
    rl, (_, _, rn) = _ref_estep(key)
    truth = {"lognorm": tl, "Enode_diagxx": tn[0], "Enode_x": tn[1], "sample0": tn[1]}
    hip = _distances({"lognorm": ln, "Enode_diagxx": dxx, "Enode_x": x, "sample0": smp[:, :, 0]}, truth)
    want = _distances({"lognorm": rl, "Enode_diagxx": rn[0], "Enode_x": rn[1], "sample0": rn[1]}, truth)
    return hip, want


@needs_ref
@pytest.mark.parametrize("accurate", [True, False])
@pytest.mark.parametrize("B", [1, 513, 1100])
def test_inference_forward_replicated_ill_draw_against_truth(B, accurate):
    """the training forward on seed 262 at B = 1, 513, 1100 (past 1024 the default is the [chol(P)^-T | c] records)"""
    hip, want = inference_case("n7_s262", accurate, B)
    _judge(("inference", B, accurate), hip, want)


# ---------------------------------------------------------------------------------------------------------------- tile path
def tile_case(key):
    from svae_amd.lds.lds_inference import natural_lds_estep_general, natural_lds_sample
    n, T, seed = TILE_DRAWS[key]
    init, pair, node = _draw(n, T, seed)
    nat, nodes = _dev_model(init, pair, node)
    with torch.no_grad():
        got = _stats_arrays(*natural_lds_estep_general(nat, nodes, check=True))
        smp = natural_lds_sample(nat, nodes, 1, eps=torch.zeros((1, T, 1, n), dtype=torch.float64, device="cuda"))
    ln, st = _truth_estep(key)
    truth = _stats_arrays(ln, st)
    hip = _distances(got, truth)
    hip["sample0"] = _dist(smp[:, :, 0], st[2][1])
    want = _distances(_stats_arrays(*_ref_estep(key)), truth)
    want["sample0"] = want["Enode_x"]
    return hip, want


@needs_ref
@pytest.mark.parametrize("key", list(TILE_DRAWS))
def test_tile_path_against_truth(key):
    hip, want = tile_case(key)
    _judge(("tile", key), hip, want)


# ------------------------------------------------------------------------------------------------------- fused training VJP
def _closed_form_grad_h(init, pair, node, g_l, g_d, g_x, truth):
    """d/dh of g_l lognorm + <g_d, diag E[xx']> + <g_x, E[x]> = g_l E[x] + Sigma (g_x + 2 g_d * E[x]): one solve"""
    Ex = truth[1][2][1]
    rhs = g_x + 2 * g_d * Ex
    solve = lds_mp.smoothed_means_mp((init[0], np.zeros_like(init[1])), pair, node[0][0], rhs)
    return g_l * Ex + solve


def _estep_cotangent_jvp(natparam, node, v_J, g_l, g_d, g_x):
    d = lds_mp.jvp_mp(lds_mp.estep_mp, (natparam, node), (None, (v_J, None, None)))
    return g_l * d[0] + float(np.sum(g_d * d[1][2][0])) + float(np.sum(g_x * d[1][2][1]))


def _top(a, k):
    return [np.unravel_index(i, a.shape) for i in np.argsort(np.abs(a), axis=None)[::-1][:k]]


def fused_vjp_case(key):
    """node-J / node-h gradients of a random cotangent on (lognorm, diag E[xx'], E[x]) through lds_inference_differentiable
    in both modes and with / without the sampler, against the truth; -> {mode: HIP-vs-truth}, reference-vs-truth"""
    from svae_amd.lds import lds_inference as li
    n, T, seed = DRAWS[key]
    init, pair, node = _draw(n, T, seed)
    node1 = tuple(x[0] for x in node)
    rng = np.random.default_rng(1000 + seed)
    g_l, g_d, g_x = float(rng.standard_normal()), rng.standard_normal((T, n)), rng.standard_normal((T, n))
    (wJ, wh, _), _ = ref.estep_vjp((init, pair), node1, g_l, (g_d, g_x))
    nat, _ = _dev_model(init, pair, node)
    cu = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda")
    grads = {}
    for accurate in (True, False):
        for sampler in (False, True):
            old = li.set_accurate_smoother(accurate)
            try:
                nJ, nh, nz = (cu(x).requires_grad_(True) for x in node)
                eps = torch.zeros((1, T, 1, n), dtype=torch.float64, device="cuda") if sampler else None
                ln, (dxx, x), _, _ = li.lds_inference_differentiable(nat, (nJ, nh, nz), eps=eps)
                ((ln * g_l).sum() + (dxx * cu(g_d)[None]).sum() + (x * cu(g_x)[None]).sum()).backward()
            finally:
                li.set_default_options(old)
            grads[(accurate, sampler)] = (_np(nJ.grad[0]), _np(nh.grad[0]))
    truth = _truth_estep(key)
    th = _closed_form_grad_h(init, pair, node, g_l, g_d, g_x, truth)
    # node J: the coordinates where the fp64 sides disagree most, the largest one, and two random directions
    coords = {_top(wJ, 1)[0]}
    for gJ, _ in grads.values():
        coords.update(_top(gJ - wJ, 2))
    dirs = []
    for c in sorted(coords):
        v = np.zeros((T, n))
        v[c] = 1.0
        dirs.append(v)
    dirs += [rng.standard_normal((T, n)) for _ in range(2)]
    tJ = [_estep_cotangent_jvp((init, pair), node1, v, g_l, g_d, g_x) for v in dirs]
    scale_J = float(np.max(np.abs(wJ)))

    def dist(gJ, gh):       # (a coordinate direction gives |a_k - truth_k| / max|truth|; a random one a lower bound of it)
        eJ = max(abs(float(np.sum(gJ * v)) - t) / (scale_J * float(np.abs(v).sum())) for v, t in zip(dirs, tJ))
        return {"gJ": eJ, "gh": _dist(gh, th)}
    return {k: dist(*g) for k, g in grads.items()}, dist(wJ, wh)


@needs_ref
@pytest.mark.parametrize("key", ["n7_s262", "n8_s116"])
def test_fused_vjp_against_truth(key):
    hip, want = fused_vjp_case(key)
    for (accurate, sampler), d in hip.items():
        _judge(("vjp", key, accurate, sampler), d, want)


# ------------------------------------------------------------------------------------- the three reverse-mode primitives
# Every (kernel, n, form) of tests/test_lds_primitives_hip.py's BOUNDS, on that file's draws and cotangents, plus its seed-262
# case.  The truth is evaluated on the one sequence where the HIP kernel and the reference disagree most.

def _prim():
    import test_lds_primitives_hip as prim      # (tests/ is on sys.path under pytest: the same draws, not a copy of them)
    return prim


def _sym(G):
    """the derivative of a symmetric-matrix argument along E_ij + E_ji (i != j) / E_ii: G + G' - diag(G)"""
    G = np.asarray(G, float)
    return G + np.swapaxes(G, -1, -2) - np.eye(G.shape[-1]) * np.diagonal(G, axis1=-2, axis2=-1)[..., None, :]


def _prim_model(n, T, B, form, seed):
    """tests/test_lds_primitives_hip.py's draw (same rng stream) with exactly symmetric J0, J11, J22 (_symmetric_model)"""
    rng, init3, pairs, lib_pair, node = _prim()._model(n, T, B, form, seed)
    init3 = (_sym_blocks(init3[0]),) + tuple(init3[1:])
    pairs = [_symmetric_model(init3, p)[1] for p in pairs]
    return rng, init3, pairs, _symmetric_model(init3, lib_pair)[1], node


def _ref_messages(init3, pair, node, b):
    msgs, aux = _prim()._ref_messages(init3, pair, node, b)
    for J in (msgs[0][0], msgs[1][0]):         # the reference's messages of a symmetric model are symmetric
        assert np.array_equal(np.asarray(J), np.swapaxes(np.asarray(J), -1, -2))
    return msgs, aux


def _worst_seq(hip, want):
    """index of the sequence where the normwise HIP-vs-reference distance (worst array) is largest"""
    B = hip[0].shape[0]
    return int(np.argmax([max(_dist(h[b], w[b]) for h, w in zip(hip, want)) for b in range(B)]))


def _grad_truth(f, args, place, inner, hip, want, sym, rng, per_array, per_direction=False):
    """(HIP-vs-truth, reference-vs-truth) of gradient arrays of one sequence.  `place(vs)` puts direction arrays vs (one per
    gradient array) into f's argument structure; `inner(d)` = <g, J v> for jvp_mp's output d.  Arrays flagged in `sym` are
    gradients w.r.t. symmetric matrices: their directions are symmetric (E_ij + E_ji), so either convention of splitting
    the gradient between G_ij and G_ji pairs correctly.  Directions: the coordinate of largest normwise |HIP - reference|
    of each array (per_array) or of all arrays, then one random direction over all arrays; a coordinate gives
    |a_k - truth_k| / max|truth|, the random direction a lower bound of the normwise distance.  per_direction=True (with
    per_array): the pair of distances of every direction -- one per array, then the random one -- instead of their maxima."""
    hip = [np.asarray(a, float) for a in hip]
    want = [np.asarray(a, float) for a in want]
    view = lambda G, s: _sym(G) if s else G
    scale = [max(float(np.max(np.abs(view(w, s)))), 1e-300) for w, s in zip(want, sym)]
    cand = [(float(np.max(np.abs(view(h, s) - view(w, s)))) / sc, i, _top(view(h, s) - view(w, s), 1)[0])
            for i, (h, w, s, sc) in enumerate(zip(hip, want, sym, scale))]
    dirs = []
    for _, i, c in (cand if per_array else [max(cand, key=lambda x: x[0])]):
        vs = [np.zeros_like(w) for w in want]
        vs[i][c] = 1.0
        if sym[i]:
            vs[i][c[:-2] + (c[-1], c[-2])] = 1.0
        dirs.append((vs, scale[i]))
    rnd = [rng.standard_normal(w.shape) for w in want]
    rnd = [(r + np.swapaxes(r, -1, -2)) / 2 if s else r for r, s in zip(rnd, sym)]
    dirs.append((rnd, sum(sc * float(np.abs(r).sum()) for sc, r in zip(scale, rnd))))
    each = []
    for vs, norm in dirs:
        t = inner(lds_mp.jvp_mp(f, args, place(vs)))
        dot = lambda G: sum(float(np.sum(g * v)) for g, v in zip(G, vs))
        each.append((abs(dot(hip) - t) / norm, abs(dot(want) - t) / norm))
    return each if per_direction else (max(h for h, _ in each), max(w for _, w in each))


def _filter_run(n, T, B, form):
    """tests/test_lds_primitives_hip.py::test_filter_grad_matches_reference's draw -> hip, want, truth(b)"""
    from svae_amd.lds import cython_lds_inference as P
    prim, m = _prim(), ref._load("cython_lds_inference")
    rng, init3, pairs, lib_pair, node = _prim_model(n, T, B, form, 100 + n + T)
    msgs_list, auxes = zip(*[_ref_messages(init3, pairs[b], node, b) for b in range(B)])
    g = (((rng.standard_normal((B, T, n, n)), rng.standard_normal((B, T, n))),
          (rng.standard_normal((B, T, n, n)), rng.standard_normal((B, T, n)))), rng.standard_normal(B))
    _, inter = P.natural_filter_forward_general(init3, lib_pair, tuple(torch.as_tensor(x).cuda() for x in node))
    (_, _), (Jf, hf) = prim._stack_msgs(msgs_list)
    inter.Jf, inter.hf = Jf.contiguous(), hf.contiguous()
    gJ, gh, _ = P.natural_filter_grad((tuple(tuple(torch.as_tensor(z).cuda() for z in y) for y in g[0]),
                                       torch.as_tensor(g[1]).cuda()), inter)
    cp = lambda x: np.array(x, dtype=float, copy=True)
    wants = [m.natural_filter_grad((((cp(g[0][0][0][b]), cp(g[0][0][1][b])), (cp(g[0][1][0][b]), cp(g[0][1][1][b]))),
                                    float(g[1][b])), auxes[b]) for b in range(B)]
    hip = (_np(gJ), _np(gh))
    want = tuple(np.stack([np.asarray(w[k]) for w in wants]) for k in range(2))

    def truth(b, per_array):
        args = (init3, pairs[b], (node[0][b], node[1][b], node[2][b]))
        gb = [g[0][i][j][b] for i in range(2) for j in range(2)]
        inner = lambda d: sum(float(np.sum(x * y)) for x, y in zip(gb, [d[0][i][j] for i in range(2) for j in range(2)])) \
            + float(g[1][b]) * d[1]
        return _grad_truth(lds_mp.filter_mp, args, lambda vs: (None, None, (vs[0], vs[1], None)), inner,
                           [a[b] for a in hip], [a[b] for a in want], (False, False), np.random.default_rng(b), per_array)
    return hip, want, truth


def _smoother_run(n, T, B, form):
    """test_smoother_grad_matches_reference's draw"""
    from svae_amd.lds import cython_lds_inference as P
    prim, m = _prim(), ref._load("cython_lds_inference")
    rng, init3, pairs, lib_pair, node = _prim_model(n, T, B, form, 200 + n + T)
    msgs_list = [_ref_messages(init3, pairs[b], node, b)[0] for b in range(B)]
    per_step = form != "homog"
    pshape = (B, T - 1, n, n) if per_step else (B, n, n)
    g_init = (rng.standard_normal((B, n, n)), rng.standard_normal((B, n)))
    g_pair = tuple(rng.standard_normal(pshape) for _ in range(3))
    g_node = (rng.standard_normal((B, T, n)), rng.standard_normal((B, T, n)))
    _, inter = P.natural_smoother_general(prim._stack_msgs(msgs_list), lib_pair)
    cu = lambda x: torch.as_tensor(x).cuda()
    got = P.natural_smoother_general_grad(((cu(g_init[0]), cu(g_init[1]), 1., 1.),
                                           (cu(g_pair[0]), cu(g_pair[1]), cu(g_pair[2]), None),
                                           (cu(g_node[0]), cu(g_node[1]), None)), inter)
    hip = tuple(_np(got[i][j]) for i in range(2) for j in range(2))
    cp = lambda x: np.array(x, dtype=float, copy=True)
    wants = []
    for b in range(B):
        _, aux = m.natural_smoother_general(msgs_list[b], pairs[b])
        gb = ((cp(g_init[0][b]), cp(g_init[1][b]), 0., 0.), (cp(g_pair[0][b]), cp(g_pair[1][b]), cp(g_pair[2][b]), 0.),
              (cp(g_node[0][b]), cp(g_node[1][b]), np.zeros(T)))
        w = m.natural_smoother_general_grad(gb, aux)
        wants.append([np.asarray(w[i][j]) for i in range(2) for j in range(2)])
    want = tuple(np.stack([w[k] for w in wants]) for k in range(4))

    def truth(b, per_array):
        msgs = tuple(tuple(np.asarray(x) for x in y) for y in msgs_list[b])
        gs = [g_init[0][b], g_init[1][b]] + [g_pair[k][b] for k in range(3)] + [g_node[0][b], g_node[1][b]]
        inner = lambda d: sum(float(np.sum(x * y)) for x, y in zip(gs, [d[0][0], d[0][1], d[1][0], d[1][1], d[1][2],
                                                                          d[2][0], d[2][1]]))
        place = lambda vs: (((vs[0], vs[1]), (vs[2], vs[3])), None)
        return _grad_truth(lds_mp.smoother_on_messages_mp, (msgs, pairs[b]), place, inner, [a[b] for a in hip],
                           [a[b] for a in want], (True, False, True, False), np.random.default_rng(b), per_array)
    return hip, want, truth


def _sampler_run(n, T, B, form, S):
    """test_sample_grad_matches_reference's draw"""
    from svae_amd.lds import cython_lds_inference as P
    prim, m = _prim(), ref._load("cython_lds_inference")
    rng, init3, pairs, lib_pair, node = _prim_model(n, T, B, form, 300 + n + T)
    msgs_list = [_ref_messages(init3, pairs[b], node, b)[0] for b in range(B)]
    eps_all, auxes = [], []
    for b in range(B):
        np.random.seed(7 + b)
        _, aux = m.natural_sample_backward(msgs_list[b], pairs[b], S)
        np.random.seed(7 + b)
        eps_all.append(np.random.randn(T, S, n)[::-1].copy())
        auxes.append(aux)
    gs = rng.standard_normal((B, T, S, n))
    _, inter = P.natural_sample_backward(prim._stack_msgs(msgs_list), lib_pair, S, eps=np.stack(eps_all))
    (_, _), (gJf, ghf) = P.natural_sample_backward_grad(torch.as_tensor(gs).cuda(), inter)
    hip = (_np(gJf), _np(ghf))
    wants = [m.natural_sample_backward_grad(np.copy(gs[b]), auxes[b])[1] for b in range(B)]
    want = tuple(np.stack([np.asarray(w[k]) for w in wants]) for k in range(2))

    def truth(b, per_array):
        msgs = tuple(tuple(np.asarray(x) for x in y) for y in msgs_list[b])
        place = lambda vs: (((None, None), (vs[0], vs[1])), None, None)
        return _grad_truth(lds_mp.sample_on_messages_mp, (msgs, pairs[b], eps_all[b]), place,
                           lambda d: float(np.sum(gs[b] * d)), [a[b] for a in hip], [a[b] for a in want], (True, False),
                           np.random.default_rng(b), per_array)
    return hip, want, truth


def _bounds_configs(kind, n, form):
    prim = _prim()
    cases = [c for c in prim.CASES if c[0] == n and c[3] == form and (kind != "sampler" or c[2] <= 5)]
    if kind == "sampler":
        return [c + (S,) for c in cases for S in (1, 3, 16)]
    return cases


def primitive_case(kind, n, form):
    """(HIP-vs-truth, reference-vs-truth) on the sequence (of every draw of `kind`, n, form in tests/test_lds_primitives_hip.py)
    where the kernel and the reference disagree most"""
    run = {"filter": _filter_run, "smoother": _smoother_run, "sampler": _sampler_run}[kind]
    worst = None
    for cfg in _bounds_configs(kind, n, form):
        hip, want, truth = run(*cfg)
        b = _worst_seq(hip, want)
        d = max(_dist(h[b], w[b]) for h, w in zip(hip, want))
        if worst is None or d > worst[0]:
            worst = (d, cfg, b, truth)
    d, cfg, b, truth = worst
    return truth(b, cfg[1] <= 25)


BOUNDS_KEYS = [("filter", 10, "batched"), ("smoother", 10, "batched"), ("smoother", 13, "homog"),
               ("smoother", 13, "inhomog"), ("smoother", 13, "batched"), ("smoother", 15, "batched"),
               ("sampler", 10, "batched"), ("sampler", 10, "inhomog"), ("sampler", 15, "batched")]


@needs_ref
@pytest.mark.parametrize("kind,n,form", BOUNDS_KEYS)
def test_primitive_vjp_bounds_cases_against_truth(kind, n, form):
    assert set(BOUNDS_KEYS) == set(_prim().BOUNDS)
    hip, want = primitive_case(kind, n, form)
    _judge(("prim", kind, n, form), {"grad": hip}, {"grad": want})


def seed262_primitive_case(kind):
    """test_conditioning_seed262_all_three_grads's model (n = 7, T = 45, cond(J22) = 7.8e7) with cotangents of its own"""
    from svae_amd.lds import cython_lds_inference as P
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    m = ref._load("cython_lds_inference")
    n, T, S = 7, 45, 3
    rng = np.random.default_rng(262)
    init, pair = _symmetric_model(*rand_lds_natparam(n, rng))
    node = rand_node_potentials((1, T, n), rng, with_logZ=True)
    init3 = (np.asarray(init[0]), np.asarray(init[1]), float(sum(np.sum(x) for x in init[2:])))
    msgs, aux_f = _ref_messages(init3, pair, node, 0)
    msgs = tuple(tuple(np.asarray(x) for x in y) for y in msgs)
    g_rng = np.random.default_rng(9)
    cp = lambda x: np.array(x, dtype=float, copy=True)
    if kind == "filter":
        gf = (((g_rng.standard_normal((T, n, n)), g_rng.standard_normal((T, n))),
               (g_rng.standard_normal((T, n, n)), g_rng.standard_normal((T, n)))), float(g_rng.standard_normal()))
        _, fi = P.natural_filter_forward_general(init3, pair, tuple(np.asarray(x[0]) for x in node))
        fi.Jf, fi.hf = (torch.as_tensor(msgs[1][k])[None].cuda().contiguous() for k in range(2))
        got = P.natural_filter_grad(gf, fi)
        want = m.natural_filter_grad((((cp(gf[0][0][0]), cp(gf[0][0][1])), (cp(gf[0][1][0]), cp(gf[0][1][1]))), gf[1]),
                                     aux_f)
        gb = [gf[0][i][j] for i in range(2) for j in range(2)]
        inner = lambda d: sum(float(np.sum(x * y)) for x, y in zip(gb, [d[0][i][j] for i in range(2) for j in range(2)])) \
            + gf[1] * d[1]
        return _grad_truth(lds_mp.filter_mp, (init3, pair, tuple(x[0] for x in node)),
                           lambda vs: (None, None, (vs[0], vs[1], None)), inner, got[:2], want[:2], (False, False),
                           g_rng, True)
    if kind == "smoother":
        gs = ((g_rng.standard_normal((n, n)), g_rng.standard_normal(n), 0., 0.),
              tuple(g_rng.standard_normal((n, n)) for _ in range(3)) + (0.,),
              (g_rng.standard_normal((T, n)), g_rng.standard_normal((T, n)), np.zeros(T)))
        _, si = P.natural_smoother_general(msgs, pair)
        got = P.natural_smoother_general_grad(gs, si)
        _, aux_s = m.natural_smoother_general(msgs, pair)
        want = m.natural_smoother_general_grad(tuple(tuple(cp(x) if isinstance(x, np.ndarray) else x for x in y)
                                                     for y in gs), aux_s)
        flat = [gs[0][0], gs[0][1], gs[1][0], gs[1][1], gs[1][2], gs[2][0], gs[2][1]]
        inner = lambda d: sum(float(np.sum(x * y)) for x, y in zip(flat, [d[0][0], d[0][1], d[1][0], d[1][1], d[1][2],
                                                                            d[2][0], d[2][1]]))
        return _grad_truth(lds_mp.smoother_on_messages_mp, (msgs, pair), lambda vs: (((vs[0], vs[1]), (vs[2], vs[3])), None),
                           inner, [got[i][j] for i in range(2) for j in range(2)],
                           [want[i][j] for i in range(2) for j in range(2)], (True, False, True, False), g_rng, True)
    np.random.seed(4)
    _, aux_q = m.natural_sample_backward(msgs, pair, S)
    np.random.seed(4)
    eps = np.random.randn(T, S, n)[::-1].copy()
    _, qi = P.natural_sample_backward(msgs, pair, S, eps=eps)
    gq = g_rng.standard_normal((T, S, n))
    got = P.natural_sample_backward_grad(gq, qi)[1]
    want = m.natural_sample_backward_grad(cp(gq), aux_q)[1]
    return _grad_truth(lds_mp.sample_on_messages_mp, (msgs, pair, eps), lambda vs: (((None, None), (vs[0], vs[1])), None, None),
                       lambda d: float(np.sum(gq * d)), got, want, (True, False), g_rng, True)


@needs_ref
@pytest.mark.parametrize("kind", ["filter", "smoother", "sampler"])
def test_primitive_vjp_seed262_against_truth(kind):
    hip, want = seed262_primitive_case(kind)
    _judge(("prim262", kind), {"grad": hip}, {"grad": want})


# ------------------------------------------------------------------------ gradients w.r.t. the init / pair natural parameters
# lds_inference_differentiable(..., natparam_grad=True).  The reference has no compiled parameter gradient: the comparator is
# the fp64 CPU autograd of tests/_lds_large_torch.torch_estep (the oracle of tests/test_lds_param_grads_hip.py and
# tests/test_lds_param_grads_routes_hip.py; pinned to 60 digits on small shapes by tests/test_lds_param_grads_cpu.py).

PGRAD_NAMES = ("init_J", "init_h", "init_logZ", "J11", "J12", "J22", "logZ_pair")
PGRAD_SYM = (True, False, False, True, False, True, False)
PGRAD_STEP_T = 12


def _param_grads(init, pair, node, cot, sampler, hip):
    """the seven parameter gradients of g_l lognorm + <g_d, diag E[xx']> + <g_x, E[x]> [+ <g_s, sample at zero noise>] by
    autograd through the HIP path (hip) or through torch_estep in fp64 on the CPU, as NumPy arrays"""
    import _lds_large_torch as lt
    from svae_amd.lds import lds_inference as li
    g_l, g_d, g_x, g_s = cot
    T, n = node[1].shape[1:]
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda" if hip else "cpu")
    P = [t(x).requires_grad_(True) for x in tuple(init[:3]) + tuple(pair[:4])]
    eps = t(np.zeros((1, T, 1, n))) if sampler else None
    if hip:
        ln, (dxx, x), smp, _ = li.lds_inference_differentiable(((P[0], P[1], P[2]), tuple(P[3:])), tuple(t(a) for a in node),
                                                               eps=eps, natparam_grad=True)
    else:
        ln, dxx, x, smp, _, _ = lt.torch_estep((P[0], P[1], P[2].reshape(1), P[3], P[4], P[5], P[6].reshape(-1)),
                                               t(node[0]), t(node[1]), eps=eps)
    loss = (ln * g_l).sum() + (dxx * t(g_d)[None]).sum() + (x * t(g_x)[None]).sum()
    if sampler:
        loss = loss + (smp[:, :, 0] * t(g_s)[None]).sum()
    loss.backward()
    return [np.zeros(tuple(p.shape)) if p.grad is None else _np(p.grad) for p in P]


def _param_truth(init, pair, node, cot, sampler, hip, want, rng):
    """{array: (HIP-vs-truth, comparator-vs-truth)} + "random": eight jvp_mp evaluations of estep_mp -- per array the
    coordinate where HIP and the comparator part most, then one random direction over all seven.  A sample at zero noise is
    E[x] (x_t = c_t + G_t x_{t+1}) and chol(P_t)^-T eps_t has no derivative at eps = 0: its truth is that of E[x]."""
    g_l, g_d, g_x, g_s = cot
    gx = g_x + g_s if sampler else g_x
    inner = lambda d: g_l * float(d[0]) + float(np.sum(g_d * d[1][2][0])) + float(np.sum(gx * d[1][2][1]))
    place = lambda vs: ((tuple(vs[:3]), tuple(vs[3:])), None)
    each = _grad_truth(lds_mp.estep_mp, ((init, pair), (node[0][0], node[1][0])), place, inner, hip, want, PGRAD_SYM, rng,
                       True, per_direction=True)
    return dict(zip(PGRAD_NAMES + ("random",), each))


def param_grad_case(key, layout, accurate=True):
    """{array: (HIP-vs-truth, comparator-vs-truth)} of the seven parameter gradients of a random cotangent on (lognorm,
    diag E[xx'], E[x]) on draw `key`.  layout "homog"; "homog_zero_noise": with the sampler at zero noise and a cotangent
    on its sample too; "step": the draw cut to T = 12 with the homogeneous blocks repeated per step (T-1,n,n) -- the
    per-step truth from jvp_mp on those arrays, and ("sum_" entries) the HIP gradient summed over t against the
    homogeneous truth."""
    from svae_amd.lds import lds_inference as li
    n, T, seed = DRAWS[key]
    init, pair, node = _draw(n, T, seed)
    init, pair = tuple(init[:3]), tuple(np.asarray(x, float) for x in pair[:4])
    sampler = layout == "homog_zero_noise"
    if layout == "step":
        T = PGRAD_STEP_T
        node = tuple(x[:, :T] for x in node)
    rng = np.random.default_rng(2000 + seed)
    cot = (float(rng.standard_normal()), rng.standard_normal((T, n)), rng.standard_normal((T, n)), rng.standard_normal((T, n)))
    models = [pair]
    if layout == "step":
        models.insert(0, tuple(np.repeat(x[None], T - 1, axis=0) for x in pair))
    old = li.set_accurate_smoother(accurate)
    try:
        hip = _param_grads(init, models[0], node, cot, sampler, True)
    finally:
        li.set_default_options(old)
    out = _param_truth(init, models[0], node, cot, sampler, hip, _param_grads(init, models[0], node, cot, sampler, False), rng)
    if layout == "step":
        summed = hip[:3] + [a.sum(0) for a in hip[3:]]
        total = _param_truth(init, pair, node, cot, sampler, summed, _param_grads(init, pair, node, cot, sampler, False), rng)
        out.update(("sum_" + k, v) for k, v in total.items())
    return out


PGRAD_CASES = [(key, "homog", accurate) for key in ("n7_s0", "n7_s1", "n7_s262", "n8_s116") for accurate in (True, False)] \
    + [("n7_s262", "homog_zero_noise", True), ("n7_s1", "step", True)]


@pytest.mark.parametrize("key,layout,accurate", PGRAD_CASES)
def test_param_gradients_against_truth(key, layout, accurate):
    """accurate mode: every array meets the cond * eps rule (or its GAP_PINS entry under ("pgrad", draw, layout)).  The
    default mode is cond^2 * eps by design: the rule is applied on n7_s0 only, the other draws are printed (PGTRUTH).
    Measured on MI355X: the two modes return the same figures on all four draws -- natparam_grad=True runs on the full
    records either way (GAP_PINS)."""
    d = param_grad_case(key, layout, accurate)
    print("PGTRUTH %s %s %s: " % (key, layout, "accurate" if accurate else "default")
          + ", ".join("%s %.2e|%.2e" % (k, h, w) for k, (h, w) in d.items()))
    if accurate or key == "n7_s0":
        _judge(("pgrad", key, layout), {k: h for k, (h, _) in d.items()}, {k: w for k, (_, w) in d.items()})


# --------------------------------------------------------------------------------------------- host-array entry points
# The reference's calling convention (every argument a NumPy array, no options word): the documented guarantee is that
# ill-conditioned host pair blocks get the cond * eps kernels (lds_inference._host_condition_options).

def host_entry_case(entry):
    from svae_amd.lds import cython_lds_inference as P
    from svae_amd.lds import lds_inference as li
    init, pair, node = _draw(*DRAWS["n7_s262"])
    n, T = node[1].shape[2], node[1].shape[1]
    node1 = tuple(np.asarray(x[0]) for x in node)
    tl, tst = _truth_estep("n7_s262")
    truth = _stats_arrays(tl, tst)
    want = _distances(_stats_arrays(*_ref_estep("n7_s262")), truth)
    zeros = np.zeros((T, 1, n))
    if entry == "natural_lds_estep_general":
        with torch.no_grad():
            return _distances(_stats_arrays(*li.natural_lds_estep_general((init, pair), node1)), truth), want
    if entry == "natural_lds_inference_general":
        with torch.no_grad():
            samples, stats, lognorm = li.natural_lds_inference_general((init, pair), node1, num_samples=1, eps=zeros)
        hip = _distances(_stats_arrays(lognorm, stats), truth)
        hip["sample0"], want["sample0"] = _dist(samples[:, 0], truth["Enode_x"]), want["Enode_x"]
        return hip, want
    if entry == "lds_inference_differentiable":
        rng = np.random.default_rng(5)
        g_l, g_d, g_x = float(rng.standard_normal()), rng.standard_normal((T, n)), rng.standard_normal((T, n))
        cu = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda")
        nJ, nh, nz = (cu(x).requires_grad_(True) for x in node)
        ln, (dxx, x), _, _ = li.lds_inference_differentiable((init, pair), (nJ, nh, nz))
        ((ln * g_l).sum() + (dxx * cu(g_d)[None]).sum() + (x * cu(g_x)[None]).sum()).backward()
        th = _closed_form_grad_h(init, pair, node, g_l, g_d, g_x, (tl, tst))
        (_, wh, _), _ = ref.estep_vjp((init, pair), node1, g_l, (g_d, g_x))
        keys = ("lognorm", "Enode_diagxx", "Enode_x")
        hip = _distances({"lognorm": ln[0], "Enode_diagxx": dxx[0], "Enode_x": x[0]}, {k: truth[k] for k in keys})
        hip["grad_h"] = _dist(nh.grad[0], th)
        return hip, dict({k: want[k] for k in keys}, grad_h=_dist(wh, th))
    m = ref._load("cython_lds_inference")
    init3 = (np.asarray(init[0]), np.asarray(init[1]), float(sum(np.sum(x) for x in init[2:])))
    msgs = tuple(tuple(np.asarray(x) for x in y) for y in m.natural_filter_forward_general(init3, pair, node1)[0][0])
    Ei, Ep, En = lds_mp.smoother_on_messages_mp(msgs, pair)
    truth = _stats_arrays(0., (Ei, Ep, En))
    if entry == "natural_smoother_general":
        stats, _ = P.natural_smoother_general(msgs, pair)
        (wi, wp, wn), _ = ref.smoother(msgs, pair)
        return _distances(_stats_arrays(0., stats), truth), _distances(_stats_arrays(0., (wi, wp, wn)), truth)
    assert entry == "natural_sample_backward"
    samples, _ = P.natural_sample_backward(msgs, pair, 1, eps=zeros)
    # the reference's compiled sampler at zero noise: it draws numpy.random.randn(T, S, n) when called (:333)
    randn = np.random.randn
    np.random.randn = lambda *shape: np.zeros(shape)
    try:
        want, _ = m.natural_sample_backward(msgs, pair, 1)
    finally:
        np.random.randn = randn
    return {"sample0": _dist(samples[:, 0], En[1])}, {"sample0": _dist(np.asarray(want)[:, 0], En[1])}


@needs_ref
@pytest.mark.parametrize("entry", ["natural_lds_estep_general", "natural_lds_inference_general",
                                   "lds_inference_differentiable", "natural_smoother_general", "natural_sample_backward"])
def test_host_array_entry_points_on_the_ill_draw(entry):
    hip, want = host_entry_case(entry)
    _judge(("host", entry), hip, want)
