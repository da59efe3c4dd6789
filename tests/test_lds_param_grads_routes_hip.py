"""The LDS parameter gradients (lds_inference_differentiable(..., natparam_grad=True); LDSEStepPlan.vjp(param_out=True);
svae_lds_estep_vjp_params_f64) on EVERY LAUNCH ROUTE and at every edge of their reduction, against the oracle of
tests/test_lds_param_grads_hip.py: fp64 CPU autograd through tests/_lds_large_torch.torch_estep (itself pinned to 60
digits by tests/test_lds_param_grads_cpu.py), the same draws (`_inputs`, models redrawn until cond <= MAX_COND = 1e6), the
same random linear functional (`_loss`), the same metric (`_rel` of tests/test_vjp_hip.py).  That file's SHAPES stop at
B = 5, T = 7 and the default options word; the thresholds below are read from the sources.

What every case asserts (`_check`): all seven parameter gradients and both node gradients within the project's 1e-6
(element-wise, `_rel`); the sums of the lognorm cotangent (init_logZ, the shared logZ_pair) within
B * 2^-53 * sum_b |g_b| of the oracle AND of the correctly rounded sum (math.fsum) -- N u sum|terms|, the a-priori
bound of any summation order of N terms, so derived, not measured; the homogeneous logZ_pair is T-1 times the batch sum in
the kernel (T-1 times the bound against fsum) and a sum of N = B (T-1) terms in the oracle's autograd ((T-1)^2 times the
bound against the oracle); init_J / J11 / J22 exactly symmetric;
in the `batched` layout logZ_pair[b, t] == g_lognorm[b] exactly.  Each case prints its worst `_rel` (PGROUTES, pytest -s).

Reduction kernels (svae_amd/csrc/lds_param_grad.hip): a workgroup owns 16 entries, its 16 chunks take the terms
r = chunk, chunk + 16, .. in FOUR interleaved partial sums (u & 3) and meet in a fixed LDS tree.
  BATCH_EDGES  n = 3, T = 3, S = 1, `homog` and `step`:  B = 16 one term per chunk; 17 a second term in chunk 0 only;
               33 uneven chunks (3 / 2 terms); 64 all four partial sums used; 65 the interleave wraps (a fifth term in
               chunk 0); 81 wraps in chunk 0 alone, uneven again (6 / 5 terms)
  TIME_EDGES   `homog`, B = 2, n = 3, S = 0: T = 17, 18, 66 -- the time pass (lds_param_grad_time_kernel) has 16, 17 and 65
               terms: one per chunk, a second one, the wrap
  ENTRY_TILING B = 17, T = 3, S = 1: n = 4 (nn = 16: exactly one workgroup of pair entries; the init block's
               nn + n + 1 = 21 entries end in a second one), n = 5 (two workgroups, the last one partial), n = 15
               (nn + n + 1 = 241: the workgroup that writes g_init_logZ and the shared logZ_pair holds that one entry
               only), and n = 15, T = 4 in the `step` layout (logZ_pair[t] = gsum for every t)
Launch routes (launch_vjp, svae_amd/csrc/lds_vjp_kernel.hpp): VJP_S4_MAX_B = 512 (one sequence per consumer up to it),
prod_max_b = 1024 (producer wavefronts up to it; lds_estep.hip decode_options: 0 with OPT_PRODUCERS_OFF, unbounded
with OPT_PRODUCERS_ON), VJP_PROD2_MAX_N = 12 (no producer sweep 2 beyond), VJP_SPLIT_MAX_S = 4 and B <= 2048 (two-role
`split` launches).  Only the packed sweep 2 in its PGR form writes g_P / g_R; `pg_only` = 1 makes it a second pass that
leaves the node gradients of the sweep 2 before it alone.
  ROUTES_S0    T = 3, `homog`: (n 4, B 512) one-sequence sweeps, PGR <N,false,false,true> as second pass; (4, 513)
               producer sweep 2, PGR as second pass; (13, 513) n > 12: no producer sweep 2, PGR alone (pg_only = 0);
               (4, 1025) B > prod_max_b: packed sweeps, PGR alone
  ROUTES_S     T = 3, S = 2: n = 4 at B = 512 (s4 sweep 2 + PGR <N,true,true,true> second pass), 513 (producer sweep 2 +
               second pass), 1025 (<N,true,true,true> with pg_only = 0), 2048 | 2049 (the edge split | not split:
               <N,true,false,true>); (13, 513) split, no producer sweep 2; (4, B 40, S 5) S > VJP_SPLIT_MAX_S: not split
               at a small batch; (4, 40, 17) S > 16: LDSEStepPlan.vjp adds the parameter gradients of its second chunk
  options      (n 4, T 3, B 40, S 0 | 2) on plans with OPT_PRODUCERS_OFF (prod_max_b = 0: PGR alone at a small batch)
               and OPT_PRODUCERS_ON, each | OPT_LEAN_OFF: both against the oracle and each other (twice the bound)
  statistics   pair_stats_grad=True with natparam_grad=True, cotangents on E_init and E_pair too (the `statc` forms
               of sweep 1), (n 4, T 4, B 33, S 0 | 2), `homog` (summed E_pair) and `step` (per-step E_pair)
  forward      (n 7, T 5, B 9, S 1, `homog`) once per options word of _lib.KERNEL_OPTIONS, | OPT_LEAN_OFF (full records)
  slab loop    `batched`, n = 2, T = 3, B = 32769, S = 0 | 1: grid.y is 16 bits wide and B (T-1) = 65538 > 65535, so
               svae_lds_param_grad_launch cuts the launch into slabs of 65535 / (T-1) = 32767 whole sequences and a
               remainder of 2; every sequence has pair parameters of its own, and the first and the last sequence run
               alone (B = 1) must give the same blocks (twice the bound)
  layouts      (n 5, T 4, B 70, S 1): `step` == sum_b `batched` of the model with its pair parameters replicated,
               `homog` == sum_t `step` of the model with its blocks repeated; tolerance: the sum of the terms'
               element-wise oracle bounds."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _lds_large_torch as lt  # noqa: E402  (the oracle: imported, not copied)
from test_lds_param_grads_hip import NAMES, _inputs, _leaves, _loss  # noqa: E402  (the draws and the functional of that file)
from test_vjp_hip import _rel  # noqa: E402

BOUND = 1e-6
U = 2.0 ** -53


def _seed(n, T, B, S):
    return 100000 * n + 1000 * T + 7 * B + S


@functools.lru_cache(maxsize=None)
def _case(n, T, B, S, layout):
    """`_inputs` of the case, drawn once (the slab case draws 65538 models)"""
    return _inputs(n, T, B, S, layout, _seed(n, T, B, S))


def _with_S(inputs, S):
    """the same draw with its first S samples only"""
    init, pair, node, g, eps = inputs
    return init, pair, node, dict(g, s=g["s"][:, :, :S]), (eps[:, :, :S] if S > 0 else None)


def _take(inputs, b):
    """sequences `b` (a slice) of a `batched` draw"""
    init, pair, node, g, eps = inputs
    return (init, tuple(x[b] for x in pair), tuple(x[b] for x in node), {k: v[b] for k, v in g.items()},
            None if eps is None else eps[b])


def _stat_cotangents(inputs, seed):
    """cotangents of E_init (B, n*n+n) and of E_pair ((B,3,n,n) summed for homogeneous parameters, else (B,T-1,3,n,n))"""
    init, pair, node, g, eps = inputs
    B, T, n = node[1].shape
    rng = np.random.default_rng(seed)
    lead = (B, 3) if np.ndim(pair[0]) == 2 else (B, T - 1, 3)
    return dict(g, Ei=rng.standard_normal((B, n * n + n)), Ep=rng.standard_normal(lead + (n, n)))


def _functional(g, outs, dev):
    lognorm, dxx, ex, samples, E_init, E_pair = outs
    S = g["s"].shape[2]
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev)
    loss = _loss(g, (lognorm, dxx, ex, samples), S, dev)
    if "Ei" in g:
        loss = loss + (t(g["Ei"]) * E_init).sum() + (t(g["Ep"]) * E_pair).sum()
    return loss


def _oracle_run(inputs):
    """-> (the seven parameter gradients, (g_node_J, g_node_h)) by fp64 CPU autograd through torch_estep, NumPy"""
    init, pair, node, g, eps = inputs
    cpu = torch.device("cpu")
    P = _leaves(init, pair, cpu)
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64)
    nJ, nh = t(node[0]).requires_grad_(True), t(node[1]).requires_grad_(True)
    params = (P[0], P[1], P[2].reshape(1), P[3], P[4], P[5], P[6].reshape(-1))
    outs = lt.torch_estep(params, nJ, nh, eps=None if eps is None else t(eps), per_step_stats=np.ndim(pair[0]) != 2)
    _functional(g, outs, cpu).backward()
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().copy()
    return tuple(zero(x) for x in P), (nJ.grad.numpy().copy(), nh.grad.numpy().copy())


@functools.lru_cache(maxsize=None)
def _oracle(n, T, B, S, layout, S_used=None):
    """the oracle of a drawn case, computed once and shared (callers do not modify it)"""
    inputs = _case(n, T, B, S, layout)
    return _oracle_run(inputs if S_used is None else _with_S(inputs, S_used))


def _hip_run(inputs, plan=None):
    """-> (the seven parameter gradients, (g_node_J, g_node_h)) of the HIP path, device tensors"""
    from svae_amd.lds.lds_inference import lds_inference_differentiable
    init, pair, node, g, eps = inputs
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev)
    P = _leaves(init, pair, dev)
    nJ, nh, nz = (t(x).requires_grad_(True) for x in node)
    lognorm, (dxx, ex), samples, (E_init, E_pair) = lds_inference_differentiable(
        ((P[0], P[1], P[2]), (P[3], P[4], P[5], P[6])), (nJ, nh, nz), eps=None if eps is None else t(eps), plan=plan,
        natparam_grad=True, pair_stats_grad="Ei" in g)
    _functional(g, (lognorm, dxx, ex, samples, E_init, E_pair), dev).backward()
    for x in P:
        assert x.grad is not None
    return [x.grad for x in P], (nJ.grad, nh.grad)


def _check(group, inputs, got, got_node, want, want_node):
    """the assertions every case makes (module docstring); -> {name: _rel}"""
    init, pair, node, g, eps = inputs
    B, T, n = node[1].shape
    layout = {2: "homog", 3: "step", 4: "batched"}[np.ndim(pair[0])]
    # (the node gradients first: g_init_h is a sum of g_node_h, so a sweep 2 that leaves them unwritten is named as such)
    errs = {"node_J": _rel(got_node[0], want_node[0]), "node_h": _rel(got_node[1], want_node[1])}
    for name, a, b in zip(NAMES, got, want):
        assert tuple(a.shape) == tuple(b.shape), name
        errs[name] = _rel(a, b)
    worst = max(errs, key=errs.get)
    print("PGROUTES %s n=%d T=%d B=%d S=%d %s: worst %s %.2e" % (group, n, T, B, g["s"].shape[2], layout, worst, errs[worst]))
    for name, err in errs.items():
        assert err < BOUND, (name, err)
    # the sums of the cotangent of lognorm: any summation order is within (B - 1) u sum|g| of the exact sum, the correctly
    # rounded one within u |sum|: B u sum|g| covers both
    gl = g["ln"]
    tol = B * U * float(np.abs(gl).sum())
    exact = math.fsum(gl)
    gz0, gzp = float(got[2].reshape(-1)[0]), got[6].detach().cpu().numpy()
    assert abs(gz0 - float(want[2])) <= tol and abs(gz0 - exact) <= tol, ("init_logZ", gz0, float(want[2]), exact, tol)
    if layout == "homog":
        # the kernel forms (T-1) x the batch sum: T-1 times its bound.  The oracle's autograd adds the B (T-1) terms g_b
        # one by one: the same a-priori bound with N = B (T-1) terms of absolute sum (T-1) sum|g|
        gp = float(gzp.reshape(-1)[0])
        assert abs(gp - (T - 1) * exact) <= (T - 1) * tol, ("logZ_pair", gp, (T - 1) * exact, tol)
        assert abs(gp - float(want[6])) <= (T - 1) ** 2 * tol, ("logZ_pair", gp, float(want[6]), tol)
    elif layout == "step":
        assert gzp.shape == (T - 1,)
        assert np.all(np.abs(gzp - want[6]) <= tol) and np.all(np.abs(gzp - exact) <= tol), ("logZ_pair", gzp, want[6], exact, tol)
    else:
        assert np.array_equal(gzp, np.repeat(gl[:, None], T - 1, axis=1)), "logZ_pair[b, t] == g_lognorm[b]"
    for name in ("init_J", "J11", "J22"):                       # returned symmetrised
        a = got[NAMES.index(name)]
        assert torch.equal(a, a.transpose(-1, -2)), name
    return errs


def _run_case(group, n, T, B, S, layout, plan=None):
    inputs = _case(n, T, B, S, layout)
    want, want_node = _oracle(n, T, B, S, layout)
    got, got_node = _hip_run(inputs, plan)
    _check(group, inputs, got, got_node, want, want_node)
    return got, got_node


BATCH_EDGES = [(3, 3, B, 1, layout) for layout in ("homog", "step") for B in (16, 17, 33, 64, 65, 81)]
TIME_EDGES = [(3, T, 2, 0, "homog") for T in (17, 18, 66)]
ENTRY_TILING = [(4, 3, 17, 1, "homog"), (5, 3, 17, 1, "homog"), (15, 3, 17, 1, "homog"), (15, 4, 17, 1, "step")]
ROUTES_S0 = [(4, 3, 512, 0, "homog"), (4, 3, 513, 0, "homog"), (13, 3, 513, 0, "homog"), (4, 3, 1025, 0, "homog")]
ROUTES_S = [(4, 3, B, 2, "homog") for B in (512, 513, 1025, 2048, 2049)] + [
    (13, 3, 513, 2, "homog"), (4, 3, 40, 5, "homog"), (4, 3, 40, 17, "homog")]


@pytest.mark.parametrize("n,T,B,S,layout", BATCH_EDGES)
def test_batch_reduction_edges(n, T, B, S, layout):
    _run_case("batch", n, T, B, S, layout)


@pytest.mark.parametrize("n,T,B,S,layout", TIME_EDGES)
def test_time_reduction_edges(n, T, B, S, layout):
    _run_case("time", n, T, B, S, layout)


@pytest.mark.parametrize("n,T,B,S,layout", ENTRY_TILING)
def test_entry_tiling(n, T, B, S, layout):
    _run_case("tiling", n, T, B, S, layout)


@pytest.mark.parametrize("n,T,B,S,layout", ROUTES_S0)
def test_routes_without_sample_cotangents(n, T, B, S, layout):
    _run_case("routes_s0", n, T, B, S, layout)


@pytest.mark.parametrize("n,T,B,S,layout", ROUTES_S)
def test_routes_with_sample_cotangents(n, T, B, S, layout):
    _run_case("routes_s", n, T, B, S, layout)


@pytest.mark.parametrize("S", [0, 2])
def test_producers_switched_by_the_options_word(S):
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan
    n, T, B = 4, 3, 40
    dev = torch.device("cuda:0")
    runs = []
    for word in (_lib.OPT_PRODUCERS_OFF, _lib.OPT_PRODUCERS_ON):
        plan = LDSEStepPlan(B, T, n, dev, options=word | _lib.OPT_LEAN_OFF)
        runs.append(_run_case("options_%#x" % word, n, T, B, S, "homog", plan))
    (off, off_node), (on, on_node) = runs
    for name, a, b in zip(NAMES + ("node_J", "node_h"), list(off) + list(off_node), list(on) + list(on_node)):
        assert _rel(a, b.detach().cpu().numpy()) < 2 * BOUND, name


@pytest.mark.parametrize("layout", ["homog", "step"])
@pytest.mark.parametrize("S", [0, 2])
def test_statistics_cotangents_with_parameter_gradients(S, layout):
    n, T, B = 4, 4, 33
    inputs = _case(n, T, B, S, layout)
    init, pair, node, g, eps = inputs
    inputs = (init, pair, node, _stat_cotangents(inputs, 11 + S), eps)
    want, want_node = _oracle_run(inputs)
    got, got_node = _hip_run(inputs)
    _check("statc", inputs, got, got_node, want, want_node)


def _full_record_words():
    from svae_amd import _lib
    words = {}
    for name, word in _lib.KERNEL_OPTIONS.items():
        words.setdefault(word | _lib.OPT_LEAN_OFF, name)
    return sorted(words.items())


@pytest.mark.parametrize("word,name", _full_record_words())
def test_forward_variants(word, name):
    from svae_amd.lds.lds_inference import LDSEStepPlan
    n, T, B, S = 7, 5, 9, 1
    plan = LDSEStepPlan(B, T, n, torch.device("cuda:0"), options=word)
    assert not plan.lib.svae_lds_inference_is_lean(B, T, n, S, 0, 1, word)          # full per-step records
    _run_case("forward_" + name, n, T, B, S, "homog", plan)


SLAB = (2, 3, 32769, 1, "batched")          # drawn once with S = 1; the S = 0 case drops the sample cotangents


@pytest.mark.parametrize("S", [0, 1])
def test_slab_loop_of_the_per_sequence_layout(S):
    n, T, B = SLAB[:3]
    assert B * (T - 1) > 65535 and B == 65535 // (T - 1) + 2           # one full slab and a remainder of 2
    inputs = _with_S(_case(*SLAB), S)
    want, want_node = _oracle(*SLAB, S_used=S)
    got, got_node = _hip_run(inputs)
    _check("slab", inputs, got, got_node, want, want_node)
    # every sequence has a model of its own: the blocks of different sequences differ in the oracle
    assert not np.array_equal(want[3][0], want[3][B - 1]) and not np.array_equal(want[3][B - 3], want[3][B - 2])
    for b in (0, B - 1):
        alone, _ = _hip_run(_take(inputs, slice(b, b + 1)))
        for name in ("J11", "J12", "J22", "logZ_pair"):
            k = NAMES.index(name)
            ref = want[k][b:b + 1]
            scale = np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(want[k])))      # (`_rel`'s scale, of the whole array)
            diff = np.abs(got[k][b:b + 1].cpu().numpy() - alone[k].cpu().numpy())
            assert np.all(diff <= 2 * BOUND * scale), (name, b, float(np.max(diff / scale)))


def _term_bounds(want):
    """element-wise oracle bound of each term (leading axis) of an array: BOUND x `_rel`'s scale; summed over the terms"""
    want = np.asarray(want, float)
    return (BOUND * np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want)))).sum(0)


def test_shared_against_per_sequence_layouts():
    n, T, B, S = 5, 4, 70, 1
    pairs = ("J11", "J12", "J22", "logZ_pair")
    # step == sum_b batched, the (T-1,n,n) blocks replicated over the batch
    step = _case(n, T, B, S, "step")
    init, pair, node, g, eps = step
    batched = (init, tuple(np.repeat(np.asarray(x)[None], B, axis=0) for x in pair), node, g, eps)
    got_s, node_s = _hip_run(step)
    got_b, node_b = _hip_run(batched)
    want_b, _ = _oracle_run(batched)
    for name in pairs:
        k = NAMES.index(name)
        diff = np.abs(got_s[k].cpu().numpy() - got_b[k].sum(0).cpu().numpy())
        tol = _term_bounds(want_b[k])
        print("PGROUTES layouts step-vs-batched %s: %.2e of the tolerance" % (name, float(np.max(diff / tol))))
        assert np.all(diff <= tol), (name, float(np.max(diff / tol)))
    for k in range(3):                                           # the init gradients: the same sums in both layouts
        assert _rel(got_s[k], got_b[k].cpu().numpy()) < 2 * BOUND, NAMES[k]
    for a, b in zip(node_s, node_b):
        assert _rel(a, b.cpu().numpy()) < 2 * BOUND
    # homog == sum_t step, the (n,n) blocks repeated over time
    homog = _case(n, T, B, S, "homog")
    init, pair, node, g, eps = homog
    rep = (init, tuple(np.repeat(np.asarray(x, float)[None], T - 1, axis=0) for x in pair), node, g, eps)
    got_h, node_h = _hip_run(homog)
    got_r, node_r = _hip_run(rep)
    want_r, _ = _oracle_run(rep)
    for name in pairs:
        k = NAMES.index(name)
        diff = np.abs(got_h[k].cpu().numpy() - got_r[k].sum(0).cpu().numpy())
        tol = _term_bounds(want_r[k])
        print("PGROUTES layouts homog-vs-step %s: %.2e of the tolerance" % (name, float(np.max(diff / tol))))
        assert np.all(diff <= tol), (name, float(np.max(diff / tol)))
    for k in range(3):
        assert _rel(got_h[k], got_r[k].cpu().numpy()) < 2 * BOUND, NAMES[k]
    for a, b in zip(node_h, node_r):
        assert _rel(a, b.cpu().numpy()) < 2 * BOUND
