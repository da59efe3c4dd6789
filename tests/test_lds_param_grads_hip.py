"""Gradients of the LDS inference w.r.t. the init and pair NATURAL PARAMETERS (lds_inference_differentiable(...,
natparam_grad=True); svae_lds_estep_vjp_params_f64) -- the part of the reference's differentiable surface its Python
path has through autograd (lds_inference.py:205-218).

Oracle: fp64 autograd on the CPU through tests/_lds_large_torch.torch_estep (a differentiable restatement of the
recursion).  Metric: `_rel` of tests/test_vjp_hip.py (element-wise, floor 1e-3 of the array's maximum); bound 1e-6 for
all seven gradients, 1e-12 for the two logZ ones (sums of the cotangent of lognorm).  At T = 1 the per-step layouts
(T-1,n,n) / (B,T-1,n,n) have no pair blocks at all -- empty parameter tensors, nothing to differentiate -- so that shape
runs with homogeneous parameters, where the pair gradients must be exact zeros.
Models come from `rand_lds_natparam`, redrawn while cond(init_J) or cond(J22) exceeds MAX_COND = 1e6 (below: what fp64
resolves at the 1e-6 bound; an input-only criterion).
Also: central finite differences of the HIP forward itself, the structural identities between the gradients, bit-exactness
against the default call, and the error paths.
The SHAPES here stop at B = 5, T = 7 and the default options word.  Tested elsewhere:
  * every launch route of launch_vjp's PGR forms (B around 512 / 1024 / 2048, n = 13, S = 5 and 17, the producer bits of
    the options word, the statistics cotangents, every forward variant), every edge of the reduction kernels (a second
    term per chunk, the wrap of the four interleaved sums, the time pass, the entry tiling) and the slab loop at
    B (T-1) > 65535, all against this file's oracle: tests/test_lds_param_grads_routes_hip.py;
  * the parameter gradients against the 60-digit truth of oracle/lds_mp on the ill-conditioned draws:
    tests/test_lds_truth_hip.py::test_param_gradients_against_truth;
  * this file's oracle itself (torch_estep's fp64 autograd) against that truth, every coordinate, without a GPU:
    tests/test_lds_param_grads_cpu.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _lds_large_torch as lt  # noqa: E402  (the oracle: imported, not copied)
from test_vjp_hip import _rel  # noqa: E402  (the metric of the node-gradient tests)

LAYOUTS = ("homog", "step", "batched")
NAMES = ("init_J", "init_h", "init_logZ", "J11", "J12", "J22", "logZ_pair")


# Largest condition number of the blocks the model inverts (Sigma_init = (-2 init_J)^-1, Q = (-2 J22)^-1) a drawn model may
# have.  fp64 resolves a gradient of this recursion to about cond * eps * (growth over the T n^2-term steps, taken as 100):
# at cond = 1e6 that is 1e6 * 1.1e-16 * 100 = 1e-8, two decimal places below the 1e-6 bound, for the oracle and the kernels
# alike.  `rand_lds_natparam` squares a Gaussian matrix, so its draws reach any condition number (5e9 among the first
# draws at n = 10): beyond ~1e8 the CPU oracle itself no longer holds 1e-6 (its autograd and its hand-written adjoint
# already part at 1e-8 there) and the comparison would measure the draw, not the code.  Such draws are redrawn from the
# same stream; the criterion looks at the inputs only.
MAX_COND = 1e6


def _draw_natparam(n, rng):
    from svae_amd.lds.synthetic_data import rand_lds_natparam
    while True:
        init, pair = rand_lds_natparam(n, rng)
        if max(np.linalg.cond(init[0]), np.linalg.cond(pair[2])) <= MAX_COND:
            return init, pair


def _inputs(n, T, B, S, layout, seed):
    """natural parameters in `layout`, node potentials, cotangents of a random linear functional, noise -- NumPy"""
    from svae_amd.lds.synthetic_data import rand_node_potentials
    rng = np.random.default_rng(seed)
    init, pair = _draw_natparam(n, rng)
    if layout != "homog":
        sets = B if layout == "batched" else 1
        draws = [[_draw_natparam(n, rng)[1] for _ in range(T - 1)] for _ in range(sets)]
        pair = tuple(np.stack([np.stack([p[i] for p in row]) for row in draws]) for i in range(4))   # (sets,T-1,..)
        if layout == "step":
            pair = tuple(x[0] for x in pair)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    g = dict(ln=rng.standard_normal(B), dxx=rng.standard_normal((B, T, n)), x=rng.standard_normal((B, T, n)),
             s=rng.standard_normal((B, T, S, n)))
    eps = rng.standard_normal((B, T, S, n)) if S > 0 else None
    return init, pair, node, g, eps


def _leaves(init, pair, device):
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=device).clone().requires_grad_(True)
    return [t(init[0]), t(init[1]), t(init[2]), t(pair[0]), t(pair[1]), t(pair[2]), t(pair[3])]


def _loss(g, outs, S, device):
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=device)
    lognorm, dxx, ex, samples = outs
    loss = (t(g["ln"]) * lognorm).sum() + (t(g["dxx"]) * dxx).sum() + (t(g["x"]) * ex).sum()
    if S > 0:
        loss = loss + (t(g["s"]) * samples).sum()
    return loss


@functools.lru_cache(maxsize=None)
def _oracle(n, T, B, S, layout, seed):
    """the seven parameter gradients + the node gradients by fp64 CPU autograd through torch_estep (computed once per
    case and shared; callers do not modify it)"""
    init, pair, node, g, eps = _inputs(n, T, B, S, layout, seed)
    cpu = torch.device("cpu")
    P = _leaves(init, pair, cpu)
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64)
    nJ, nh = t(node[0]).requires_grad_(True), t(node[1]).requires_grad_(True)
    params = (P[0], P[1], P[2].reshape(1), P[3], P[4], P[5], P[6].reshape(-1))
    lognorm, dxx, ex, samples, _, _ = lt.torch_estep(params, nJ, nh, eps=t(eps) if S > 0 else None)
    _loss(g, (lognorm, dxx, ex, samples), S, cpu).backward()
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().copy()
    return tuple(zero(x) for x in P), (nJ.grad.numpy().copy(), nh.grad.numpy().copy())


def _hip(n, T, B, S, layout, seed, natparam_grad=True, plan=None):
    """-> (parameter gradients | None, (g_node_J, g_node_h), forward outputs) of the HIP path, as device tensors"""
    from svae_amd.lds.lds_inference import lds_inference_differentiable
    init, pair, node, g, eps = _inputs(n, T, B, S, layout, seed)
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev)
    P = _leaves(init, pair, dev)
    nJ, nh, nz = (t(x).requires_grad_(True) for x in node)
    lognorm, (dxx, ex), samples, _ = lds_inference_differentiable(
        ((P[0], P[1], P[2]), (P[3], P[4], P[5], P[6])), (nJ, nh, nz), eps=t(eps) if S > 0 else None, plan=plan,
        natparam_grad=natparam_grad)
    _loss(g, (lognorm, dxx, ex, samples), S, dev).backward()
    fwd = [x.detach().clone() for x in (lognorm, dxx, ex)] + ([samples.detach().clone()] if S > 0 else [])
    if not natparam_grad:
        assert all(x.grad is None for x in P)
        return None, (nJ.grad, nh.grad), fwd
    return [x.grad for x in P], (nJ.grad, nh.grad), fwd


# (n, T, B, S): smallest n; T = 2 with B no multiple of the 4 sequences per wavefront and no samples; T = 1; ...; n > 12;
# largest n; S > 16 (chunked)
SHAPES = [(1, 4, 2, 1), (4, 2, 5, 0), (4, 1, 3, 1), (7, 3, 5, 2), (10, 7, 3, 1), (13, 5, 2, 3), (15, 5, 1, 3), (6, 4, 2, 17)]


# every shape in every layout, except T = 1 per step (no pair blocks to hold a parameter)
CASES = [shape + (layout,) for shape in SHAPES for layout in LAYOUTS if not (shape[1] == 1 and layout != "homog")]


@pytest.mark.parametrize("n,T,B,S,layout", CASES)
def test_parameter_gradients_against_cpu_autograd(n, T, B, S, layout):
    seed = 1000 * n + 10 * T + LAYOUTS.index(layout)
    want, want_node = _oracle(n, T, B, S, layout, seed)
    got, got_node, _ = _hip(n, T, B, S, layout, seed)
    errs = {}
    for name, a, b in zip(NAMES, got, want):
        assert a is not None, name
        assert tuple(a.shape) == tuple(b.shape), name
        if T == 1 and name in ("J11", "J12", "J22", "logZ_pair"):
            assert float(a.abs().max()) == 0.0, name          # no pair step: exact zeros
            continue
        errs[name] = _rel(a, b)
    errs["node_J"], errs["node_h"] = _rel(got_node[0], want_node[0]), _rel(got_node[1], want_node[1])
    print("n=%d T=%d B=%d S=%d %s: " % (n, T, B, S, layout) + ", ".join("%s %.2e" % kv for kv in errs.items()))
    for name, err in errs.items():
        assert err < (1e-12 if "logZ" in name else 1e-6), (name, err)
    for name in ("init_J", "J11", "J22"):                       # returned symmetrised
        a = got[NAMES.index(name)]
        assert torch.equal(a, a.transpose(-1, -2)), name


def test_parameter_gradients_against_finite_differences_of_the_hip_forward():
    """Independent of any restatement: central differences (h = 1e-6) of a random linear functional of the HIP forward's
    outputs at 12 random entries spread over the five array parameters; init_J / J11 / J22 are perturbed symmetrically
    (the forward pass reads them as symmetric matrices), so the difference quotient is g[i,j] + g[j,i] off the diagonal."""
    from svae_amd.lds.lds_inference import lds_inference_differentiable
    n, T, B, S = 4, 6, 2, 2
    init, pair, node, g, eps = _inputs(n, T, B, S, "homog", 5)
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev)
    grads, _, _ = _hip(n, T, B, S, "homog", 5)
    base = [np.asarray(x, float) for x in (init[0], init[1], init[2], pair[0], pair[1], pair[2], pair[3])]

    def f(P):
        lognorm, (dxx, ex), samples, _ = lds_inference_differentiable(
            ((t(P[0]), t(P[1]), t(P[2])), (t(P[3]), t(P[4]), t(P[5]), t(P[6]))), (t(node[0]), t(node[1]), t(node[2])),
            eps=t(eps))
        return float(_loss(g, (lognorm, dxx, ex, samples), S, dev))

    h = 1e-6
    rng = np.random.default_rng(1)
    arrays = [0, 1, 3, 4, 5]                                    # init_J, init_h, J11, J12, J22
    for k in range(12):
        which = arrays[k % 5]
        i, j = int(rng.integers(n)), int(rng.integers(n))
        d = np.zeros_like(base[which])
        gr = grads[which]
        if which == 1:
            d[i] = h
            ana = float(gr[i])
        elif which == 4:
            d[i, j] = h
            ana = float(gr[i, j])
        else:
            d[i, j] = d[j, i] = h
            ana = float(gr[i, j]) + (float(gr[j, i]) if i != j else 0.0)
        P = list(base)
        P[which] = base[which] + d
        fp = f(P)
        P[which] = base[which] - d
        fm = f(P)
        num = (fp - fm) / (2 * h)
        print("%s[%d,%d]: analytic %.10e numeric %.10e" % (NAMES[which], i, j, ana, num))
        assert abs(ana - num) < 2e-5 * max(1.0, abs(num)), (NAMES[which], i, j, ana, num)


def test_structural_identities_between_the_gradients():
    """Per-step parameters: J22_t and J11_{t+1} enter the same pivot block P_{t+1}, init_J and J11_0 the same P_0, and
    the diagonal node potential of step t is the diagonal of what J11_t adds to."""
    n, T, B, S = 5, 6, 3, 2
    got, (gJ, _), _ = _hip(n, T, B, S, "step", 77)
    g = dict(zip(NAMES, got))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(g["J22"][:-1], g["J11"][1:]) < 1e-12
    assert rel(g["init_J"], g["J11"][0]) < 1e-12
    assert rel(torch.diagonal(g["J11"], dim1=-1, dim2=-2), gJ.sum(0)[:T - 1]) < 1e-12
    assert not torch.equal(g["J12"], g["J12"].transpose(-1, -2))          # J12 is no symmetric matrix, nor is its gradient


# B <= 512: one sequence per consumer in sweep 2 (S <= 4), B <= 1024: producer wavefronts (n <= 12), n = 13 / S = 5: the
# packed sweep already -- then a plan without lean records beyond 1024 (packed, two roles up to 2048, fused beyond)
@pytest.mark.parametrize("n,T,B,S,layout", [(4, 3, 5, 2, "homog"), (4, 3, 5, 0, "step"), (6, 4, 3, 5, "batched"),
                                            (13, 3, 2, 1, "homog"), (4, 3, 600, 1, "homog"), (4, 3, 1100, 1, "homog"),
                                            (3, 2, 2052, 1, "homog")])
def test_node_gradients_and_forward_keep_their_bits(n, T, B, S, layout):
    """natparam_grad=True changes neither the node gradients nor (B <= 1024) the forward outputs by a bit, and two runs
    of the parameter gradients are the same bits (fixed summation order, no atomics)."""
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan
    dev = torch.device("cuda:0")
    plans = [None, None, None]
    if B > 1024:      # (the default call keeps lean records there -- another forward pass; compare on full records)
        plans = [LDSEStepPlan(B, T, n, dev, layout != "homog", layout == "batched", options=_lib.OPT_LEAN_OFF)
                 for _ in range(3)]
    _, node0, fwd0 = _hip(n, T, B, S, layout, 3, natparam_grad=False, plan=plans[0])
    p1, node1, fwd1 = _hip(n, T, B, S, layout, 3, plan=plans[1])
    p2, node2, fwd2 = _hip(n, T, B, S, layout, 3, plan=plans[2])
    for a, b in zip(node0, node1):
        assert torch.equal(a, b)
    for a, b in zip(fwd0, fwd1):
        assert torch.equal(a, b)
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)
    for a, b in zip(node1, node2):
        assert torch.equal(a, b)


def test_error_paths_raise_before_any_launch():
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan, lds_inference_differentiable
    dev = torch.device("cuda:0")
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=dev)

    def call(n, T, B, plan):
        init, pair, node, g, eps = _inputs(n, T, B, 1, "homog", 9)
        return lds_inference_differentiable((tuple(t(x) for x in init), tuple(t(x) for x in pair)),
                                            (t(node[0]), t(node[1])), eps=t(eps), plan=plan, natparam_grad=True)

    plan = LDSEStepPlan(2, 4, 16, dev)
    with pytest.raises(ValueError, match="15"):
        call(16, 4, 2, plan)
    assert plan.epoch == 0
    with pytest.raises(ValueError, match="15"):
        call(16, 4, 2, None)
    lean = LDSEStepPlan(2, 4, 4, dev, options=_lib.OPT_LEAN_ON)
    with pytest.raises(ValueError, match="lean"):
        call(4, 4, 2, lean)
    assert lean.epoch == 0
    # .. and the plan-level call after a lean forward pass
    init, pair, node, g, eps = _inputs(4, 4, 2, 1, "homog", 9)
    lean.infer(t(init[0]), t(init[1]), t(init[2]).reshape(1), t(pair[0]), t(pair[1]), t(pair[2]), t(pair[3]).reshape(1),
               t(node[0]), t(node[1]), None, False, t(eps))
    assert lean.lean and lean.epoch == 1
    with pytest.raises(ValueError, match="lean"):
        lean.vjp(t(g["ln"]), param_out=True)
    assert lean.epoch == 1
