"""GPU tests of the LDS E-step for latent dimension 65 <= n <= 128 (svae_amd/csrc/lds_estep_xl.hip) against the NumPy
oracle, the reference's own compiled E-step (oracle/_ref) and the long-double restatement (oracle/lds_longdouble)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import lds_longdouble, lds_numpy, ref  # noqa: E402  (checkers only)
from svae_amd.lds.synthetic_data import (rand_lds_natparam, rand_node_potentials,  # noqa: E402
                                         rotation_lds_natparam)

DEV = "cuda:0"


def _t(x):
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=DEV)


def _nat(natparam):
    return (tuple(_t(x) for x in natparam[0]), tuple(_t(x) for x in natparam[1]))


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, float)


def _rel(a, b):
    a, b = _np(a), np.asarray(b, float)
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale)) if b.size else 0.0


def _flat(out):
    lognorm, (Ei, Ep, En) = out
    return [lognorm, Ei[0], Ei[1], Ep[0], Ep[1], Ep[2], En[0], En[1]]


def _seq(out, b):
    lognorm, (Ei, Ep, En) = out
    return (lognorm[b], (tuple(x[b] for x in Ei[:2]), tuple(x[b] for x in Ep[:3]), tuple(x[b] for x in En[:2])))


def _check(got, want, tol):
    for k, (g, w) in enumerate(zip(_flat(got), _flat(want))):
        assert _rel(g, w) < tol, (k, _rel(g, w))


def _dist(a, t):
    """normwise distance (scalars: relative to max(|t|, 1))"""
    a, t = _np(a), np.asarray(t, float)
    scale = max(abs(float(t)), 1.0) if t.ndim == 0 else max(float(np.max(np.abs(t))), 1e-300)
    return float(np.max(np.abs(a - t)) / scale) if t.size else 0.0


def _check_arbitrated(got, want, natparam, node, tol=1e-7):
    """`got` within `tol` of the fp64 oracle `want` on every output; where it is not (rand_lds_natparam's conditioning grows
    with n), the long-double truth decides: the kernel's normwise distance to it at most 3x the oracle's (floor 1e-11),
    the rule tests/test_lds_truth_hip.py applies to cond * eps paths"""
    truth = None
    for k, (g, w) in enumerate(zip(_flat(got), _flat(want))):
        if _rel(g, w) < tol:
            continue
        if truth is None:
            truth = _flat(lds_longdouble.estep(natparam, node))
        assert _dist(g, truth[k]) <= max(3 * _dist(w, truth[k]), 1e-11), (k, _rel(g, w), _dist(g, truth[k]),
                                                                          _dist(w, truth[k]))


def _run(natparam, node, **kw):
    from svae_amd.lds.lds_inference import natural_lds_estep_general
    return natural_lds_estep_general(_nat(natparam), tuple(_t(x) for x in node), **kw)


def _symmetric(natparam):
    """exactly symmetric J0, J11, J22 (the kernels and the reference read opposite triangles)"""
    (J0, h0, z0), (J11, J12, J22, zp) = natparam
    s = lambda M: 0.5 * (M + np.swapaxes(M, -1, -2))
    return (s(J0), h0, z0), (s(J11), J12, s(J22), zp)


@pytest.mark.parametrize("n,T", [(65, 3), (72, 1), (79, 2), (80, 4), (96, 2), (97, 3), (112, 1), (113, 2), (127, 3),
                                 (128, 4)])
def test_xl_estep_matches_oracle(n, T):
    rng = np.random.default_rng(7 * n + T)
    natparam = rand_lds_natparam(n, rng)
    node = rand_node_potentials((T, n), rng, with_logZ=True)
    _check_arbitrated(_run(natparam, node), lds_numpy.natural_lds_estep_general(natparam, node), natparam, node)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("n", [80, 128])
def test_xl_estep_batched_matches_compiled_reference(n):
    B, T = 3, 9
    rng = np.random.default_rng(n)
    natparam = rand_lds_natparam(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    out = _run(natparam, node)
    for b in range(B):
        _check(_seq(out, b), ref.estep(natparam, tuple(x[b] for x in node)), 1e-7)


@pytest.mark.parametrize("n,batched", [(72, False), (72, True), (128, False), (128, True)])
def test_xl_estep_per_step_and_per_sequence_pairs(n, batched):
    B, T = 3, 5
    rng = np.random.default_rng(3 * n + batched)
    init = rand_lds_natparam(n, rng)[0]
    pairs = [[rand_lds_natparam(n, rng)[1] for _ in range(T - 1)] for _ in range(B if batched else 1)]
    stack = lambda i: np.stack([np.stack([p[i] for p in row]) for row in pairs])
    pair = tuple(stack(i) for i in range(4))                 # (B|1, T-1, n, n) x3, (B|1, T-1)
    if not batched:
        pair = tuple(x[0] for x in pair)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    out = _run((init, pair), node)
    for b in range(B):
        pb = tuple(x[b] for x in pair) if batched else pair
        nb = tuple(x[b] for x in node)
        want = ref.estep((init, pb), nb) if ref.available() else lds_numpy.natural_lds_estep_general((init, pb), nb)
        _check_arbitrated(_seq(out, b), want, (init, pb), nb)


@pytest.mark.parametrize("n", [96, 128])
def test_xl_estep_full_length_well_conditioned(n):
    """T = 200 on the rotation model, one workgroup round more than the CUs (B = CU count + 37)"""
    T = 200
    B = torch.cuda.get_device_properties(0).multi_processor_count + 37
    rng = np.random.default_rng(n)
    natparam = _symmetric(rotation_lds_natparam(n, rng))
    node = rand_node_potentials((B, T, n), rng)
    out = _run(natparam, node)
    for b in (0, B - 1):
        _check(_seq(out, b), lds_longdouble.estep(natparam, (node[0][b], node[1][b])), 1e-10)
    if ref.available():
        for b in (0, B // 2, B - 1):
            _check(_seq(out, b), ref.estep(natparam, (node[0][b], node[1][b], np.zeros(T))), 1e-8)


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("n,seed", [(96, 96), (128, 128)])
def test_xl_estep_on_the_reference_generator_within_3x_of_the_reference(n, seed):
    """rand_lds_natparam (the reference's own generator, cond(J22) ~ 1e5..1e7): per output array, the kernel's distance
    to the long-double truth is at most 3x the compiled reference's (floor 1e-11)"""
    T = 50
    rng = np.random.default_rng(seed)
    natparam = _symmetric(rand_lds_natparam(n, rng))
    node = rand_node_potentials((1, T, n), rng, with_logZ=True)
    nb = tuple(x[0] for x in node)
    truth = _flat(lds_longdouble.estep(natparam, nb))
    hip = _flat(_seq(_run(natparam, node), 0))
    theirs = _flat(ref.estep(natparam, nb))

    for k in range(len(truth)):
        d_hip, d_ref = _dist(hip[k], truth[k]), _dist(theirs[k], truth[k])
        assert d_hip <= max(3 * d_ref, 1e-11), (k, d_hip, d_ref)


def test_xl_estep_flags_indefinite_potentials():
    n, T = 80, 4
    rng = np.random.default_rng(0)
    natparam = rand_lds_natparam(n, rng)
    J, h = rand_node_potentials((2, T, n), rng)
    J[1, 2] = +50.0                      # makes the filtered precision indefinite
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    plan = LDSEStepPlan(2, T, n, DEV)
    natural_lds_estep_general(_nat(natparam), (_t(J), _t(h)), plan=plan)
    assert int(plan.info.item()) == 2    # sequence 1 (+1)
    plan.info.zero_()
    with pytest.raises(FloatingPointError):
        natural_lds_estep_general(_nat(natparam), (_t(J), _t(h)), plan=plan, check=True)


def test_xl_plumbing_repeatable_single_and_empty_batches():
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    n, T = 100, 6
    rng = np.random.default_rng(5)
    natparam = rand_lds_natparam(n, rng)
    node = rand_node_potentials((3, T, n), rng, with_logZ=True)
    a = [x.clone() for x in _flat(_run(natparam, node))]
    b = _flat(_run(natparam, node))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    one = _run(natparam, tuple(x[:1] for x in node))
    n0 = tuple(x[0] for x in node)
    _check_arbitrated(_seq(one, 0), lds_numpy.natural_lds_estep_general(natparam, n0), natparam, n0)
    # B = 0: the call succeeds and returns empty outputs
    plan = LDSEStepPlan(0, T, n, DEV)
    empty = torch.empty(0, T, n, dtype=torch.float64, device=DEV)
    lognorm, (Ei, Ep, En) = natural_lds_estep_general(_nat(natparam), (empty, empty), plan=plan)
    assert lognorm.shape == (0,) and Ei[0].shape == (0, n, n) and En[1].shape == (0, T, n)


def test_xl_graph_capture_replays_bitwise():
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general
    n, T, B = 96, 12, 4
    rng = np.random.default_rng(9)
    natparam = rand_lds_natparam(n, rng)
    nat = _nat(natparam)
    node = [_t(x) for x in rand_node_potentials((B, T, n), rng)]
    plan = LDSEStepPlan(B, T, n, DEV)
    natural_lds_estep_general(nat, tuple(node), plan=plan)          # warm-up (LDS grant, buffers)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = natural_lds_estep_general(nat, tuple(node), plan=plan)
    new = rand_node_potentials((B, T, n), rng)
    for dst, src in zip(node, new):
        dst.copy_(_t(src))
    graph.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in _flat(out)]
    eager = _flat(natural_lds_estep_general(nat, tuple(_t(x) for x in new), plan=LDSEStepPlan(B, T, n, DEV)))
    for x, y in zip(got, eager):
        assert torch.equal(x, y)


def test_xl_reduce_stats_is_the_batch_sum():
    from svae_amd.lds.lds_inference import LDSEStepPlan, natural_lds_estep_general, reduce_stats
    n, T, B = 90, 5, 37
    rng = np.random.default_rng(11)
    natparam = rand_lds_natparam(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    plan = LDSEStepPlan(B, T, n, DEV)
    natural_lds_estep_general(_nat(natparam), tuple(_t(x) for x in node), plan=plan)
    Ei, Ep, lognorm = reduce_stats(plan)
    again = reduce_stats(plan)
    assert torch.equal(again[2], lognorm) and torch.equal(again[0][0], Ei[0])
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))
    assert close(Ei[0], plan.E_init[:, :n * n].sum(0).reshape(n, n))
    assert close(Ei[1], plan.E_init[:, n * n:].sum(0))
    for k in range(3):
        assert close(Ep[k], plan.E_pair[:, k].sum(0))
    assert close(lognorm, plan.lognorm.sum())
    assert Ei[2] == B and Ep[3] == B * (T - 1)


def test_xl_dense_node_potentials_match_oracle():
    n, T = 80, 4
    rng = np.random.default_rng(13)
    natparam = rand_lds_natparam(n, rng)
    Jd, h = rand_node_potentials((T, n), rng)
    M = rng.standard_normal((T, n, n)) * 0.05
    J = np.stack([np.diag(Jd[t]) - 0.5 * (M[t] @ M[t].T) for t in range(T)])
    from svae_amd.lds.lds_inference import natural_lds_estep_general
    got = natural_lds_estep_general(_nat(natparam), (_t(J), _t(h)))
    _check(got, lds_numpy.natural_lds_estep_general(natparam, (J, h)), 1e-7)


def test_xl_sampler_and_vjp_calls_raise_before_any_launch():
    from svae_amd.lds.lds_inference import (LDSEStepPlan, lds_inference_differentiable, natural_lds_inference_general,
                                            natural_lds_sample)
    from svae_amd.models import lds as lds_model
    n, T, B = 80, 4, 2
    rng = np.random.default_rng(17)
    natparam = rand_lds_natparam(n, rng)
    node = tuple(_t(x) for x in rand_node_potentials((B, T, n), rng))
    eps = torch.zeros(B, T, 1, n, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="64"):
        natural_lds_sample(_nat(natparam), node, 1)
    with pytest.raises(ValueError, match="64"):
        natural_lds_inference_general(_nat(natparam), node, num_samples=1)
    with pytest.raises(ValueError, match="64"):
        lds_inference_differentiable(_nat(natparam), node, eps=eps)
    with pytest.raises(ValueError, match="64"):
        lds_model.run_inference(None, None, node, 1)
    plan = LDSEStepPlan(B, T, n, DEV)
    plan.lognorm.fill_(float("nan"))
    init = tuple(_t(x) for x in natparam[0][:2]) + (_t([natparam[0][2]]),)
    pair = tuple(_t(x) for x in natparam[1][:3]) + (_t([natparam[1][3]]),)
    args = init + pair + node
    calls = [lambda: plan.launch(*args, half=1), lambda: plan.launch(*args, keep_factor=True),
             lambda: plan.launch(*args, keep_cross=True), lambda: plan.launch(*args, keep_sigma=True),
             lambda: plan.infer(*args), lambda: plan.sample(eps), lambda: plan.filter(*args),
             lambda: plan.vjp(plan.lognorm), lambda: plan.vjp_tail(1)]
    for call in calls:
        with pytest.raises(ValueError, match="64"):
            call()
    torch.cuda.synchronize()
    assert plan.epoch == 0 and bool(torch.isnan(plan.lognorm).all())
