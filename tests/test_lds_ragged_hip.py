"""GPU tests of the variable-length LDS batch (`lengths=`; svae_lds_ragged_*): every sequence of a ragged batch against
the reference's own compiled code (oracle/_ref) run on the sequence truncated to its own length -- forward outputs,
samples under the reference's noise, gradients w.r.t. the node potentials -- with the metric and the bounds that
tests/test_lean_hip.py applies to the uniform kernels (1e-8 forward and samples, 1e-6 g_node_J / g_node_h, 1e-12
g_node_logZ); sequences of length 1, which the reference's compiled path does not take, against oracle/lds_numpy.py
(forward) and fp64 CPU autograd through tests/_lds_large_torch.torch_estep (gradients, 1e-6).  Then: padding is never
read, rows of a wavefront do not see each other's lengths, all-lengths-equal-T agrees with the uniform call, the model
layer, and the errors.

The ragged dispatcher has ONE route per call -- the packed one-directional kernels at every batch size -- so
"every route" is: records kept or not, n <= 10 or 11..15 (the low-register variant), the few-sample or the lane-per-sample
sampler, sweeps with or without sample cotangents; the options word selects nothing (checked bit for bit)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _lds_ragged_numpy as rn  # noqa: E402
from oracle import lds_numpy, ref  # noqa: E402  (checker only)

needs_ref = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")

try:        # the reference works on n x n blocks: a BLAS thread pool only costs there (1000 x, on a busy host)
    from threadpoolctl import threadpool_limits
except ImportError:
    import contextlib
    threadpool_limits = lambda limits: contextlib.nullcontext()


def _rel(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, float)
    b = np.asarray(b, float)
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale)) if b.size else 0.0


def _t(x):
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda:0")


def _lengths(T, B, rng):
    """1, 2, T-1 and T, the remainder drawn in [1, T]; B = 3 holds 1, T and 2 (four values do not fit)"""
    must = [1, T, min(2, T), max(T - 1, 1)][:B]
    rest = rng.integers(1, T + 1, size=B - len(must)).tolist()
    L = np.array(must + rest, dtype=np.int64)
    return L[rng.permutation(B)]


@functools.lru_cache(maxsize=None)
def _case(n, T, B, S, seed, model="rand", lengths=None):
    """inputs, cotangents and the per-sequence reference of one ragged batch (computed once, shared, left unchanged)"""
    with threadpool_limits(limits=1):
        return _case_body(n, T, B, S, seed, model, lengths)


def _case_body(n, T, B, S, seed, model, lengths):
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials, rotation_lds_natparam
    import _lds_large_torch as lt
    rng = np.random.default_rng(seed)
    init, pair = (rand_lds_natparam if model == "rand" else rotation_lds_natparam)(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    g = dict(ln=rng.standard_normal(B), dxx=rng.standard_normal((B, T, n)), x=rng.standard_normal((B, T, n)),
             s=rng.standard_normal((B, T, S, n)))
    L = _lengths(T, B, rng) if lengths is None else np.asarray(lengths, dtype=np.int64)
    eps = rng.standard_normal((B, T, S, n))
    want = []
    for b in range(B):
        l = int(L[b])
        nb = tuple(x[b, :l] for x in node)
        if l >= 2:
            ln, (oi, op, on) = ref.estep((init, pair), nb)
            smp, e = ref.sample_backward((init, pair), nb, S, seed=100 + b)
            (gJ0, gh0, gz0), _ = ref.estep_vjp((init, pair), nb, g["ln"][b], (g["dxx"][b, :l], g["x"][b, :l]), None)
            (gJ1, gh1, gz1), e1 = ref.estep_vjp((init, pair), nb, g["ln"][b], (g["dxx"][b, :l], g["x"][b, :l]),
                                                g["s"][b, :l], seed=100 + b)
            assert np.array_equal(e, e1)
            eps[b, :l] = e
        else:
            ln, (oi, op, on) = lds_numpy.natural_lds_estep_general((init, pair), nb)
            msgs, _ = lds_numpy.natural_filter_forward_general(init, pair, lds_numpy._canonical_node_params(nb))
            smp = lds_numpy.natural_sample_backward_general(msgs, pair, eps[b, :l])
            c = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64)
            params = (c(init[0]), c(init[1]), c(sum(init[2:])).reshape(1), c(pair[0]), c(pair[1]), c(pair[2]), c(pair[3]).reshape(1))
            grads = []
            for ws in (False, True):
                nJ, nh = c(nb[0])[None].requires_grad_(True), c(nb[1])[None].requires_grad_(True)
                lnt, dxx, ex, sm, _, _ = lt.torch_estep(params, nJ, nh, eps=c(eps[b:b + 1, :l]))
                loss = g["ln"][b] * lnt.sum() + (c(g["dxx"][b:b + 1, :l]) * dxx).sum() + (c(g["x"][b:b + 1, :l]) * ex).sum()
                if ws:
                    loss = loss + (c(g["s"][b:b + 1, :l]) * sm).sum()
                loss.backward()
                grads.append((nJ.grad[0].numpy(), nh.grad[0].numpy(), np.full(l, g["ln"][b])))
            (gJ0, gh0, gz0), (gJ1, gh1, gz1) = grads
        want.append(dict(ln=ln, Ei=oi, Ep=[np.asarray(x, float) if l >= 2 else np.zeros((n, n)) for x in op[:3]], En=on,
                         smp=np.asarray(smp), g0=(gJ0, gh0, gz0), g1=(gJ1, gh1, gz1)))
    return dict(init=init, pair=pair, node=node, g=g, L=L, eps=eps, want=want, n=n, T=T, B=B, S=S)


def _run(c, with_samples, lengths=None, node=None, eps=None, g=None, options=None, sample=True):
    """lds_inference_differentiable(lengths=) forward + backward on the case's inputs -> detached outputs and gradients"""
    from svae_amd.lds.lds_inference import LDSEStepPlan, lds_inference_differentiable
    n, T, B = c["n"], c["T"], c["B"]
    node = c["node"] if node is None else node
    eps = c["eps"] if eps is None else eps
    g = c["g"] if g is None else g
    L = c["L"] if lengths is None else lengths
    plan = LDSEStepPlan(B, T, n, "cuda:0", options=options)
    nJ, nh, nz = (_t(x).requires_grad_(True) for x in node)
    lognorm, (dxx, ex), samples, (E_init, E_pair) = lds_inference_differentiable(
        (tuple(_t(x) for x in c["init"]), tuple(_t(x) for x in c["pair"])), (nJ, nh, nz),
        eps=_t(eps) if sample else None, plan=plan, lengths=L)
    # one backward pass; the cotangents arrive through autograd as given (NaN ones at t >= L included)
    outs, cots = [lognorm, dxx, ex], [_t(g["ln"]), _t(g["dxx"]), _t(g["x"])]
    if with_samples:
        outs.append(samples)
        cots.append(_t(g["s"]))
    torch.autograd.backward(outs, cots)
    info = int(plan.info.item())
    out = dict(lognorm=lognorm, dxx=dxx, ex=ex, E_init=E_init, E_pair=E_pair, gJ=nJ.grad, gh=nh.grad, gz=nz.grad)
    if sample:
        out["samples"] = samples
    return {k: v.detach().clone() for k, v in out.items()}, info, plan


def _check(out, c, with_samples, sampled=None, rows=None):
    """every sequence against its truncated reference; everything at t >= L exactly 0"""
    n = c["n"]
    sampled = with_samples if sampled is None else sampled
    worst = {}

    def chk(name, a, b, bound):
        r = _rel(a, b)
        worst[name] = max(worst.get(name, 0.0), r)
        assert r < bound, (name, r)
    for b in (range(c["B"]) if rows is None else rows):
        l, w = int(c["L"][b]), c["want"][b]
        chk("lognorm", out["lognorm"][b], w["ln"], 1e-8)
        chk("E_init", out["E_init"][b, :n * n].reshape(n, n), w["Ei"][0], 1e-8)
        chk("E_init_x", out["E_init"][b, n * n:], w["Ei"][1], 1e-8)
        for i in range(3):
            chk("E_pair%d" % i, out["E_pair"][b, i], w["Ep"][i], 1e-8)
        chk("dxx", out["dxx"][b, :l], w["En"][0], 1e-8)
        chk("ex", out["ex"][b, :l], w["En"][1], 1e-8)
        if sampled:
            chk("samples", out["samples"][b, :l], w["smp"], 1e-8)
            assert bool((out["samples"][b, l:] == 0.0).all())
        gJ, gh, gz = w["g1"] if with_samples else w["g0"]
        chk("g_node_J", out["gJ"][b, :l], gJ, 1e-6)
        chk("g_node_h", out["gh"][b, :l], gh, 1e-6)
        chk("g_node_logZ", out["gz"][b, :l], gz, 1e-12)
        for k in ("dxx", "ex", "gJ", "gh", "gz"):
            assert bool((out[k][b, l:] == 0.0).all()), k
    print("worst relative errors:", {k: "%.2e" % v for k, v in worst.items()})


# seed rule of tests/test_lean_hip.py: 17 n + T; where that draw is so ill-conditioned that the parity bounds do not hold
# between the reference and the EXISTING uniform kernels on the truncated sequences either, the next seed.
# (15, 7): seed 262 draws a pair block J22 of condition 5.7e6 -- oracle/lds_numpy.py is then 1.8e-8 (E_init, E_pair) from
# the compiled reference in plain fp64 on the CPU, and the uniform kernels and the ragged ones alike miss 1e-8 there;
# seed 263 (condition 7e3) leaves 1e-11.
_NEXT_SEED = {(15, 7): 263}


def _seed(n, T):
    return _NEXT_SEED.get((n, T), 17 * n + T)


SHAPES =[(10, 12, 7), (4, 9, 5), (15, 7, 6), (11, 8, 5), (1, 6, 3), (10, 5, 9), (7, 40, 6)]


@needs_ref
@pytest.mark.parametrize("n,T,B", SHAPES + [(1, 6, 5)])      # ((1, 6, 3) cannot hold 1, 2, T-1 and T at once: (1, 6, 5) does)
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("with_samples", [False, True])
def test_ragged_parity_every_sequence(n, T, B, S, with_samples):
    c = _case(n, T, B, S, _seed(n, T))
    if B >= 4:
        assert {1, 2, T - 1, T} <= set(c["L"].tolist())
    out, info, _ = _run(c, with_samples, sample=with_samples)
    assert info == 0
    _check(out, c, with_samples)


@needs_ref
@pytest.mark.parametrize("with_samples", [False, True])
def test_ragged_parity_five_samples(with_samples):
    """S = 5: the lane-per-sample sampler; sampled in both runs, with and without sample cotangents"""
    n, T, B, S = 10, 12, 7, 5
    c = _case(n, T, B, S, _seed(n, T))
    out, info, _ = _run(c, with_samples)
    assert info == 0
    _check(out, c, with_samples, sampled=True)


@needs_ref
@pytest.mark.parametrize("n,T,B,S", [(10, 12, 7, 1), (11, 8, 5, 2), (10, 12, 7, 5)])
def test_ragged_forward_routes_without_records(n, T, B, S):
    """the E-step that keeps no record (natural_lds_estep_general) and the one that keeps the factor only
    (natural_lds_inference_general: E-step + sampler, no VJP record), n <= 10 and the low-register variant"""
    from svae_amd.lds.lds_inference import natural_lds_estep_general, natural_lds_inference_general, natural_lds_sample
    c = _case(n, T, B, S, _seed(n, T))
    natparam = (tuple(_t(x) for x in c["init"]), tuple(_t(x) for x in c["pair"]))
    node = tuple(_t(x) for x in c["node"])
    L = torch.as_tensor(c["L"], dtype=torch.int32, device="cuda:0")        # (a device tensor: used as it is)
    lognorm, (Ei, Ep, En) = natural_lds_estep_general(natparam, node, lengths=L, check=True)
    first = [x.clone() for x in (lognorm,) + tuple(Ei[:2]) + tuple(Ep) + tuple(En)]
    samples, (Ei2, Ep2, En2), lognorm2 = natural_lds_inference_general(natparam, node, num_samples=S, eps=_t(c["eps"]),
                                                                       lengths=c["L"])
    second = [x.clone() for x in (lognorm2,) + tuple(Ei2[:2]) + tuple(Ep2) + tuple(En2)]
    only = natural_lds_sample(natparam, node, S, eps=_t(c["eps"]), lengths=c["L"])
    assert torch.equal(only, samples)
    for b in range(B):
        l, w = int(c["L"][b]), c["want"][b]
        for ln, ei0, ei1, ep0, ep1, ep2, ep3, en0, en1, en2 in (first, second):
            assert _rel(ln[b], w["ln"]) < 1e-8
            assert _rel(ei0[b], w["Ei"][0]) < 1e-8 and _rel(ei1[b], w["Ei"][1]) < 1e-8
            for got, want in zip((ep0, ep1, ep2), w["Ep"]):
                assert _rel(got[b], want) < 1e-8
            assert float(ep3[b]) == l - 1
            assert _rel(en0[b, :l], w["En"][0]) < 1e-8 and _rel(en1[b, :l], w["En"][1]) < 1e-8
            assert bool((en0[b, l:] == 0).all()) and bool((en1[b, l:] == 0).all())
            assert bool((en2[b, :l] == 1).all()) and bool((en2[b, l:] == 0).all())
        assert _rel(samples[b, :l], w["smp"]) < 1e-8 and bool((samples[b, l:] == 0).all())


@needs_ref
def test_ragged_options_word_selects_nothing():
    """one route: every valid kernel-selection word gives the same bits"""
    from svae_amd import _lib
    n, T, B, S = 10, 12, 7, 2
    c = _case(n, T, B, S, _seed(n, T))
    base, _, _ = _run(c, True)
    for word in (_lib.OPT_LEAN_ON, _lib.OPT_TWOEND_OFF | _lib.OPT_LAYOUT_PACKED, _lib.OPT_LAYOUT_SPLIT | _lib.OPT_PRODUCERS_ON,
                 _lib.OPT_TWOEND_FULL | _lib.OPT_LEAN_OFF | _lib.OPT_PRODUCERS_OFF):
        out, info, _ = _run(c, True, options=word)
        assert info == 0
        for k in base:
            assert torch.equal(out[k], base[k]), (hex(word), k)


@needs_ref
def test_ragged_large_batch_default_dispatch():
    """B = 1030 (beyond every batch threshold of the uniform dispatcher), T = 12, n = 10, random lengths"""
    n, T, B, S = 10, 12, 1030, 1
    c = _case(n, T, B, S, _seed(n, T))
    out, info, _ = _run(c, True)
    assert info == 0
    _check(out, c, True)


@needs_ref
@pytest.mark.parametrize("n,T,B,S", [(10, 12, 7, 2), (15, 7, 6, 1), (10, 12, 7, 5)])
def test_ragged_padding_is_never_read(n, T, B, S):
    """NaN in node_*[b, L:], eps[b, L:] and the cotangents at t >= L: outputs and gradients there are 0, all others are
    bit-equal to the run with zeros there, info stays 0"""
    c = _case(n, T, B, S, _seed(n, T))
    pad = np.arange(T)[None, :] >= c["L"][:, None]

    def filled(x, v):
        x = np.array(x, dtype=float, copy=True)
        x[pad] = v
        return x
    runs = []
    for v in (0.0, np.nan):
        node = tuple(filled(x, v) for x in c["node"])
        g = dict(ln=c["g"]["ln"], dxx=filled(c["g"]["dxx"], v), x=filled(c["g"]["x"], v), s=filled(c["g"]["s"], v))
        out, info, _ = _run(c, True, node=node, eps=filled(c["eps"], v), g=g)
        assert info == 0
        runs.append(out)
    zero, nan = runs
    for k in zero:
        assert torch.equal(zero[k], nan[k]), k                 # (torch.equal is False for any NaN)
    padt = torch.as_tensor(pad, device="cuda:0")
    for k in ("dxx", "ex", "gJ", "gh", "gz", "samples"):
        assert bool((nan[k][padt] == 0.0).all()), k
    _check(nan, c, True)


@needs_ref
@pytest.mark.parametrize("n", [10, 13])
def test_ragged_rows_do_not_see_each_others_lengths(n):
    """the same batch twice with every length but lengths[b] changed: sequence b's outputs and gradients keep their
    bits -- b in each of the four DPP-row positions of a wavefront, and in the second wavefront"""
    T, B, S = 9, 8, 1
    c = _case(n, T, B, S, _seed(n, T))
    L0 = c["L"]
    base, _, _ = _run(c, True)
    rng = np.random.default_rng(4)
    for b in (0, 1, 2, 3, 5, 6):
        L1 = (L0 - 1 + rng.integers(1, T, size=B)) % T + 1          # every length changes, all stay in 1..T
        assert np.all(L1 != L0) and L1.min() >= 1 and L1.max() <= T
        L1[b] = L0[b]
        out, info, _ = _run(c, True, lengths=L1)
        assert info == 0
        for k in base:
            assert torch.equal(out[k][b], base[k][b]), (b, k)


@pytest.mark.parametrize("n,T,B,S", [(10, 12, 7, 2), (15, 7, 6, 1), (4, 1, 5, 1)])
def test_ragged_with_full_lengths_agrees_with_the_uniform_call(n, T, B, S):
    """all lengths = T on rotation_lds_natparam: within 1e-10 of the existing uniform call (other kernels: not bit-equal)"""
    from svae_amd.lds.lds_inference import lds_inference_differentiable
    from svae_amd.lds.synthetic_data import rand_node_potentials, rotation_lds_natparam
    rng = np.random.default_rng(17 * n + T)
    init, pair = rotation_lds_natparam(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    g = dict(ln=rng.standard_normal(B), dxx=rng.standard_normal((B, T, n)), x=rng.standard_normal((B, T, n)),
             s=rng.standard_normal((B, T, S, n)))
    eps = rng.standard_normal((B, T, S, n))
    natparam = (tuple(_t(x) for x in init), tuple(_t(x) for x in pair))

    def run(lengths):
        nJ, nh, nz = (_t(x).requires_grad_(True) for x in node)
        kw = {} if lengths is None else dict(lengths=lengths)
        lognorm, (dxx, ex), samples, (Ei, Ep) = lds_inference_differentiable(natparam, (nJ, nh, nz), eps=_t(eps), **kw)
        torch.autograd.backward([lognorm, dxx, ex, samples], [_t(g["ln"]), _t(g["dxx"]), _t(g["x"]), _t(g["s"])])
        return [x.detach().clone() for x in (lognorm, dxx, ex, samples, Ei, Ep, nJ.grad, nh.grad, nz.grad)]
    names = ["lognorm", "diagxx", "x", "samples", "E_init", "E_pair", "g_node_J", "g_node_h", "g_node_logZ"]
    for name, a, b in zip(names, run(np.full(B, T)), run(None)):
        r = _rel(a, b.cpu().numpy())
        print(name, "%.2e" % r)
        assert r < 1e-10, (name, r)


def _lds_globals(n, rng, scale=1.0):
    """A (NIW, MNIW) global natural parameter near svae/models/lds.py:57-67 (as tests/test_models_hip.py builds it)."""
    from oracle import expfam_numpy as ef
    nu, S, mu, kappa = n + 1. + rng.random(), 2. * scale * (n + 1) * np.eye(n), 0.1 * rng.standard_normal(n), 1. / (2. * scale * n)
    M = np.eye(n) * 0.9 + 0.05 * rng.standard_normal((n, n))
    K = 1. / (2. * scale * n) * np.eye(n)
    return ef.niw_standard_to_natural(S, mu, np.array(kappa), np.array(nu)), ef.mniw_standard_to_natural(nu, S, M, K)


def test_ragged_model_layer():
    """run_inference(..., lengths=) at (n, T, B) = (4, 9, 5): local_kl, the NIW statistics, the MNIW statistics and count
    are the sums of the per-sequence results of the model oracle on the truncated sequences (1e-8), with NaN in the
    padding; natural_gradient's d component uses sum (len - 1); run_inference_differentiable's gradient of local_kl
    matches the per-sequence reference VJPs (1e-6)."""
    from oracle import expfam_numpy as ef, models_numpy
    from svae_amd.lds.synthetic_data import rand_node_potentials
    from svae_amd.models.lds import natural_gradient, run_inference, run_inference_differentiable
    n, T, B, S = 4, 9, 5, 2
    rng = np.random.default_rng(n + T)
    prior, glob = _lds_globals(n, rng), _lds_globals(n, rng, scale=0.7)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    eps = rng.standard_normal((B, T, S, n))
    L = np.array([T, 1, 2, T - 1, 5])
    pad = np.arange(T)[None, :] >= L[:, None]
    node_nan = tuple(np.where(pad[..., None] if x.ndim == 3 else pad, np.nan, x) for x in node)
    eps_nan = np.where(pad[:, :, None, None], np.nan, eps)
    samples, stats, global_kl, local_kl = run_inference(prior, glob, node_nan, S, eps=eps_nan, lengths=L)
    want = [models_numpy.lds_run_inference(prior, glob, tuple(x[b, :L[b]] for x in node), eps[b, :L[b]]) for b in range(B)]
    niw_stats, mniw_stats = stats
    for b in range(B):
        assert _rel(samples[b, :L[b]], want[b][0]) < 1e-8 and bool((samples[b, L[b]:] == 0).all())
    assert _rel(niw_stats, sum(ef.pack_dense(w[1][0][0], w[1][0][1], np.array(1.), np.array(1.)) for w in want)) < 1e-8
    for i in range(3):
        assert _rel(mniw_stats[i], sum(np.asarray(w[1][1][i]) for w in want if np.ndim(w[1][1][i]) == 2)) < 1e-8
    assert float(mniw_stats[3]) == float(np.sum(L - 1)) and float(mniw_stats[3]) != B * (T - 1)
    assert float(local_kl) == pytest.approx(sum(w[3] for w in want), rel=1e-8)
    assert float(global_kl) == pytest.approx(want[0][2], rel=1e-8)
    # the natural gradient's MNIW count: -scale (prior_d + num_batches sum (len - 1) - global_d)
    nb, scale = 3.0, 0.5
    ng = natural_gradient(prior, glob, stats, nb, scale)
    d_want = -scale * (float(prior[1][3]) + nb * float(np.sum(L - 1)) - float(glob[1][3]))
    assert float(ng[1][3]) == pytest.approx(d_want, rel=1e-13)
    A_want = -scale * (np.asarray(prior[1][0]) + nb * mniw_stats[0].cpu().numpy() - np.asarray(glob[1][0]))
    assert _rel(ng[1][0], A_want) < 1e-12
    # gradient of local_kl w.r.t. the node potentials
    nJ, nh, nz = (_t(x).requires_grad_(True) for x in node_nan)
    _, _, _, kl = run_inference_differentiable(prior, glob, (nJ, nh, nz), S, eps=_t(eps_nan), lengths=L)
    assert float(kl) == pytest.approx(sum(w[3] for w in want), rel=1e-8)
    kl.backward()
    if not ref.available():
        pytest.skip("oracle/_ref not built: the forward half of this test passed, the gradient half needs the reference VJP")
    es = models_numpy.lds_prior_expectedstats(glob)
    natparam = (ef.unpack_dense(es[0]), es[1])
    for b in range(B):
        l = int(L[b])
        nb_ = tuple(x[b, :l] for x in node)
        if l >= 2:
            # d/dnode [<J, dxx> + <h, ex> + sum logZ - lognorm] = (dxx, ex, 1) + VJP(g_dxx = J, g_x = h, g_lognorm = -1)
            (gJ, gh, gz), _ = ref.estep_vjp(natparam, nb_, -1.0, (nb_[0], nb_[1]), None)
            _, (_, _, on) = ref.estep(natparam, nb_)
            assert _rel(nJ.grad[b, :l], gJ + on[0]) < 1e-6 and _rel(nh.grad[b, :l], gh + on[1]) < 1e-6
            assert _rel(nz.grad[b, :l], gz + 1.0) < 1e-12
        for gr in (nJ.grad, nh.grad, nz.grad):
            assert bool((gr[b, l:] == 0).all()) and bool(torch.isfinite(gr[b]).all())


def test_ragged_errors_come_before_any_launch():
    """every limit of the ragged kernels is a ValueError raised before a launch (plan.epoch unchanged); a length of 0 or
    T + 1 is device data: it raises the status word, check=True reports it, nothing faults"""
    from svae_amd.lds.lds_inference import (LDSEStepPlan, lds_inference_differentiable, natural_lds_estep_general,
                                            natural_lds_inference_general, natural_lds_sample)
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    from svae_amd.models.lds import run_inference
    rng = np.random.default_rng(0)
    n, T, B = 4, 6, 3
    init, pair = rand_lds_natparam(n, rng)
    natparam = (tuple(_t(x) for x in init), tuple(_t(x) for x in pair))
    node = tuple(_t(x) for x in rand_node_potentials((B, T, n), rng))
    L = np.array([6, 1, 3])
    plan = LDSEStepPlan(B, T, n, "cuda:0")
    calls = (lambda np_, nd, **kw: natural_lds_estep_general(np_, nd, **kw),
             lambda np_, nd, **kw: natural_lds_sample(np_, nd, 1, **kw),
             lambda np_, nd, **kw: natural_lds_inference_general(np_, nd, num_samples=1, **kw),
             lambda np_, nd, **kw: lds_inference_differentiable(np_, nd, **kw))
    per_step = (natparam[0], tuple(x.expand(T - 1, n, n).contiguous() for x in natparam[1][:3]) + (natparam[1][3].expand(T - 1).contiguous(),))
    per_seq = (natparam[0], tuple(x.expand(B, T - 1, n, n).contiguous() for x in natparam[1][:3])
               + (natparam[1][3].expand(B, T - 1).contiguous(),))
    dense = (torch.diag_embed(node[0]), node[1])
    for call in calls:
        with pytest.raises(ValueError, match="15"):                        # n > 15
            n2 = 16
            i2, p2 = rand_lds_natparam(n2, rng)
            call((tuple(_t(x) for x in i2), tuple(_t(x) for x in p2)), tuple(_t(x) for x in rand_node_potentials((B, T, n2), rng)),
                 lengths=L)
        for bad_np in (per_step, per_seq):
            with pytest.raises(ValueError, match="pair parameters"):
                call(bad_np, node, lengths=L)
        with pytest.raises(ValueError, match="dense"):
            call(natparam, dense, lengths=L)
        with pytest.raises(ValueError, match=r"\(B,T,n\)"):               # unbatched nodes
            call(natparam, tuple(x[0] for x in node), lengths=L[:1])
        for bad_L in (L[:2], np.zeros((B, 1), dtype=int), 3):
            with pytest.raises(ValueError, match="shape"):
                call(natparam, node, lengths=bad_L, plan=plan)
    with pytest.raises(ValueError, match="natparam_grad"):
        lds_inference_differentiable(natparam, node, lengths=L, natparam_grad=True, plan=None)
    with pytest.raises(ValueError, match="pair_stats_grad"):
        lds_inference_differentiable(natparam, node, lengths=L, pair_stats_grad=True)
    with pytest.raises(ValueError, match="shape"):
        plan.launch(*([None] * 9), lengths=L[:2])
    with pytest.raises(ValueError, match="pair parameters"):
        LDSEStepPlan(B, T, n, "cuda:0", inhomog=True).launch(*([None] * 9), lengths=L)
    gp = _lds_globals(n, rng)
    with pytest.raises(ValueError, match="15"):
        run_inference(_lds_globals(16, rng), _lds_globals(16, rng), rand_node_potentials((B, T, 16), rng), 1, lengths=L)
    with pytest.raises(ValueError, match="shape"):
        run_inference(gp, gp, tuple(x.cpu().numpy() for x in node), 1, lengths=L[:2])
    assert plan.epoch == 0
    # device data: a length outside 1..T
    for bad in (0, T + 1):
        Lb = L.copy()
        Lb[1] = bad
        natural_lds_estep_general(natparam, node, plan=plan, lengths=Lb)       # silent, like the reference
        with pytest.raises(FloatingPointError):
            plan.check_info()
        with pytest.raises(FloatingPointError):
            natural_lds_estep_general(natparam, node, plan=plan, lengths=Lb, check=True)
        # sampler and sweeps clamp the same way: the whole training pass runs, the status word is raised
        nJ, nh = node[0].clone().requires_grad_(True), node[1].clone().requires_grad_(True)
        lognorm, (dxx, ex), samples, _ = lds_inference_differentiable(natparam, (nJ, nh), eps=_t(rng.standard_normal((B, T, 1, n))),
                                                                      plan=plan, lengths=Lb)
        (lognorm.sum() + dxx.sum() + ex.sum() + samples.sum()).backward()
        torch.cuda.synchronize()
        with pytest.raises(FloatingPointError):
            plan.check_info()
        ok = [b for b in range(B) if b != 1]
        assert bool(torch.isfinite(nJ.grad[ok]).all()) and bool(torch.isfinite(lognorm[ok]).all())
    lognorm, _ = natural_lds_estep_general(natparam, node, plan=plan, lengths=L, check=True)      # the device is fine
    assert bool(torch.isfinite(lognorm).all())
    # the plan remembers what its records are: a uniform launch ends the ragged state, vjp(lengths=) then refuses
    natural_lds_estep_general(natparam, node, plan=plan)
    assert plan._lengths is None
    with pytest.raises(ValueError, match="no per-sequence lengths"):
        plan.vjp(torch.zeros(B, dtype=torch.float64, device="cuda:0"), lengths=L)
