"""GPU tests of the packed LDS E-step with PER-STEP pair parameters and per-sequence lengths (svae_lds_ragged_perstep_*;
LDSEStepPlan.launch_ragged_perstep / infer_ragged_perstep): every sequence of a ragged batch against oracle/lds_numpy.py
run on the sequence cut at its own length, the init potential passed whole -- the metric and the bound of
tests/test_lds_ragged_hip.py (1e-8), exact zeros beyond the length.  Then: padding (NaN) is never read, rows of a wavefront
do not see each other, a length outside 1..T raises the status word, and the uniform per-step kernel is where it was.

Inputs: per-step pair parameters and init potentials that are convex mixtures (Dirichlet weights per step) of K = 3
parameter sets of the SLDS test recipe -- the SLDS's own use of this kernel."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _slds_ragged_numpy as sr  # noqa: E402


def _rel(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, float)
    b = np.asarray(b, float)
    if not b.size:
        return 0.0
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale))


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, float)), dtype=torch.float64, device="cuda:0")


def _lengths(T, B, rng):
    """1, 2, T-1 and T first (as many as fit), the remainder drawn in [1, T]; then shuffled: mixed inside a wavefront"""
    must = list(dict.fromkeys([1, T, min(2, T), max(T - 1, 1)]))[:B]
    rest = rng.integers(1, T + 1, size=B - len(must)).tolist()
    L = np.array(must + rest, dtype=np.int64)
    return L[rng.permutation(B)]


# (n, T, B, pair_batched, init_batched, S): n = 1, 4, 9 the plain kernel, 10 its boundary, 11, 15 the low-register variant;
# T = 17, 33: the lane-strided log-normaliser sums cross 16 and 32; B = 1, 5, 9: a partial wavefront and surplus rows
CASES = [(1, 17, 5, 0, 0, 1), (4, 3, 9, 1, 1, 5), (9, 33, 5, 1, 0, 0), (10, 17, 9, 1, 1, 1), (11, 2, 1, 0, 1, 1),
         (15, 17, 5, 1, 1, 5), (11, 33, 5, 1, 1, 1), (10, 3, 5, 0, 0, 0)]


@functools.lru_cache(maxsize=None)
def _case(n, T, B, pb, ib, S, full=False):
    """inputs and the per-sequence reference of one batch (computed once, shared, left unchanged)"""
    rng = np.random.default_rng(10000 * n + 100 * T + 10 * B + 2 * pb + ib)
    init, pair = sr.mixed_lds_params(n, T, rng, lead=(B,))
    if not pb:
        pair = tuple(x[0] for x in pair)
    if not ib:
        init = tuple(x[0] for x in init)
    J, h = sr.slds_nodes(B, T, n, rng)
    node = (J, h, rng.standard_normal((B, T)))
    eps = rng.standard_normal((B, T, max(S, 1), n))
    L = np.full(B, T, dtype=np.int64) if full else _lengths(T, B, rng)
    want = []
    for b in range(B):
        ini = tuple(x[b] for x in init) if ib else init
        pr = tuple(x[b] for x in pair) if pb else pair
        want.append(sr.cut_perstep_run(ini, pr, tuple(x[b] for x in node), int(L[b]), eps[b] if S else None))
    return dict(n=n, T=T, B=B, pb=pb, ib=ib, S=S, init=init, pair=pair, node=node, eps=eps, L=L, want=want)


def _inputs(c, nan_pad=False, L=None):
    """device tensors; nan_pad: everything the contract calls unread is NaN"""
    L = c["L"] if L is None else L
    init = [np.array(x, dtype=float, copy=True) for x in c["init"]]
    init[2] = init[2].reshape(-1)                       # (B,) per sequence, (1,) shared
    pair = [np.array(x, dtype=float, copy=True) for x in c["pair"]]
    node = [np.array(x, dtype=float, copy=True) for x in c["node"]]
    eps = np.array(c["eps"], copy=True)
    if nan_pad:
        for b in range(c["B"]):
            l = int(min(max(L[b], 1), c["T"]))
            for x in node:
                x[b, l:] = np.nan
            eps[b, l:] = np.nan
            if c["pb"]:
                for x in pair:
                    x[b, l - 1:] = np.nan
        if not c["pb"]:
            lmax = int(min(max(L.max(), 1), c["T"]))
            for x in pair:
                x[lmax - 1:] = np.nan
    return [_t(x) for x in init], [_t(x) for x in pair], [_t(x) for x in node], _t(eps)


def _run(c, nan_pad=False, L=None, plan=None, inputs=None):
    from svae_amd.lds.lds_inference import LDSEStepPlan
    L = c["L"] if L is None else L
    init, pair, node, eps = _inputs(c, nan_pad, L) if inputs is None else inputs
    plan = plan or LDSEStepPlan(c["B"], c["T"], c["n"], "cuda:0", inhomog=True, pair_batched=bool(c["pb"]))
    kw = dict(lengths=L, pair_batched=bool(c["pb"]), init_batched=bool(c["ib"]))
    if c["S"]:
        samples = plan.infer_ragged_perstep(*init, *pair, *node, eps=eps, **kw)
    else:
        plan.launch_ragged_perstep(*init, *pair, *node, **kw)
        samples = None
    torch.cuda.synchronize()
    out = dict(lognorm=plan.lognorm.clone(), E_init=plan.E_init.clone(), E_pair=plan.E_pair.clone(),
               dxx=plan.E_node_diagxx.clone(), ex=plan.E_node_x.clone(), samples=None if samples is None else samples.clone())
    return out, plan


def _check(out, c, rows=None, L=None):
    n, T = c["n"], c["T"]
    L = c["L"] if L is None else L
    worst = {}
    for b in (range(c["B"]) if rows is None else rows):
        l = int(L[b])
        ln, (Ei, Ep, En), smp = c["want"][b]

        def chk(name, a, w):
            r = _rel(a, w)
            worst[name] = max(worst.get(name, 0.0), r)
            assert bool(torch.isfinite(a).all()), (name, b)
            assert r < 1e-8, (name, b, l, r)
        chk("lognorm", out["lognorm"][b], ln)
        chk("E_init", out["E_init"][b, :n * n].reshape(n, n), Ei[0])
        chk("E_init_x", out["E_init"][b, n * n:], Ei[1])
        for i in range(3):
            chk("E_pair%d" % i, out["E_pair"][b, :l - 1, i], Ep[i])
        chk("dxx", out["dxx"][b, :l], En[0])
        chk("ex", out["ex"][b, :l], En[1])
        assert bool((out["E_pair"][b, l - 1:] == 0).all()), b
        assert bool((out["dxx"][b, l:] == 0).all()) and bool((out["ex"][b, l:] == 0).all()), b
        if c["S"]:
            chk("samples", out["samples"][b, :l], smp)
            assert bool((out["samples"][b, l:] == 0).all()), b
    print("worst relative errors:", {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("nan_pad", [False, True])
@pytest.mark.parametrize("n,T,B,pb,ib,S", CASES)
def test_perstep_ragged_parity_every_sequence(n, T, B, pb, ib, S, nan_pad):
    """nan_pad: node potentials and eps at t >= L are NaN, and the pair parameters at t >= L-1 (per sequence with
    pair_batched; past the longest sequence otherwise): every output is still finite and right"""
    c = _case(n, T, B, pb, ib, S)
    assert B < 4 or {1, T, min(2, T), max(T - 1, 1)} <= set(c["L"].tolist())
    out, plan = _run(c, nan_pad)
    plan.check_info()
    _check(out, c)
    # the plan knows its records are ragged ones: the uniform sampler and the sweeps refuse
    with pytest.raises(RuntimeError):
        plan.sample(_t(c["eps"]))
    with pytest.raises(RuntimeError):
        plan.vjp(plan.lognorm)


def test_perstep_ragged_isolation_and_determinism():
    """sequence 0's outputs are bit-identical when its neighbours' data change, when their lengths change, and on a
    second run"""
    c = _case(10, 17, 5, 1, 1, 1)
    base, plan = _run(c)
    again, _ = _run(c, plan=plan)
    init, pair, node, eps = _inputs(c)
    node[0][1:] *= 1.1                                  # the neighbours' data: node potentials, noise, init potential, logZ
    node[1][1:] *= 1.25
    node[2][1:] += 0.5
    eps[1:] += 0.5
    init[1][1:] *= 0.9
    pair[3][1:] += 0.3
    other_data, _ = _run(c, inputs=(init, pair, node, eps))
    L2 = c["L"].copy()
    L2[1:] = np.roll(L2[1:], 1)
    L2[0] = c["L"][0]
    other_len, _ = _run(c, L=L2)
    for o in (again, other_data, other_len):
        for k in ("lognorm", "E_init", "E_pair", "dxx", "ex", "samples"):
            assert torch.equal(o[k][0], base[k][0]), k
    for k in ("lognorm", "E_init", "E_pair", "dxx", "ex", "samples"):
        assert torch.equal(again[k], base[k]), k


@pytest.mark.parametrize("bad", ["zero", "T+1"])
def test_perstep_ragged_length_outside_the_range_raises_the_status_word(bad):
    c = _case(4, 3, 9, 1, 1, 5)
    L = c["L"].copy()
    L[2] = 0 if bad == "zero" else c["T"] + 1
    out, plan = _run(c, L=L)
    with pytest.raises(FloatingPointError):
        plan.check_info()
    plan.check_info()                                   # (read and cleared)
    ok = [b for b in range(c["B"]) if b != 2]
    _check(out, c, rows=ok)
    out, plan = _run(c, plan=plan)
    plan.check_info()


@pytest.mark.parametrize("n,T,B,S", [(10, 17, 9, 1), (15, 17, 5, 5), (4, 3, 9, 0)])
def test_full_lengths_agree_with_the_uniform_per_step_kernel(n, T, B, S):
    """lengths = T everywhere: the ragged route against the plain `launch` of an inhomogeneous plan (the uniform kernel,
    which this feature must leave alone) at 1e-12; the uniform call itself against the oracle at 1e-8"""
    from svae_amd.lds.lds_inference import LDSEStepPlan
    c = _case(n, T, B, 1, 0, S, True)
    out, _ = _run(c)
    _check(out, c)
    init, pair, node, eps = _inputs(c)
    plan = LDSEStepPlan(B, T, n, "cuda:0", inhomog=True, pair_batched=True)
    plan.launch(*init, *pair, *node, pair_batched=True, keep_factor=bool(S))
    smp = plan.sample(eps) if S else None
    torch.cuda.synchronize()
    plan.check_info()
    uni = dict(lognorm=plan.lognorm, E_init=plan.E_init, E_pair=plan.E_pair, dxx=plan.E_node_diagxx, ex=plan.E_node_x,
               samples=smp)
    _check(uni, c)
    for k, v in uni.items():
        if v is not None:
            r = _rel(out[k], v.cpu().numpy())
            assert r < 1e-12, (k, r)


def test_perstep_ragged_errors_come_before_any_launch():
    from svae_amd.lds.lds_inference import LDSEStepPlan
    c = _case(4, 3, 9, 1, 1, 5)
    init, pair, node, eps = _inputs(c)
    B, T, n = c["B"], c["T"], c["n"]
    kw = dict(lengths=c["L"], pair_batched=True, init_batched=True)
    homog = LDSEStepPlan(B, T, n, "cuda:0")
    with pytest.raises(ValueError, match="inhomog"):
        homog.launch_ragged_perstep(*init, *pair, *node, **kw)
    plan = LDSEStepPlan(B, T, n, "cuda:0", inhomog=True, pair_batched=True)
    with pytest.raises(ValueError, match="lengths"):
        plan.launch_ragged_perstep(*init, *pair, *node, pair_batched=True, init_batched=True)
    with pytest.raises(ValueError, match="shape"):
        plan.launch_ragged_perstep(*init, *pair, *node, **dict(kw, lengths=c["L"][:2]))
    with pytest.raises(ValueError, match="integer"):
        plan.launch_ragged_perstep(*init, *pair, *node, **dict(kw, lengths=c["L"].astype(float)))
    with pytest.raises(ValueError, match="J11"):
        plan.launch_ragged_perstep(*init, *pair, *node, **dict(kw, pair_batched=False))
    with pytest.raises(ValueError, match="init_J"):
        plan.infer_ragged_perstep(*init, *pair, *node, eps=eps, **dict(kw, init_batched=False))
    with pytest.raises(ValueError, match="eps"):
        plan.infer_ragged_perstep(*init, *pair, *node, eps=eps[:, :, :, :2], **kw)
    with pytest.raises(ValueError, match="pair parameters"):          # the existing refusal stays
        plan.launch(*([None] * 9), lengths=c["L"])
    assert plan.epoch == 0 and homog.epoch == 0
