"""GPU tests of the reverse sweeps of the per-step ragged LDS (LDSEStepPlan.infer_ragged_perstep(keep_vjp=True) + vjp();
svae_lds_ragged_perstep_inference_keep_f64, svae_lds_ragged_perstep_vjp_f64).  Inputs: the recipe of
tests/test_lds_ragged_perstep_hip.py (convex mixtures of K = 3 SLDS parameter sets per step, lengths holding 1, 2, T-1 and T
shuffled inside a wavefront).  Every sequence of the batch against its own cut sequence: forward outputs against
oracle/lds_numpy.py at 1e-8, g_node_J / g_node_h against fp64 CPU autograd through tests/_lds_large_torch.torch_estep
(pinned by tests/test_lds_ragged_perstep_vjp_cpu.py) at 1e-6 in the metric of tests/test_lds_ragged_hip.py, with random
cotangents of lognorm, dxx, ex, samples and -- once absent (the labelled SLDS path), once present -- of E_init and the
per-step E_pair.  Then: exact zeros beyond L, NaN in everything the contract calls unread, isolation, all lengths = T
against the uniform per-step infer() + vjp(), S = 20 (chunked) and the refusals."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _slds_ragged_numpy as sr  # noqa: E402

try:
    from threadpoolctl import threadpool_limits
except ImportError:
    import contextlib
    threadpool_limits = lambda limits: contextlib.nullcontext()


def _rel(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, float)
    b = np.asarray(b, float)
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300)) if b.size else 1.0
    return float(np.max(np.abs(a - b) / scale)) if b.size else 0.0


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, float)), dtype=torch.float64, device="cuda:0")


def _lengths(T, B, rng):
    """1, 2, T-1 and T first (as many as fit), the remainder drawn in [1, T]; then shuffled: mixed inside a wavefront"""
    must = list(dict.fromkeys([1, T, min(2, T), max(T - 1, 1)]))[:B]
    rest = rng.integers(1, T + 1, size=B - len(must)).tolist()
    L = np.array(must + rest, dtype=np.int64)
    return L[rng.permutation(B)]


# (n, T, B, pair_batched, init_batched, S): n = 1, 4, 9 the plain kernel, 10 its boundary, 11, 15 the low-register variant,
# 7 inside the range where the cross-moment store met the hazard rule; T = 17, 33 cross the 16- and 32-lane sums; B = 1, 5, 9:
# a partial wavefront and surplus rows
CASES = [(1, 17, 5, 0, 0, 1), (4, 3, 9, 1, 1, 5), (9, 33, 5, 1, 0, 0), (10, 17, 9, 1, 1, 1), (11, 2, 1, 0, 1, 1),
         (15, 17, 5, 1, 1, 5), (7, 17, 5, 1, 1, 1)]
STAT_KEYS = ("Ei", "Ep")


@functools.lru_cache(maxsize=None)
def _case(n, T, B, pb, ib, S, full=False):
    """inputs, cotangents and the per-sequence references of one batch (computed once, shared, left unchanged)"""
    with threadpool_limits(limits=1):
        return _case_body(n, T, B, pb, ib, S, full)


def _case_body(n, T, B, pb, ib, S, full):
    import _lds_large_torch as lt
    rng = np.random.default_rng(10000 * n + 100 * T + 10 * B + 2 * pb + ib + 7)
    init, pair = sr.mixed_lds_params(n, T, rng, lead=(B,))
    if not pb:
        pair = tuple(x[0] for x in pair)
    if not ib:
        init = tuple(x[0] for x in init)
    J, h = sr.slds_nodes(B, T, n, rng)
    node = (J, h, rng.standard_normal((B, T)))
    S1 = max(S, 1)
    eps = rng.standard_normal((B, T, S1, n))
    L = np.full(B, T, dtype=np.int64) if full else _lengths(T, B, rng)
    g = dict(ln=rng.standard_normal(B), dxx=rng.standard_normal((B, T, n)), x=rng.standard_normal((B, T, n)),
             s=rng.standard_normal((B, T, S1, n)), Ei=rng.standard_normal((B, n * n + n)),
             Ep=rng.standard_normal((B, T - 1, 3, n, n)))
    c64 = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x, float)), dtype=torch.float64)
    want = []
    for b in range(B):
        l = int(L[b])
        ini = tuple(x[b] for x in init) if ib else init
        pr = tuple(x[b] for x in pair) if pb else pair
        fwd = sr.cut_perstep_run(ini, pr, tuple(x[b] for x in node), l, eps[b] if S else None)
        params = (c64(ini[0]), c64(ini[1]), c64(ini[2]).reshape(1)) + tuple(c64(np.asarray(x)[:l - 1]) for x in pr)
        grads = {}
        for statc in (False, True):
            nJ = c64(node[0][b:b + 1, :l]).requires_grad_(True)
            nh = c64(node[1][b:b + 1, :l]).requires_grad_(True)
            ln, dxx, ex, smp, Ei, Ep = lt.torch_estep(params, nJ, nh, eps=c64(eps[b:b + 1, :l]) if S else None,
                                                      per_step_stats=True)
            loss = g["ln"][b] * ln.sum() + (c64(g["dxx"][b:b + 1, :l]) * dxx).sum() + (c64(g["x"][b:b + 1, :l]) * ex).sum()
            if S:
                loss = loss + (c64(g["s"][b:b + 1, :l]) * smp).sum()
            if statc:
                loss = loss + (c64(g["Ei"][b:b + 1]) * Ei).sum() + (c64(g["Ep"][b:b + 1, :l - 1]) * Ep).sum()
            loss.backward()
            grads[statc] = (nJ.grad[0].numpy(), nh.grad[0].numpy())
        want.append(dict(fwd=fwd, grads=grads))
    return dict(n=n, T=T, B=B, pb=pb, ib=ib, S=S, init=init, pair=pair, node=node, eps=eps, L=L, g=g, want=want)


def _inputs(c, nan_pad=False, L=None):
    """device tensors of the model, the noise and the cotangents; nan_pad: everything the contract calls unread is NaN"""
    L = c["L"] if L is None else L
    init = [np.array(x, dtype=float, copy=True) for x in c["init"]]
    init[2] = init[2].reshape(-1)
    pair = [np.array(x, dtype=float, copy=True) for x in c["pair"]]
    node = [np.array(x, dtype=float, copy=True) for x in c["node"]]
    eps = np.array(c["eps"], copy=True)
    g = {k: np.array(v, copy=True) for k, v in c["g"].items()}
    if nan_pad:
        for b in range(c["B"]):
            l = int(min(max(L[b], 1), c["T"]))
            for x in node:
                x[b, l:] = np.nan
            eps[b, l:] = np.nan
            for k in ("dxx", "x", "s"):
                g[k][b, l:] = np.nan
            g["Ep"][b, l - 1:] = np.nan          # blocks 0, 1 of pairs t >= l-1 and block 2 of pairs t-1 >= l-1
            if c["pb"]:
                for x in pair:
                    x[b, l - 1:] = np.nan
        if not c["pb"]:
            lmax = int(min(max(L.max(), 1), c["T"]))
            for x in pair:
                x[lmax - 1:] = np.nan
    return [_t(x) for x in init], [_t(x) for x in pair], [_t(x) for x in node], _t(eps), {k: _t(v) for k, v in g.items()}


def _run(c, statc, nan_pad=False, L=None, inputs=None, keep_vjp=True, backward=True):
    """infer_ragged_perstep(keep_vjp) [+ vjp()] -> forward outputs and gradients, cloned"""
    from svae_amd.lds.lds_inference import LDSEStepPlan
    L = c["L"] if L is None else L
    init, pair, node, eps, g = _inputs(c, nan_pad, L) if inputs is None else inputs
    plan = LDSEStepPlan(c["B"], c["T"], c["n"], "cuda:0", inhomog=True, pair_batched=bool(c["pb"]))
    samples = plan.infer_ragged_perstep(*init, *pair, *node, lengths=L, pair_batched=bool(c["pb"]), init_batched=bool(c["ib"]),
                                        eps=eps if c["S"] else None, keep_vjp=keep_vjp)
    out = dict(lognorm=plan.lognorm.clone(), E_init=plan.E_init.clone(), E_pair=plan.E_pair.clone(),
               dxx=plan.E_node_diagxx.clone(), ex=plan.E_node_x.clone(), samples=None if samples is None else samples.clone())
    if backward:
        smp_in = None
        if c["S"]:
            smp_in = samples.clone()
            if nan_pad:                       # samples[b, L:] are never read either
                for b in range(c["B"]):
                    smp_in[b, int(min(max(L[b], 1), c["T"])):] = float("nan")
        gJ, gh = plan.vjp(g["ln"], g["dxx"], g["x"], g["s"] if c["S"] else None, eps if c["S"] else None, smp_in,
                          g["Ei"] if statc else None, g["Ep"] if statc else None)
        out["gJ"], out["gh"] = gJ.clone(), gh.clone()
    torch.cuda.synchronize()
    return out, plan


def _check_forward(out, c):
    n = c["n"]
    for b in range(c["B"]):
        l = int(c["L"][b])
        ln, (Ei, Ep, En), smp = c["want"][b]["fwd"]
        pairs = [("lognorm", out["lognorm"][b], ln), ("E_init", out["E_init"][b, :n * n].reshape(n, n), Ei[0]),
                 ("E_init_x", out["E_init"][b, n * n:], Ei[1]), ("dxx", out["dxx"][b, :l], En[0]), ("ex", out["ex"][b, :l], En[1])]
        pairs += [("E_pair%d" % i, out["E_pair"][b, :l - 1, i], Ep[i]) for i in range(3)]
        if c["S"]:
            pairs.append(("samples", out["samples"][b, :l], smp))
        for name, a, w in pairs:
            r = _rel(a, w)
            assert r < 1e-8, (name, b, l, r)
        assert bool((out["E_pair"][b, l - 1:] == 0).all()) and bool((out["dxx"][b, l:] == 0).all())


def _check_grads(out, c, statc, bound=1e-6, rows=None):
    worst = {"g_node_J": 0.0, "g_node_h": 0.0}
    for b in (range(c["B"]) if rows is None else rows):
        l = int(c["L"][b])
        gJ, gh = c["want"][b]["grads"][statc]
        for name, a, w in (("g_node_J", out["gJ"][b, :l], gJ), ("g_node_h", out["gh"][b, :l], gh)):
            worst[name] = max(worst[name], _rel(a, w))
        for k in ("gJ", "gh"):
            assert bool(torch.isfinite(out[k][b]).all()), (k, b)
            assert bool((out[k][b, l:] == 0).all()), (k, b, l)            # exact zeros beyond L
    print("worst relative errors (statistics cotangents %s):" % ("present" if statc else "absent"),
          {k: "%.2e" % v for k, v in worst.items()})
    for name, v in worst.items():
        assert v < bound, (name, v)


@pytest.mark.parametrize("statc", [False, True])
@pytest.mark.parametrize("n,T,B,pb,ib,S", CASES)
def test_parity_every_sequence(n, T, B, pb, ib, S, statc):
    """forward outputs against the oracle on the cut sequence (1e-8) and the same bits as without keep_vjp; g_node_J and
    g_node_h on [:L] against CPU autograd on the cut sequence (1e-6), exactly 0 beyond L"""
    c = _case(n, T, B, pb, ib, S)
    assert B < 4 or {1, T, min(2, T), max(T - 1, 1)} <= set(c["L"].tolist())
    out, plan = _run(c, statc)
    plan.check_info()
    _check_forward(out, c)
    plain, _ = _run(c, statc, keep_vjp=False, backward=False)
    for k, v in plain.items():
        if v is not None:
            assert torch.equal(out[k], v), k
    _check_grads(out, c, statc)


@pytest.mark.parametrize("n,T,B,pb,ib,S", CASES)
def test_nan_in_everything_unread_changes_no_bit(n, T, B, pb, ib, S):
    """NaN in the node potentials, eps, samples and cotangents beyond each mask and in the pair parameters at t >= L-1:
    all gradients finite and bit-identical to the clean run's"""
    c = _case(n, T, B, pb, ib, S)
    clean, _ = _run(c, True)
    dirty, _ = _run(c, True, nan_pad=True)
    for k in ("gJ", "gh", "lognorm", "E_init", "E_pair", "dxx", "ex"):
        assert bool(torch.isfinite(dirty[k]).all()), k
        assert torch.equal(dirty[k], clean[k]), k
    clean0, _ = _run(c, False)
    dirty0, _ = _run(c, False, nan_pad=True)
    for k in ("gJ", "gh"):
        assert torch.equal(dirty0[k], clean0[k]), k


def test_isolation():
    """sequence 0's gradients are bit-identical when its neighbours' data change and when their lengths change"""
    c = _case(10, 17, 9, 1, 1, 1)
    base, _ = _run(c, True)
    init, pair, node, eps, g = _inputs(c)
    node[0][1:] *= 1.1
    node[1][1:] *= 1.25
    eps[1:] += 0.5
    init[1][1:] *= 0.9
    pair[1][1:] *= 0.9
    for k in g:
        g[k][1:] *= 1.5
    other_data, _ = _run(c, True, inputs=(init, pair, node, eps, g))
    L2 = c["L"].copy()
    L2[1:] = np.roll(L2[1:], 1)
    other_len, _ = _run(c, True, L=L2)
    for o in (other_data, other_len):
        for k in ("gJ", "gh", "lognorm", "E_pair"):
            assert torch.equal(o[k][0], base[k][0]), k
    assert not torch.equal(other_data["gJ"][1], base["gJ"][1])


@pytest.mark.parametrize("n,T,B,S", [(10, 17, 9, 1), (15, 17, 5, 5), (4, 3, 9, 0), (7, 17, 5, 1)])
def test_all_lengths_T_agree_with_the_uniform_per_step_sweeps(n, T, B, S):
    """lengths = T everywhere: within 1e-10 of the uniform per-step infer() + vjp(g_E_init, g_E_pair) on the same inputs
    (other kernels: not bit-equal; the bound of test_ragged_with_full_lengths_agrees_with_the_uniform_call)"""
    from svae_amd.lds.lds_inference import LDSEStepPlan
    c = _case(n, T, B, 1, 0, S, True)
    out, _ = _run(c, True)
    _check_grads(out, c, True)
    init, pair, node, eps, g = _inputs(c)
    plan = LDSEStepPlan(B, T, n, "cuda:0", inhomog=True, pair_batched=True)
    smp = plan.infer(*init, *pair, *node, pair_batched=True, eps=eps if S else None)
    gJ, gh = plan.vjp(g["ln"], g["dxx"], g["x"], g["s"] if S else None, eps if S else None, smp, g["Ei"], g["Ep"])
    torch.cuda.synchronize()
    plan.check_info()
    for name, a, w in (("g_node_J", out["gJ"], gJ), ("g_node_h", out["gh"], gh), ("E_pair", out["E_pair"], plan.E_pair)):
        r = _rel(a, w.cpu().numpy())
        print(name, "%.2e" % r)
        assert r < 1e-10, (name, r)


def test_twenty_samples_are_chunked():
    c = _case(4, 3, 9, 1, 1, 20)
    for statc in (False, True):
        out, _ = _run(c, statc)
        _check_forward(out, c)
        _check_grads(out, c, statc)


def test_refusals():
    c = _case(4, 3, 9, 1, 1, 5)
    out, plan = _run(c, True)
    g = _inputs(c)[4]
    with pytest.raises(ValueError):
        plan.vjp(g["ln"], param_out=True)
    with pytest.raises(ValueError):
        plan.vjp(g["ln"], dense_out=torch.empty(c["B"], c["T"], c["n"], c["n"], dtype=torch.float64, device="cuda:0"))
    with pytest.raises(RuntimeError):
        plan.sample(_t(c["eps"]))
    _, plain = _run(c, True, keep_vjp=False, backward=False)
    with pytest.raises(RuntimeError):
        plain.vjp(plain.lognorm)
