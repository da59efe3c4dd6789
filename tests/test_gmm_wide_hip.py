"""The GMM local step for latent dimensions 9 <= N <= 16 (svae_amd/csrc/gmm_wide.hip, svae_gmm_wide_*): goldens from
the reference itself (tests/golden/make_golden_gmm_wide.py), the NumPy oracle, the N <= 8 kernels on the same inputs,
torch autograd for the sampler and the local VJP, the torch global maps, and the model-level entry points.  The
CPU tests at the top check the host-side argument checks, the ISA (no scratch, no DPP hazard) and the goldens."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import expfam_numpy as ef, gmm_numpy  # noqa: E402  (checker only)

WIDE_GOLDEN = ["gmm_K15_N10_T100", "gmm_K33_N16_T24"]
DEV = "cuda:0"


def _np(x):
    return x.detach().cpu().numpy()


def _t(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float64, device=DEV)


# ---- CPU ----------------------------------------------------------------------------------------------------------

def _lib_or_skip():
    from svae_amd import _lib
    return _lib.load()


def test_wide_entries_check_their_arguments_on_the_host():
    """Same code as the N <= 8 counterpart for the same bad argument; N outside 1..16 gets the counterpart's N > 8 code.
    Every call returns before any HIP call (null stream, no device)."""
    lib = _lib_or_skip()
    one = 8                      # a non-null pointer value that is never dereferenced
    ws = lib.svae_gmm_wide_mw_workspace_bytes(100, 16, 64, 10)
    assert ws > 0 and lib.svae_gmm_wide_mw_workspace_bytes(100, 17, 64, 10) == 0
    assert lib.svae_gmm_wide_mw_workspace_bytes(100, 16, 65, 10) == 0
    assert lib.svae_gmm_wide_mw_workspace_bytes(100, 0, 5, 10) == 0
    for N in (0, 17):
        assert lib.svae_gmm_wide_mw_begin(10, N, 5, 10, one, 1 << 30, None) == lib.svae_gmm_mw_begin(10, 9, 5, 10, one, 1 << 30, None) == -2
    assert lib.svae_gmm_wide_mw_begin(10, 12, 65, 10, one, 1 << 30, None) == -3
    assert lib.svae_gmm_wide_mw_begin(10, 12, 5, 10, None, 1 << 30, None) == -5
    assert lib.svae_gmm_wide_mw_begin(10, 12, 5, 10, one, 16, None) == -5           # short workspace

    def step(phase=0, sweep=0, T=10, N=12, K=5, ptrs=None, ws_bytes=1 << 30, fn=lib.svae_gmm_wide_mw_step_f64):
        p = [one] * 16 if ptrs is None else ptrs
        return fn(phase, sweep, T, N, K, *p[:5], 1e-3, 10, *p[5:16], one, ws_bytes, None)
    for N in (0, 17):
        assert step(N=N) == step(N=9, fn=lib.svae_gmm_mw_step_f64) == -4
    assert step(K=65) == -5
    assert step(phase=3) == -1 and step(sweep=10) == -2
    nul = [one] * 16
    nul[0] = None
    assert step(ptrs=nul) == -6                                                     # label_global
    nul = [one] * 16
    nul[15] = None
    assert step(ptrs=nul) == -23                                                    # info
    assert step(ws_bytes=64) == -24

    for N in (0, 17):
        assert lib.svae_gmm_wide_sample_f64(4, N, 1, one, one, one, None) == lib.svae_gmm_sample_f64(4, 9, 1, one, one, one, None) == -2
        assert lib.svae_gmm_wide_local_vjp_f64(4, N, 5, 1, one, one, one, one, one, one, None, None, None, one, one, None) == -2
        assert lib.svae_gmm_wide_global_step_f64(5, N, one, one, None, None, one, one, None, one, None) == \
            lib.svae_gmm_global_step_f64(5, 9, one, one, None, None, one, one, None, one, None) == -2
    assert lib.svae_gmm_wide_sample_f64(4, 12, 1, None, one, one, None) == -4
    assert lib.svae_gmm_wide_local_vjp_f64(4, 12, 65, 1, one, one, one, one, one, one, None, None, None, one, one, None) == -3
    assert lib.svae_gmm_wide_local_vjp_f64(4, 12, 5, 1, None, one, one, one, one, one, None, None, None, one, one, None) == -5
    assert lib.svae_gmm_wide_local_vjp_f64(4, 12, 5, 1, one, one, one, one, one, one, None, None, one, one, one, None) == -12
    assert lib.svae_gmm_wide_global_step_f64(65, 12, one, one, None, None, one, one, None, one, None) == -1
    assert lib.svae_gmm_wide_global_step_f64(5, 12, one, one, None, None, one, one, one, one, None) == -5
    assert lib.svae_gmm_wide_global_step_f64(5, 12, one, one, None, None, one, one, None, None, None) == -10


def test_wide_unit_compiles_without_scratch_and_without_dpp_hazards(tmp_path):
    import audit_dpp_hazards
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "gmm_wide.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "svae_amd/csrc/gmm_wide.hip"), "-o", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    txt = out.read_text()
    assert "scratch_" not in txt
    n, problems = audit_dpp_hazards.audit(str(out))
    assert n > 0 and problems == [], problems[:5]


@pytest.mark.parametrize("case", WIDE_GOLDEN)
def test_wide_goldens_agree_with_the_numpy_oracle(case, golden_dir):
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    (ls, gs), (ds, ns), (ln, gn), kl, _ = gmm_numpy.local_meanfield(
        g["label_global"], g["gaussian_globals"], (g["node_J"], g["node_h"]), g["label_init"])
    assert np.array_equal(ls.argmax(1), g["label_stats"].argmax(1))
    for got, key in ((ls, "label_stats"), (gs, "gaussian_stats"), (ns, "niw_stats"), (gn, "gaussian_natparam")):
        np.testing.assert_allclose(got, g[key], rtol=1e-9, atol=1e-10, err_msg=key)
    assert kl == pytest.approx(float(g["kl"]), rel=1e-10)


# ---- GPU ----------------------------------------------------------------------------------------------------------

def _problem(T, N, K, seed):
    from svae_amd.lds.synthetic_data import rand_node_potentials
    rng = np.random.default_rng(seed)
    niw = np.stack([ef.niw_standard_to_natural((N + 10.) * np.eye(N), 2 * rng.standard_normal(N), np.array(10.),
                                               np.array(N + 10.)) for _ in range(K)])
    lg, gg = ef.dirichlet_expectedstats(rng.random(K) + 0.5), ef.niw_expectedstats(niw)
    node = rand_node_potentials((T, N), rng)
    init = rng.random((T, K))
    init /= init.sum(-1, keepdims=True)
    return lg, gg, node, init


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_GOLDEN)
def test_wide_golden_local_meanfield(case, golden_dir):
    from svae_amd.models.gmm import local_meanfield
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    (ls, gs), (ds, ns), (ln, gn), kl = local_meanfield(
        (g["dirichlet_natparam"], g["niw_natparam"]), (g["node_J"], g["node_h"]), label_init=g["label_init"])
    assert np.array_equal(_np(ls).argmax(1), g["label_stats"].argmax(1))
    for got, key in ((ls, "label_stats"), (gs, "gaussian_stats"), (ds, "dirichlet_stats"),
                     (ns, "niw_stats"), (ln, "label_natparam"), (gn, "gaussian_natparam")):
        np.testing.assert_allclose(_np(got), g[key], rtol=1e-9, atol=1e-10, err_msg=key)
    assert float(kl) == pytest.approx(float(g["kl"]), rel=1e-10)


@pytest.mark.gpu
def test_wide_golden_run_inference(golden_dir):
    from svae_amd.models import gmm
    g = np.load(os.path.join(golden_dir, "gmm_run_K6_N16_T40.npz"))
    samples, (ds, ns), gkl, lkl = gmm.run_inference(
        (_t(g["prior_dir"]), _t(g["prior_niw"])), (_t(g["glob_dir"]), _t(g["glob_niw"])),
        (_t(g["node_J"]), _t(g["node_h"])), g["eps"].shape[1], label_init=_t(g["label_init"]), eps=_t(g["eps"]))
    np.testing.assert_allclose(_np(samples), g["samples"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(ds), g["dirichlet_stats"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(ns), g["niw_stats"], rtol=1e-9, atol=1e-10)
    assert float(gkl) == pytest.approx(float(g["global_kl"]), rel=1e-10)
    assert float(lkl) == pytest.approx(float(g["local_kl"]), rel=1e-10)


_ORACLE = [(1, 9, 5), (3, 10, 15), (257, 12, 33), (1000, 15, 64), (100, 16, 1), (64, 16, 64), (9000, 10, 5),
           (257, 9, 15), (1000, 16, 15)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,K", _ORACLE)
def test_wide_against_oracle(T, N, K):
    from svae_amd.models.gmm import meanfield_from_globals
    lg, gg, node, init = _problem(T, N, K, T + N + K)
    o = meanfield_from_globals(lg, gg, node, init)
    assert o["path"] == "wide_sweeps"
    (ls, gs), (ds, ns), (ln, gn), kl, iters = gmm_numpy.local_meanfield(lg, gg, node, init)
    assert int(o["iters"].item()) == iters
    assert np.array_equal(_np(o["assign"]), ls.argmax(1))
    assert np.array_equal(_np(o["label_stats"]).argmax(1), ls.argmax(1))
    np.testing.assert_allclose(_np(o["label_stats"]), ls, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(_np(o["gaussian_stats"]), gs, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(_np(o["niw_stats"]), ns, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(_np(o["dirichlet_stats"]), ds, rtol=1e-10)
    np.testing.assert_allclose(_np(o["gaussian_natparam"]), gn, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(_np(o["label_natparam"]), ln, rtol=1e-9, atol=1e-9)
    assert float(o["kl"].item()) == pytest.approx(kl, rel=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,K", [(500, 1, 5), (300, 2, 15), (257, 5, 33), (100, 8, 64), (1000, 8, 3)])
def test_wide_kernels_match_the_n8_kernels(T, N, K):
    from svae_amd.models.gmm import meanfield_from_globals
    lg, gg, node, init = _problem(T, N, K, 7 * T + N + K)
    a = meanfield_from_globals(lg, gg, node, init, multi_wg=True, persistent=False)
    b = meanfield_from_globals(lg, gg, node, init, wide=True)
    assert (a["path"], b["path"]) == ("sweeps", "wide_sweeps")
    assert int(a["iters"].item()) == int(b["iters"].item())
    assert torch.equal(a["assign"], b["assign"])
    for k in ("label_stats", "label_fixed", "gaussian_stats", "label_natparam", "gaussian_natparam",
              "dirichlet_stats", "niw_stats", "kl"):
        np.testing.assert_allclose(_np(b[k]), _np(a[k]), rtol=1e-11, atol=1e-11, err_msg=k)
    # sampler, VJP and global step of the two families on the same inputs
    from svae_amd import _lib
    lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream(torch.device(DEV))
    S = 2
    rng = np.random.default_rng(N)
    eps, gs_ = _t(rng.standard_normal((T, S, N))), _t(rng.standard_normal((T, S, N)))
    gk = _t([0.7])
    nJ, nh, lgt, ggt = _t(node[0]), _t(node[1]), _t(lg), _t(gg)
    res = []
    for pre in ("svae_gmm_", "svae_gmm_wide_"):
        smp = torch.empty(T, S, N, dtype=torch.float64, device=DEV)
        assert getattr(lib, pre + "sample_f64")(T, N, S, p(a["gaussian_natparam"]), p(eps), p(smp), st) == 0
        gJ, gh = torch.empty_like(nJ), torch.empty_like(nh)
        assert getattr(lib, pre + "local_vjp_f64")(T, N, K, S, p(lgt), p(ggt), p(nJ), p(nh), p(a["gaussian_natparam"]),
                                                   p(a["label_natparam"]), p(gk), p(eps), p(gs_), p(gJ), p(gh), st) == 0
        res.append((smp, gJ, gh))
    for x, y in zip(*res):
        np.testing.assert_allclose(_np(y), _np(x), rtol=1e-9, atol=1e-10)


def _tail_problem(T, N, K, seed):
    from svae_amd.models import gmm
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    prior = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=0.5, niw_conc=1.0, generator=gen))
    glob = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=1.0, niw_conc=2.0, random_scale=2.0, generator=gen))
    nJ = _t(-0.5 * np.log1p(np.exp(rng.standard_normal((T, N)))) - 0.5).requires_grad_(True)
    nh = _t(2 * rng.standard_normal((T, N))).requires_grad_(True)
    init = _t(rng.random((T, K)))
    init = init / init.sum(-1, keepdim=True)
    return prior, glob, nJ, nh, init, rng


@pytest.mark.gpu
@pytest.mark.parametrize("N,S,mode", [(10, 1, "both"), (10, 3, "kl"), (16, 3, "samples"), (16, 1, "both"),
                                      (12, 3, "both")])
def test_wide_sampler_and_local_vjp_against_torch_autograd(N, S, mode):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _gmm_torch import final_pass_torch, sample_torch
    from svae_amd.distributions import expfam
    from svae_amd.models import gmm
    T, K = 37, 7
    prior, glob, nJ, nh, init, rng = _tail_problem(T, N, K, 10 * N + S)
    eps = _t(rng.standard_normal((T, S, N)))
    wS, wk = _t(rng.standard_normal((T, S, N))), 0.7
    samples, stats, gkl, lkl = gmm.run_inference_differentiable(prior, glob, (nJ, nh), S, label_init=init, eps=eps)
    loss = {"both": wk * lkl + (wS * samples).sum(), "kl": wk * lkl, "samples": (wS * samples).sum()}[mode]
    gJ, gh = torch.autograd.grad(loss, [nJ, nh])
    lg, gg = expfam.dirichlet_expectedstats(glob[0]), expfam.niw_expectedstats(glob[1])
    o = gmm.meanfield_from_globals(lg, gg, (nJ.detach(), nh.detach()), init)
    a, b = nJ.detach().clone().requires_grad_(True), nh.detach().clone().requires_grad_(True)
    _, (_, natp), kl_t = final_pass_torch(lg, gg, expfam.pack_dense(a, b), o["label_fixed"])
    smp_t = sample_torch(natp, eps)
    loss_t = {"both": wk * kl_t + (wS * smp_t).sum(), "kl": wk * kl_t, "samples": (wS * smp_t).sum()}[mode]
    wJ, wh = torch.autograd.grad(loss_t, [a, b])
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-300))
    samples, lkl = samples.detach(), lkl.detach()
    assert rel(samples, smp_t) < 1e-10 and abs(float(lkl) - float(kl_t)) < 1e-9 * max(1.0, abs(float(kl_t)))
    assert rel(gJ, wJ) < 1e-8, rel(gJ, wJ)
    assert rel(gh, wh) < 1e-8, rel(gh, wh)


@pytest.mark.gpu
def test_wide_local_tail_gradcheck():
    """The differentiable tail alone (final pass from fixed responsibilities + sampler; the fixed point is held constant
    as in the reference): forward = the wide final pass (max_iter=0) and sampler, backward = svae_gmm_wide_local_vjp_f64."""
    from svae_amd.models import gmm
    T, N, K, S = 2, 9, 3, 2
    prior, glob, nJ, nh, init, rng = _tail_problem(T, N, K, 5)
    lg, gg, _ = gmm.global_step(glob)
    eps = _t(rng.standard_normal((T, S, N)))
    wS = _t(rng.standard_normal((T, S, N)))

    def f(a, b):
        o = gmm.meanfield_from_globals(lg, gg, (a.detach(), b.detach()), init, max_iter=0)
        assert o["path"] == "wide_sweeps"
        s, l = gmm._LocalTail.apply(a, b, eps, lg, gg, o)
        return 0.3 * l + (wS * s).sum()
    assert torch.autograd.gradcheck(f, (nJ, nh), eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(1, 9), (15, 9), (64, 9), (1, 16), (15, 16), (64, 16)])
def test_wide_global_step_against_the_torch_maps(K, N):
    from svae_amd.distributions import expfam
    from svae_amd.models import gmm
    gen = torch.Generator().manual_seed(10 * K + N)
    prior = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=0.7, niw_conc=1.5, generator=gen))
    glob = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=1.3, niw_conc=3.0, random_scale=2.0, generator=gen))
    lg, gg, kl = gmm.global_step(glob, prior, reference_compat=False)
    np.testing.assert_allclose(_np(lg), _np(expfam.dirichlet_expectedstats(glob[0])), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(_np(gg), _np(expfam.niw_expectedstats(glob[1])), rtol=1e-10, atol=1e-12)
    assert float(kl) == pytest.approx(float(gmm.prior_kl(glob, prior, reference_compat=False)), rel=1e-9, abs=1e-9)
    _, _, kl_shipped = gmm.global_step(glob, prior)
    assert float(kl_shipped) == pytest.approx(float(gmm.prior_kl(glob, prior)), rel=1e-9, abs=1e-9)
    assert int(gmm.global_step.last_info.item()) == 0
    bad = glob[1].clone()
    bad[K - 1, :N, :N] = -bad[K - 1, :N, :N]
    gmm.global_step((glob[0], bad))
    assert int(gmm.global_step.last_info.item()) == 1


@pytest.mark.gpu
def test_wide_multi_wg_false_raises():
    from svae_amd.models.gmm import meanfield_from_globals
    lg, gg, node, init = _problem(20, 10, 4, 1)
    with pytest.raises(ValueError, match="single-workgroup"):
        meanfield_from_globals(lg, gg, node, init, multi_wg=False)


@pytest.mark.gpu
def test_wide_differentiable_step_captures_into_one_graph():
    from svae_amd.models import gmm
    T, N, K, S = 300, 10, 15, 1
    prior, glob, nJ, nh, init, rng = _tail_problem(T, N, K, 3)
    eps = _t(rng.standard_normal((T, S, N)))
    nJd, nhd = nJ.detach(), nh.detach()

    def step():
        a, b = nJd.clone().requires_grad_(True), nhd.clone().requires_grad_(True)
        s, stats, gkl, lkl = gmm.run_inference_differentiable(prior, glob, (a, b), S, label_init=init, eps=eps,
                                                              check=False)
        gJ, gh = torch.autograd.grad(lkl + s.sum(), [a, b])
        return s.detach(), stats[1].detach(), lkl.detach(), gJ, gh
    want = step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_wide_make_gradfun_step_gives_finite_gradients():
    from svae_amd import svae
    from svae_amd.models import gmm
    from svae_amd.nnet import gaussian_info_two_heads as gaussian_info, tanh_mlp
    K, N, P = 6, 16, 3
    dev = torch.device(DEV)
    gen = torch.Generator(device=dev).manual_seed(2)
    cpu_gen = torch.Generator().manual_seed(2)
    data = torch.randn(80, P, dtype=torch.float64, device=dev, generator=gen)
    mlp = lambda sizes: [(torch.randn(a, b, dtype=torch.float64, device=dev, generator=gen) / np.sqrt(a))
                         .requires_grad_(True) for a, b in zip(sizes[:-1], sizes[1:])]
    prior = tuple(x.to(dev) for x in gmm.init_pgm_param(K, N, alpha=0.05 / K, niw_conc=0.5, generator=cpu_gen))
    pgm = tuple(x.to(dev) for x in gmm.init_pgm_param(K, N, alpha=1., niw_conc=1., random_scale=3., generator=cpu_gen))
    recogn = (mlp([P, 20, N]), mlp([P, 20, N]))
    decoder = mlp([N, 20, P])

    def loglike(params, samples, batch):
        mean = tanh_mlp(params, samples)
        return -0.5 * ((batch.unsqueeze(1) - mean) ** 2).sum() / samples.shape[1]
    run = lambda *a: gmm.run_inference_differentiable(*a, generator=gen)
    gradfun = svae.make_gradfun(run, gaussian_info, loglike, prior, data, 40, 1, generator=cpu_gen)
    natgrad, g_dec, g_rec = gradfun((pgm, decoder, recogn), 0)
    for g in svae._leaves((natgrad, g_dec, g_rec)):
        assert torch.isfinite(g).all()
    assert float(svae.flat(g_rec).abs().sum()) > 0


def _dist_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from svae_amd.models.gmm import meanfield_from_globals
        from svae_amd.parallel import shard_bounds
        lg, gg, node, init = _problem(700, 10, 8, 11)
        lo, hi = shard_bounds(700, rank, world)
        o = meanfield_from_globals(lg, gg, (node[0][lo:hi], node[1][lo:hi]), init[lo:hi])
        ds, ns = o["dirichlet_stats"].clone(), o["niw_stats"].clone()
        dist.all_reduce(ds)
        dist.all_reduce(ns)
        q.put((rank, o["path"], _np(o["assign"]), int(o["iters"].item()), _np(ds), _np(ns)))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_wide_two_ranks_on_one_gpu_reproduce_the_single_process_results():
    import socket
    import torch.multiprocessing as mp
    from svae_amd.models.gmm import meanfield_from_globals
    lg, gg, node, init = _problem(700, 10, 8, 11)
    want = meanfield_from_globals(lg, gg, node, init)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from svae_amd.parallel import shard_bounds
    for rank, path, assign, iters, ds, ns in res:
        lo, hi = shard_bounds(700, rank, 2)
        assert path == "wide_sweeps"
        assert iters == int(want["iters"].item())
        assert np.array_equal(assign, _np(want["assign"])[lo:hi])                 # bit-exact labels
        np.testing.assert_allclose(ds, _np(want["dirichlet_stats"]), rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(ns, _np(want["niw_stats"]), rtol=1e-11, atol=1e-9)
