"""CPU tests of the reverse sweeps of the per-step ragged LDS (svae_lds_ragged_perstep_inference_keep_f64,
svae_lds_ragged_perstep_vjp_f64): the two entries exist and are declared, every documented argument error comes back
before any HIP call, the ABI version is where it was -- and the gradient oracle of the GPU tests,
tests/_lds_large_torch.torch_estep(per_step_stats=True) under fp64 autograd, is pinned against itself on the construction
the kernels implement before any GPU test trusts it."""
import ctypes
import os

import numpy as np
import pytest

import _slds_ragged_numpy as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("svae_lds_ragged_perstep_inference_keep_f64", "svae_lds_ragged_perstep_vjp_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_new_entries_are_exported_and_declared_and_the_version_stays():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15
    assert "#define SVAE_HIP_ABI_VERSION 15 " in hdr
    assert "There are no VJP sweeps on these records" not in hdr


def test_forward_entry_rejects_bad_arguments_on_the_host():
    """the pointers are host memory: nothing may be launched; an empty batch returns 0"""
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    info = (ctypes.c_int32 * 1)()
    pi = ctypes.cast(info, ctypes.c_void_p)
    need = lib.svae_lds_ragged_perstep_workspace_bytes(2, 3, 4)

    def infer(B=2, T=3, n=4, S=1, batched=0, init_batched=0, keep_vjp=1, options=0, ptrs=None, lengths=p, eps=p, smp=p,
              outs=None, info_p=pi, ws=p, ws_bytes=need):
        ptrs = [p] * 10 if ptrs is None else ptrs
        outs = [p] * 5 if outs is None else outs
        return lib.svae_lds_ragged_perstep_inference_keep_f64(B, T, n, S, batched, init_batched, keep_vjp, options, *ptrs,
                                                              lengths, eps, smp, *outs, info_p, ws, ws_bytes, None)

    assert infer(B=-1) == -1 and infer(T=0) == -2
    for n in (0, 16, 64):
        assert infer(n=n) == -3
    assert infer(S=-1) == -4 and infer(eps=None) == -4 and infer(smp=None) == -4
    assert infer(keep_vjp=2) == -23 and infer(keep_vjp=-1) == -23 and infer(keep_vjp=3) == -23
    assert infer(batched=2) == -32 and infer(init_batched=-1) == -32
    assert infer(lengths=None) == -31
    for k, code in ((0, -6), (1, -7), (2, -8), (3, -9), (4, -9), (5, -9), (6, -9), (7, -13), (8, -14)):
        ptrs = [p] * 10
        ptrs[k] = None
        assert infer(ptrs=ptrs) == code, k
    for k, code in ((0, -16), (1, -17), (2, -18), (3, -19), (4, -20)):
        outs = [p] * 5
        outs[k] = None
        assert infer(outs=outs) == code, k
    assert infer(info_p=None) == -21
    assert infer(options=3) == -24
    assert infer(ws=None) == -22 and infer(ws_bytes=need - 8) == -22
    for kv in (0, 1):
        assert infer(B=0, keep_vjp=kv) == 0 and infer(B=0, keep_vjp=kv, S=0, eps=None, smp=None) == 0
    assert infer(B=0, ws=None, ws_bytes=0) == 0
    # the entry without keep_vjp keeps refusing the cross moments
    assert lib.svae_lds_ragged_perstep_estep_f64(2, 3, 4, 0, 0, 2, 0, *([p] * 10), p, *([p] * 5), pi, p, need, None) == -23
    assert lib.svae_lds_ragged_perstep_estep_f64(2, 3, 4, 0, 0, 3, 0, *([p] * 10), p, *([p] * 5), pi, p, need, None) == -23


def test_vjp_entry_rejects_bad_arguments_on_the_host():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.svae_lds_ragged_perstep_workspace_bytes(2, 3, 4)
    vneed = lib.svae_lds_vjp_workspace_bytes(2, 3, 4)
    assert vneed > 0

    def vjp(B=2, T=3, n=4, S=1, batched=0, options=0, J12=p, g_ln=p, g_dxx=p, g_x=p, g_Ei=p, g_Ep=p, g_s=p, eps=p, smp=p,
            E_pair=p, E_x=p, lengths=p, gJ=p, gh=p, ws=p, ws_bytes=need, vws=p, vws_bytes=vneed):
        return lib.svae_lds_ragged_perstep_vjp_f64(B, T, n, S, batched, options, J12, g_ln, g_dxx, g_x, g_Ei, g_Ep, g_s, eps,
                                                   smp, E_pair, E_x, lengths, gJ, gh, ws, ws_bytes, vws, vws_bytes, None)

    assert vjp(B=-1) == -1 and vjp(T=0) == -2
    for n in (0, 16, 64):
        assert vjp(n=n) == -3
    assert vjp(batched=2) == -32 and vjp(batched=-1) == -32
    assert vjp(lengths=None) == -31
    assert vjp(S=0) == -4 and vjp(S=17) == -4
    assert vjp(J12=None) == -5
    assert vjp(g_ln=None) == -6
    assert vjp(E_pair=None) == -8 and vjp(E_x=None) == -8
    assert vjp(eps=None) == -10 and vjp(smp=None) == -10
    assert vjp(gJ=None) == -12 and vjp(gh=None) == -13
    assert vjp(options=3) == -24
    assert vjp(ws=None) == -14 and vjp(ws_bytes=need - 8) == -14
    assert vjp(ws_bytes=lib.svae_lds_workspace_bytes(2, 3, 4)) == -14        # the uniform size is too short: the table
    assert vjp(vws=None) == -16 and vjp(vws_bytes=vneed - 8) == -16
    # what may be NULL: every cotangent but lognorm's, the forward outputs without g_E_pair, J12 at T = 1, S without g_samples
    assert vjp(B=0, g_dxx=None, g_x=None, g_Ei=None, g_Ep=None, g_s=None, eps=None, smp=None, E_pair=None, E_x=None, S=99) == 0
    assert vjp(B=0, T=1, J12=None) == 0
    assert vjp(B=0, ws=None, ws_bytes=0, vws=None, vws_bytes=0) == 0
    assert vjp(B=0, lengths=None) == -31 and vjp(B=0, n=16) == -3 and vjp(B=0, options=3) == -24


def test_model_layer_names_exist_and_the_old_ones_name_them():
    pytest.importorskip("torch")
    from svae_amd.models import slds_svae
    assert callable(slds_svae.run_inference_ragged_differentiable)
    assert callable(slds_svae.run_inference_withlabels_ragged_differentiable)
    with pytest.raises(ValueError, match="run_inference_ragged_differentiable"):
        slds_svae.run_inference_differentiable(None, None, None, 1, lengths=[2, 3])
    with pytest.raises(ValueError, match="run_inference_withlabels_ragged_differentiable"):
        slds_svae.run_inference_withlabels_differentiable(None, None, None, 1, lengths=[2, 3])


# ---- the gradient oracle, pinned against itself ----------------------------------------------------------------------

def _oracle_case(n, T, S, seed):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(seed)
    init, pair = sr.mixed_lds_params(n, T, rng)
    J, h = sr.slds_nodes(1, T, n, rng)
    c = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x, float)), dtype=torch.float64)
    cot = dict(ln=c(rng.standard_normal(1)), dxx=c(rng.standard_normal((1, T, n))), x=c(rng.standard_normal((1, T, n))),
               s=c(rng.standard_normal((1, T, S, n))), Ei=c(rng.standard_normal((1, n * n + n))),
               Ep=c(rng.standard_normal((1, T - 1, 3, n, n))))
    return dict(init=[c(x) for x in init], pair=[c(x) for x in pair], J=c(J), h=c(h), eps=c(rng.standard_normal((1, T, S, n))),
                cot=cot)


def _functional(outs, cot, L):
    """<cotangents, outputs> over the part that belongs to a sequence of length L: all six outputs"""
    ln, dxx, ex, smp, Ei, Ep = outs
    return (cot["ln"] * ln).sum() + (cot["dxx"][:, :L] * dxx[:, :L]).sum() + (cot["x"][:, :L] * ex[:, :L]).sum() \
        + (cot["s"][:, :L] * smp[:, :L]).sum() + (cot["Ei"] * Ei).sum() + (cot["Ep"][:, :L - 1] * Ep[:, :L - 1]).sum()


@pytest.mark.parametrize("L", [1, 2, 5, 6])
def test_gradient_oracle_on_the_decoupled_chain_equals_the_cut_chain(L):
    """torch_estep(per_step_stats=True) on the sequence cut at L (pair parameters [:L-1], node potentials [:L], the init
    potential whole) against the same function on the decoupled chain of T steps -- Q = (0, 0, -1/2 I, 0) at pairs
    t >= L-1, the node potentials of steps t >= L replaced by 0 (a select, as the kernels do it) -- under fp64 autograd over
    one random linear functional of all six outputs, supported on the cut part: gradients on [:L] equal to 1e-12 of their
    scale, gradients beyond L exactly 0.
    Why the select belongs to the construction: with the tail's potentials as free leaves of value 0 the chain still has
    ONE tail gradient, d lognorm / d node_J[t >= L] = E[x_t^2] = 1 (a standard normal), the gradient of a potential that
    does not exist; the sweeps write 0 there by select too.  The second half of the test shows that this is the only one."""
    import torch
    import _lds_large_torch as lt
    n, T, S = 3, 6, 2
    c = _oracle_case(n, T, S, 600 + L)
    cot = c["cot"]
    # the cut chain
    nJ = c["J"][:, :L].clone().requires_grad_(True)
    nh = c["h"][:, :L].clone().requires_grad_(True)
    pp = [x[:L - 1] for x in c["pair"]]
    outs = lt.torch_estep((c["init"][0], c["init"][1], c["init"][2].reshape(1), *pp), nJ, nh, eps=c["eps"][:, :L],
                          per_step_stats=True)
    assert tuple(outs[5].shape) == (1, L - 1, 3, n, n)
    _functional(outs, cot, L).backward()
    # the decoupled chain
    dp = [torch.as_tensor(x) for x in sr.decoupled_pair_params([x.numpy() for x in c["pair"]], T, L)]
    live = (torch.arange(T) < L)[None, :, None]
    zero = torch.zeros((), dtype=torch.float64)

    def decoupled(select):
        fJ = c["J"].clone()
        fh = c["h"].clone()
        if not select:
            fJ[:, L:] = 0.0
            fh[:, L:] = 0.0
        fJ.requires_grad_(True)
        fh.requires_grad_(True)
        uJ, uh = (torch.where(live, fJ, zero), torch.where(live, fh, zero)) if select else (fJ, fh)
        o = lt.torch_estep((c["init"][0], c["init"][1], c["init"][2].reshape(1), *dp), uJ, uh, eps=c["eps"],
                           per_step_stats=True)
        _functional(o, cot, L).backward()
        return o, fJ.grad, fh.grad
    o, gJ, gh = decoupled(True)
    rel = lambda a, b: float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
    for k in range(6):                                   # the values first: the cut part of every output
        a, b = (o[k][:, :L - 1], outs[k]) if k == 5 else (o[k][:, :L], outs[k]) if k in (1, 2, 3) else (o[k], outs[k])
        assert a.numel() == 0 or rel(a, b) <= 1e-12, k
    assert rel(gJ[:, :L], nJ.grad) <= 1e-12 and rel(gh[:, :L], nh.grad) <= 1e-12
    assert bool((gJ[:, L:] == 0).all()) and bool((gh[:, L:] == 0).all())
    # free tail leaves: the same gradients on [:L]; beyond L only the log-normaliser's own term
    _, gJf, ghf = decoupled(False)
    assert rel(gJf[:, :L], nJ.grad) <= 1e-12 and rel(ghf[:, :L], nh.grad) <= 1e-12
    if L < T:
        scale = float(nJ.grad.abs().max())
        assert float(ghf[:, L:].abs().max()) <= 1e-12 * scale
        assert float((gJf[:, L:] - cot["ln"]).abs().max()) <= 1e-12 * max(scale, 1.0)
