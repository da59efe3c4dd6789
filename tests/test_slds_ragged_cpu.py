"""CPU tests of the per-step ragged LDS E-step (svae_lds_ragged_perstep_*) and of `lengths=` on the SLDS model layer: the
construction the kernel implements, restated on oracle/lds_numpy.py; the C ABI's host-side argument checks; and the
keyword errors that need no device."""
import ctypes
import os

import numpy as np
import pytest

import _slds_ragged_numpy as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,T", [(1, 6), (3, 2), (4, 7), (10, 12), (15, 5), (9, 17)])
def test_decoupled_perstep_chain_equals_the_cut_chain(n, T):
    """A chain of T steps with the real per-step pair parameters at t <= L-2, Q at t >= L-1, zero node potentials from L on
    and the init potential passed whole equals the chain cut at L: lognorm, E_init, E_pair[:L-1], E_node[:L], samples[:L]
    to 5e-15 relative (the bound of the shared-pair construction test's measurement); the tail's moments are exactly
    I and 0 and its samples exactly eps.  L = 1 included: pair 0 is then Q, which is why the init potential cannot be
    folded into J11[0]."""
    rng = np.random.default_rng(1000 * n + T)
    init, pair = sr.mixed_lds_params(n, T, rng)
    J, h = sr.slds_nodes(1, T, n, rng)
    node = (J[0], h[0], rng.standard_normal(T))
    eps = rng.standard_normal((T, 2, n))
    for L in sorted({1, min(2, T), max(T - 1, 1), T, (T + 1) // 2}):
        ln_p, (Ei_p, Ep_p, En_p), s_p = sr.padded_perstep_run(init, pair, node, L, eps)
        ln_c, (Ei_c, Ep_c, En_c), s_c = sr.cut_perstep_run(init, pair, node, L, eps)
        assert sr.rel(ln_p, ln_c) <= 5e-15
        assert sr.rel(Ei_p[0], Ei_c[0]) <= 5e-15 and sr.rel(Ei_p[1], Ei_c[1]) <= 5e-15
        assert sr.rel(En_p[0][:L], En_c[0]) <= 5e-15 and sr.rel(En_p[1][:L], En_c[1]) <= 5e-15
        assert sr.rel(s_p[:L], s_c) <= 5e-15
        for i in range(3):
            assert sr.rel(np.asarray(Ep_p[i])[:L - 1], Ep_c[i]) <= 5e-15
        # the tail: exact
        assert np.all(En_p[1][L:] == 0.0) and np.all(En_p[0][L:] == 1.0)
        assert np.array_equal(s_p[L:], eps[L:])
        assert np.all(np.asarray(Ep_p[1])[L - 1:] == 0.0)
        assert np.all(np.asarray(Ep_p[2])[L - 1:] == np.eye(n)[None])
        assert np.all(np.asarray(Ep_p[0])[L:] == np.eye(n)[None])


def test_folding_the_init_potential_into_pair_0_is_wrong_for_a_one_step_sequence():
    """what the per-sequence init potential argument is for: with L = 1 pair 0 is Q, and an init potential added to
    J11[0] is lost with it"""
    n, T = 3, 4
    rng = np.random.default_rng(5)
    init, pair = sr.mixed_lds_params(n, T, rng)
    J, h = sr.slds_nodes(1, T, n, rng)
    node = (J[0], h[0])
    ln_c, _, _ = sr.cut_perstep_run(init, pair, node, 1)
    folded = (pair[0].copy(), pair[1], pair[2], pair[3])
    folded[0][0] += init[0]
    ln_f, _, _ = sr.padded_perstep_run((np.zeros((n, n)), init[1], init[2]), folded, node, 1)
    assert not np.isfinite(ln_f) or abs(ln_f - ln_c) > 1e-3 * abs(ln_c)


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


PERSTEP_SYMBOLS = ("svae_lds_ragged_perstep_workspace_bytes", "svae_lds_ragged_perstep_estep_f64",
                   "svae_lds_ragged_perstep_inference_f64")


def test_perstep_symbols_are_exported_and_declared():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    for s in PERSTEP_SYMBOLS:
        assert s in L.SIGNATURES and hasattr(lib, s), s
        assert s + "(" in hdr, s


def test_perstep_workspace_bytes():
    _, lib = _lib()
    for B, T, n in ((1, 1, 1), (5, 9, 4), (7, 12, 10), (6, 7, 15), (512, 200, 10)):
        base = lib.svae_lds_workspace_bytes(B, T, n)
        assert lib.svae_lds_ragged_perstep_workspace_bytes(B, T, n) == (base + 255) // 256 * 256 + 2 * n * n * 8
    for B, T, n in ((0, 5, 4), (2, 0, 4), (2, 5, 0), (2, 5, 16), (2, 5, 64)):
        assert lib.svae_lds_ragged_perstep_workspace_bytes(B, T, n) == 0


def test_perstep_entries_reject_bad_arguments_on_the_host():
    """every argument error has its own code and comes back before any HIP call (the pointers are host memory: nothing
    may be launched); an empty batch returns 0"""
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    info = (ctypes.c_int32 * 1)()
    pi = ctypes.cast(info, ctypes.c_void_p)
    need = lib.svae_lds_ragged_perstep_workspace_bytes(2, 3, 4)

    def estep(B=2, T=3, n=4, batched=0, init_batched=0, keep=0, options=0, ptrs=None, lengths=p, outs=None, info_p=pi,
              ws=p, ws_bytes=need):
        ptrs = [p] * 10 if ptrs is None else ptrs
        outs = [p] * 5 if outs is None else outs
        return lib.svae_lds_ragged_perstep_estep_f64(B, T, n, batched, init_batched, keep, options, *ptrs, lengths, *outs,
                                                     info_p, ws, ws_bytes, None)

    assert estep(B=-1) == -1 and estep(T=0) == -2
    for n in (0, 16, 64, 128):
        assert estep(n=n) == -3
    assert estep(batched=2) == -32 and estep(init_batched=2) == -32 and estep(batched=-1) == -32
    assert estep(lengths=None) == -31
    assert estep(keep=2) == -23 and estep(keep=3) == -23 and estep(keep=4) == -23 and estep(keep=-1) == -23
    assert estep(options=3) == -24 and estep(options=0x1000) == -24 and estep(options=0x300) == -24
    assert estep(ws=None) == -22 and estep(ws_bytes=need - 8) == -22
    assert estep(ws_bytes=lib.svae_lds_workspace_bytes(2, 3, 4)) == -22      # the uniform size is too short: the table
    for k, code in ((0, -6), (1, -7), (2, -8), (3, -9), (4, -9), (5, -9), (6, -9), (7, -13), (8, -14)):
        ptrs = [p] * 10
        ptrs[k] = None
        assert estep(ptrs=ptrs) == code, k
    ptrs = [p] * 10
    ptrs[9] = None                                                           # node_logZ is optional
    assert estep(ptrs=ptrs, B=0) == 0
    ptrs = [p] * 3 + [None] * 4 + [p] * 3                                    # T = 1: no pair parameters, no E_pair
    assert estep(T=1, ptrs=ptrs, outs=[p, p, None, p, p], B=0) == 0
    for k, code in ((0, -16), (1, -17), (2, -18), (3, -19), (4, -20)):
        outs = [p] * 5
        outs[k] = None
        assert estep(outs=outs) == code, k
    assert estep(info_p=None) == -21
    assert estep(B=0, ws=None, ws_bytes=0) == 0
    for flags in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert estep(B=0, batched=flags[0], init_batched=flags[1], keep=1) == 0
    assert estep(B=0, lengths=None) == -31 and estep(B=0, n=16) == -3 and estep(B=0, options=3) == -24

    def infer(B=2, T=3, n=4, S=1, batched=0, init_batched=0, options=0, lengths=p, eps=p, smp=p, ws=p, ws_bytes=need):
        return lib.svae_lds_ragged_perstep_inference_f64(B, T, n, S, batched, init_batched, options, *([p] * 10), lengths,
                                                         eps, smp, *([p] * 5), pi, ws, ws_bytes, None)

    assert infer(B=-1) == -1 and infer(T=0) == -2 and infer(n=16) == -3 and infer(n=0) == -3
    assert infer(S=-1) == -4 and infer(eps=None) == -4 and infer(smp=None) == -4
    assert infer(batched=2) == -32 and infer(init_batched=-1) == -32 and infer(lengths=None) == -31
    assert infer(options=3) == -24 and infer(ws_bytes=need - 8) == -22 and infer(ws=None) == -22
    assert infer(B=0) == 0 and infer(B=0, S=0, eps=None, smp=None) == 0 and infer(B=0, S=40) == 0


def test_slds_differentiable_entries_refuse_lengths_without_a_device():
    """the VJP sweeps for per-step pair parameters with lengths are not built: ValueError before anything else happens"""
    pytest.importorskip("torch")
    from svae_amd.models import slds_svae
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_differentiable(None, None, None, 1, lengths=[2, 3])
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_withlabels_differentiable(None, None, None, 1, lengths=[2, 3])


def test_slds_lengths_errors_come_from_shapes_alone():
    """fused=True, n = 16, K = 65, a wrong shape, a float dtype, T = 1: ValueError from CPU tensors, nothing launched"""
    torch = pytest.importorskip("torch")
    from svae_amd.models import slds_svae

    def call(K=3, n=4, T=6, B=3, lengths=None, fused=None):
        glob = ((None, None), [None] * K)
        node = (torch.zeros(B, T, n, dtype=torch.float64), torch.zeros(B, T, n, dtype=torch.float64))
        lengths = [2, 3, T] if lengths is None else lengths
        return slds_svae._slds_lengths(lengths, glob, node, fused, "test")

    for kw in (dict(fused=True), dict(n=16), dict(K=65), dict(T=1, lengths=[1, 1, 1]), dict(lengths=[2, 3]),
               dict(lengths=np.array([2., 3., 4.])), dict(lengths=torch.tensor([2., 3., 4.])),
               dict(lengths=np.array([[2, 3, 4]]))):
        with pytest.raises(ValueError, match="lengths"):
            call(**kw)
    for fn, args in ((slds_svae.optimize_local_meanfield, ()), (slds_svae.run_inference, None)):
        glob = ((None, None), [None] * 3)
        node = (torch.zeros(3, 6, 16, dtype=torch.float64), torch.zeros(3, 6, 16, dtype=torch.float64))
        with pytest.raises(ValueError, match="latent dimension"):
            if args is None:
                fn(None, glob, node, 1, lengths=[2, 3, 6])
            else:
                fn(glob, node, None, lengths=[2, 3, 6])
    node = (torch.zeros(3, 6, 4, dtype=torch.float64), torch.zeros(3, 6, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="fused"):
        slds_svae.optimize_local_meanfield(((None, None), [None] * 3), node, None, fused=True, lengths=[2, 3, 6])
