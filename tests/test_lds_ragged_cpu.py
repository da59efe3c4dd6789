"""CPU tests of the variable-length LDS batch (svae_lds_ragged_*, `lengths=`): the mathematics the kernels implement,
the C ABI's host-side argument checks, and the exchange step's unpacking of the pair-count slot."""
import ctypes
import os

import numpy as np
import pytest

import _lds_ragged_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lengths_of(T):
    return sorted({1, min(2, T), max(T - 1, 1), T, (T + 1) // 2})


@pytest.mark.parametrize("model", ["rand", "rotation"])
@pytest.mark.parametrize("n,T", [(1, 6), (3, 2), (3, 9), (4, 7), (10, 12), (15, 5), (4, 1)])
def test_two_slot_chain_equals_the_truncated_chain(model, n, T):
    """lognorm, E_init, the node statistics and the pair sums over t < L-1 of the padded chain are the truncated
    chain's (bound 1e-12 relative; measured 5e-15); the tail is exactly a chain of independent standard normals: E[x] = 0,
    E[x x'] = I, cross moments 0, samples = eps, compared with ==."""
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials, rotation_lds_natparam
    rng = np.random.default_rng(1000 * n + T)
    natparam = (rand_lds_natparam if model == "rand" else rotation_lds_natparam)(n, rng)
    node = rand_node_potentials((T, n), rng, with_logZ=True)
    eps = rng.standard_normal((T, 2, n))
    for L in _lengths_of(T):
        ln_p, (Ei_p, Ep_p, En_p), s_p = rn.padded_run(natparam, node, L, eps)
        ln_t, (Ei_t, Ep_t, En_t), s_t = rn.truncated_run(natparam, node, L, eps)
        assert rn.rel(ln_p, ln_t) < 1e-12
        assert rn.rel(Ei_p[0], Ei_t[0]) < 1e-12 and rn.rel(Ei_p[1], Ei_t[1]) < 1e-12
        assert rn.rel(En_p[0][:L], En_t[0]) < 1e-12 and rn.rel(En_p[1][:L], En_t[1]) < 1e-12
        assert rn.rel(s_p[:L], s_t) < 1e-12
        if T > 1:
            for i in range(3):
                want = np.asarray(Ep_t[i]) if L > 1 else np.zeros((n, n))        # (L = 1: no pair, every sum is 0)
                assert rn.rel(np.asarray(Ep_p[i])[:L - 1].sum(0), want) < 1e-12
        # the tail: exact
        assert np.all(En_p[1][L:] == 0.0) and np.all(En_p[0][L:] == 1.0)
        assert np.array_equal(s_p[L:], eps[L:])
        if T > 1:
            cross, nxt = np.asarray(Ep_p[1]), np.asarray(Ep_p[2])
            assert np.all(cross[L - 1:] == 0.0)
            assert np.all(nxt[L - 1:] == np.eye(n)[None])


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


RAGGED_SYMBOLS = ("svae_lds_ragged_workspace_bytes", "svae_lds_ragged_estep_f64", "svae_lds_ragged_inference_f64",
                  "svae_lds_ragged_vjp_f64", "svae_lds_ragged_reduce_stats_f64", "svae_lds_ragged_natgrad_f64")


def test_ragged_symbols_are_exported_and_declared():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    for s in RAGGED_SYMBOLS:
        assert s in L.SIGNATURES and hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert lib.svae_hip_abi_version() == 15 and L.ABI_VERSION == 15
    assert "cython_lds_inference.pyx:28-90" in hdr and ":149-210" in hdr and ":310-355" in hdr


def test_ragged_workspace_bytes():
    _, lib = _lib()
    for B, T, n in ((1, 1, 1), (5, 9, 4), (7, 12, 10), (6, 7, 15), (512, 200, 10)):
        base = lib.svae_lds_workspace_bytes(B, T, n)
        assert lib.svae_lds_ragged_workspace_bytes(B, T, n) == (base + 255) // 256 * 256 + 6 * n * n * 8
    for B, T, n in ((0, 5, 4), (2, 0, 4), (2, 5, 0), (2, 5, 16), (2, 5, 64)):
        assert lib.svae_lds_ragged_workspace_bytes(B, T, n) == 0


def test_ragged_entries_reject_bad_arguments_on_the_host():
    """every argument error has its own code and comes back before any HIP call (the pointers are host memory: nothing
    may be launched); an empty batch returns 0"""
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    info = (ctypes.c_int32 * 1)()
    pi = ctypes.cast(info, ctypes.c_void_p)
    need = lib.svae_lds_ragged_workspace_bytes(2, 3, 4)

    def estep(B=2, T=3, n=4, inhomog=0, batched=0, keep=0, options=0, ptrs=None, lengths=p, outs=None, info_p=pi, ws=p,
              ws_bytes=need):
        ptrs = [p] * 10 if ptrs is None else ptrs
        outs = [p] * 5 if outs is None else outs
        return lib.svae_lds_ragged_estep_f64(B, T, n, inhomog, batched, keep, options, *ptrs, lengths, *outs, info_p, ws,
                                             ws_bytes, None)

    assert estep(B=-1) == -1 and estep(T=0) == -2
    for n in (0, 16, 64, 128):
        assert estep(n=n) == -3
    assert estep(inhomog=1) == -32 and estep(inhomog=1, batched=1) == -32 and estep(batched=1) == -32
    assert estep(lengths=None) == -31
    assert estep(keep=4) == -23 and estep(keep=-1) == -23
    assert estep(options=3) == -24 and estep(options=0x1000) == -24 and estep(options=0x300) == -24
    assert estep(ws=None) == -22 and estep(ws_bytes=need - 8) == -22
    assert estep(ws_bytes=lib.svae_lds_workspace_bytes(2, 3, 4)) == -22      # the uniform size is too short: the pair tables
    for k, code in ((0, -6), (1, -7), (2, -8), (3, -9), (7, -13), (8, -14)):
        ptrs = [p] * 10
        ptrs[k] = None
        assert estep(ptrs=ptrs) == code, k
    for k, code in ((0, -16), (1, -17), (2, -18), (3, -19), (4, -20)):
        outs = [p] * 5
        outs[k] = None
        assert estep(outs=outs) == code, k
    assert estep(info_p=None) == -21
    codes = {-1, -2, -3, -32, -31, -23, -24, -22}
    assert len(codes) == 8
    assert estep(B=0, ws=None, ws_bytes=0) == 0
    assert estep(B=0, lengths=None) == -31 and estep(B=0, n=16) == -3 and estep(B=0, options=3) == -24

    def infer(B=2, T=3, n=4, S=1, inhomog=0, batched=0, keep_vjp=1, options=0, lengths=p, eps=p, smp=p, ws_bytes=need):
        return lib.svae_lds_ragged_inference_f64(B, T, n, S, inhomog, batched, keep_vjp, options, *([p] * 10), lengths, eps,
                                                 smp, *([p] * 5), pi, p, ws_bytes, None)

    assert infer(n=16) == -3 and infer(S=-1) == -4 and infer(eps=None) == -4 and infer(smp=None) == -4
    assert infer(keep_vjp=2) == -23 and infer(inhomog=1) == -32 and infer(lengths=None) == -31
    assert infer(options=3) == -24 and infer(ws_bytes=need - 8) == -22
    assert infer(B=0) == 0 and infer(B=0, S=0, eps=None, smp=None) == 0

    vneed = lib.svae_lds_vjp_workspace_bytes(2, 3, 4)

    def vjp(B=2, T=3, n=4, S=1, inhomog=0, batched=0, options=0, g_ln=p, gs=p, eps=p, smp=p, lengths=p, gJ=p, gh=p,
            ws=p, ws_bytes=need, vws=p, vws_bytes=vneed):
        return lib.svae_lds_ragged_vjp_f64(B, T, n, S, inhomog, batched, options, g_ln, p, p, gs, eps, smp, lengths, gJ, gh,
                                           ws, ws_bytes, vws, vws_bytes, None)

    assert vjp(B=-1) == -1 and vjp(T=0) == -2 and vjp(n=16) == -3 and vjp(n=0) == -3
    assert vjp(inhomog=1) == -32 and vjp(batched=1) == -32 and vjp(lengths=None) == -31
    assert vjp(S=0) == -4 and vjp(S=17) == -4 and vjp(S=0, gs=None) != -4
    assert vjp(g_ln=None) == -6 and vjp(eps=None) == -10 and vjp(smp=None) == -10
    assert vjp(gJ=None) == -12 and vjp(gh=None) == -13
    assert vjp(options=3) == -24
    assert vjp(ws=None) == -14 and vjp(ws_bytes=need - 8) == -14
    assert vjp(vws=None) == -16 and vjp(vws_bytes=vneed - 8) == -16
    assert vjp(B=0, ws=None, vws=None) == 0

    red = lib.svae_lds_ragged_reduce_stats_f64
    assert red(-1, 3, 4, p, p, p, p, p, None) == -1 and red(2, 0, 4, p, p, p, p, p, None) == -7
    assert red(2, 3, 16, p, p, p, p, p, None) == -2 and red(2, 3, 4, None, p, p, p, p, None) == -3
    assert red(2, 3, 4, p, None, p, p, p, None) == -4 and red(2, 3, 4, p, p, None, p, p, None) == -5
    assert red(2, 3, 4, p, p, p, None, p, None) == -31 and red(2, 3, 4, p, p, p, p, None, None) == -6
    ng = lib.svae_lds_ragged_natgrad_f64
    assert ng(0, p, p, p, 1.0, 1.0, p, None) == -1 and ng(4, None, p, p, 1.0, 1.0, p, None) == -3
    assert ng(4, p, None, p, 1.0, 1.0, p, None) == -4 and ng(4, p, p, None, 1.0, 1.0, p, None) == -5
    assert ng(4, p, p, p, 1.0, 1.0, None, None) == -8


def test_ragged_exchange_takes_the_pair_count_from_its_slot():
    """allreduce_lds_stats(ragged=True) on a hand-made packed buffer: the MNIW count is the buffer's last slot (the sum of
    lengths - 1), not count (T-1); the uniform layout is unchanged; a buffer of the other layout is refused"""
    torch = pytest.importorskip("torch")
    from svae_amd.parallel import allreduce_lds_stats
    n, T = 3, 9
    nn = n * n
    body = torch.arange(1, 4 * nn + n + 1, dtype=torch.float64)
    ragged = torch.cat([body, torch.tensor([-7.5, 5.0, 17.0], dtype=torch.float64)])      # lognorm sum, B = 5, pairs = 17
    kl = torch.tensor(2.25, dtype=torch.float64)
    niw, mniw, out_kl, packed = allreduce_lds_stats(ragged, kl, n, T, return_packed=True, ragged=True)
    assert float(mniw[3]) == 17.0 and float(mniw[3]) != 5.0 * (T - 1)
    assert float(niw[n, n]) == 5.0 and float(niw[n + 1, n + 1]) == 5.0
    assert torch.equal(mniw[0], body[nn + n:2 * nn + n].reshape(n, n))
    assert torch.equal(mniw[2], body[3 * nn + n:4 * nn + n].reshape(n, n))
    assert float(out_kl) == 2.25 and float(packed[-3]) == 2.25 and float(packed[-1]) == 17.0 and packed.numel() == ragged.numel()
    assert float(ragged[-3]) == -7.5                  # (the caller's buffer is left as it was)
    uniform = torch.cat([body, torch.tensor([-7.5, 5.0], dtype=torch.float64)])
    _, mniw_u, _ = allreduce_lds_stats(uniform, kl, n, T)
    assert float(mniw_u[3]) == 5.0 * (T - 1)
    with pytest.raises(ValueError):
        allreduce_lds_stats(uniform, kl, n, T, ragged=True)
    with pytest.raises(ValueError):
        allreduce_lds_stats(ragged, kl, n, T)
