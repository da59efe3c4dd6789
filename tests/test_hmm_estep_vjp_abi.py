"""CPU tests of the C ABI of the HMM E-step's derivative (svae_hmm_estep_vjp_workspace_bytes, svae_hmm_estep_vjp_f64,
svae_hmm_ragged_estep_vjp_f64; include/svae_hip.h): the symbols, the workspace formula, and every argument code --
all decided on the host before any HIP call, so none of this needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("svae_hmm_estep_vjp_workspace_bytes", "svae_hmm_estep_vjp_f64", "svae_hmm_ragged_estep_vjp_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_symbols_are_declared_bound_and_exported_without_a_new_abi_number():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s


@pytest.mark.parametrize("K,KP", [(1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)])
def test_workspace_bytes_closed_form(K, KP):
    """B T records of [a_t | r_t] = 2 KP doubles, then B route flags, rounded up to 128 bytes"""
    _, lib = _lib()
    for B, T in ((1, 1), (3, 2), (5, 7), (1, 3), (7, 5), (2048, 500)):
        got = lib.svae_hmm_estep_vjp_workspace_bytes(B, T, K)
        assert got == -(-(B * T * 2 * KP + B) * 8 // 128) * 128 and got % 16 == 0


def test_workspace_bytes_out_of_range_is_zero():
    _, lib = _lib()
    for B, T, K in ((0, 5, 3), (-1, 5, 3), (2, 0, 3), (2, -4, 3), (2, 5, 0), (2, 5, -1), (2, 5, 65), (2, 5, 1000)):
        assert lib.svae_hmm_estep_vjp_workspace_bytes(B, T, K) == 0


def _aligned():
    raw = (ctypes.c_double * 4096)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    return raw, base


def _in_order(call, bad):
    for i, kw in enumerate(bad):
        assert call(**kw) == -(i + 1), kw
        merged = {}                       # the first failing check decides: every later argument bad as well
        for later in bad[i:]:
            merged = {**later, **merged}
        assert call(**merged) == -(i + 1), merged


def test_vjp_rejects_bad_arguments_on_the_host_in_order():
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)                 # 16-byte aligned host address: must never be dereferenced
    need = lib.svae_hmm_estep_vjp_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, g0=None, g1=None, g2=None, g3=None, di=p, dp=p, dn=p, ws=p,
             ws_bytes=need):
        return lib.svae_hmm_estep_vjp_f64(B, T, K, pb, init, pair, node, g0, g1, g2, g3, di, dp, dn, ws, ws_bytes, None)

    _in_order(call, [dict(B=-1), dict(T=0), dict(K=0), dict(pb=2), dict(init=None), dict(pair=None), dict(node=None),
                     dict(di=None), dict(dp=None), dict(dn=None), dict(ws=None), dict(ws_bytes=need - 1),
                     dict(ws=ctypes.c_void_p(base + 8))])
    assert call(T=-3) == -2 and call(K=65) == -3 and call(pb=-1) == -4 and call(ws_bytes=0) == -12


def test_ragged_vjp_rejects_bad_arguments_on_the_host_in_order():
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_estep_vjp_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, g0=None, g1=None, g2=None, g3=None, di=p, dp=p,
             dn=p, info=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_ragged_estep_vjp_f64(B, T, K, pb, init, pair, node, lengths, g0, g1, g2, g3, di, dp, dn, info,
                                                 ws, ws_bytes, None)

    _in_order(call, [dict(B=-1), dict(T=0), dict(K=0), dict(pb=2), dict(init=None), dict(pair=None), dict(node=None),
                     dict(lengths=None), dict(di=None), dict(dp=None), dict(dn=None), dict(info=None), dict(ws=None),
                     dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(base + 8))])
    assert call(K=65) == -3 and call(ws_bytes=0) == -14


def test_empty_batch_returns_zero_after_the_shared_checks():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, g = lib.svae_hmm_estep_vjp_f64, lib.svae_hmm_ragged_estep_vjp_f64
    n7, n8 = (None,) * 7, (None,) * 8
    assert f(0, 3, 5, 0, p, p, None, *n7, None, 0, None) == 0
    assert f(0, 3, 5, 1, p, p, None, *n7, None, 0, None) == 0
    assert f(0, 0, 5, 0, p, p, None, *n7, None, 0, None) == -2
    assert f(0, 3, 65, 0, p, p, None, *n7, None, 0, None) == -3
    assert f(0, 3, 5, 0, None, p, None, *n7, None, 0, None) == -5
    assert f(0, 3, 5, 0, p, None, None, *n7, None, 0, None) == -6
    assert g(0, 3, 5, 0, p, p, None, None, *n8, None, 0, None) == 0
    assert g(0, 3, 5, 2, p, p, None, None, *n8, None, 0, None) == -4
    assert g(0, 3, 5, 0, p, None, None, None, *n8, None, 0, None) == -6
