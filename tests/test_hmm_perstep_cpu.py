"""CPU tests of the HMM E-step with per-step transition potentials (svae_hmm_perstep_estep_f64, hmm_estep_perstep): its
NumPy oracle (tests/_hmm_perstep_numpy.py) against path enumeration, against oracle/hmm_numpy at constant P_t and by the
marginal identities; the C ABI's host-side checks; the Python layer's shape refusals; and the kernel unit's ISA."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _hmm_perstep_numpy as ps  # noqa: E402
from oracle import hmm_numpy  # noqa: E402  (checker only)


def _problem(T, K, rng, scale=1.0):
    init = np.log(rng.dirichlet(np.ones(K)))
    pair = np.log(rng.dirichlet(np.ones(K), size=(max(T - 1, 0), K))) + 0.5 * rng.standard_normal((max(T - 1, 0), K, K))
    node = scale * rng.standard_normal((T, K))
    return init, pair, node


# ---- the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T", [(3, 4), (2, 6)])
def test_oracle_against_enumeration_of_all_paths(K, T):
    rng = np.random.default_rng(10 * K + T)
    init, pair, node = _problem(T, K, rng, 1.5)
    pair[1] += 7.0                                                       # a step at another offset
    pair[0][0, 1] = -np.inf                                              # a forbidden transition at one step only
    for L in [None] + list(range(1, T + 1)):
        lz, (ei, et, es) = ps.hmm_estep_perstep((init, pair, node), L)
        bz, (bi, bt, bs) = ps.brute_force((init, pair, node), L)
        assert abs(lz - bz) < 1e-12
        for a, b in ((ei, bi), (et, bt), (es, bs)):
            assert a.shape == b.shape and np.abs(a - b).max() < 1e-12
        cut = T if L is None else L
        assert (es[cut:] == 0).all() and (et[cut - 1:] == 0).all()


@pytest.mark.parametrize("K,T", [(1, 1), (4, 1), (3, 9), (17, 6)])
def test_oracle_reduces_to_the_uniform_oracle_at_constant_matrices(K, T):
    rng = np.random.default_rng(100 + K + T)
    init, pair, node = _problem(T, K, rng)
    P = np.log(rng.dirichlet(np.ones(K), size=K)) + 0.3 * rng.standard_normal((K, K))
    pair = np.broadcast_to(P, (T - 1, K, K)).copy()
    lz, (ei, et, es) = ps.hmm_estep_perstep((init, pair, node))
    uz, (ui, ut, us) = hmm_numpy.hmm_estep((init, P, node))
    assert lz == pytest.approx(uz, rel=1e-13, abs=1e-13)
    np.testing.assert_allclose(ei, ui, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(es, us, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(et.sum(0), ut, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("L", [None, 1, 2, 6, 7])
def test_oracle_pair_marginals_sum_to_the_state_marginals(L):
    T, K = 7, 5
    rng = np.random.default_rng(7)
    init, pair, node = _problem(T, K, rng, 2.0)
    pair[3][np.tril_indices(K, -1)] = -np.inf                           # left-to-right at one step
    lz, (ei, et, es) = ps.hmm_estep_perstep((init, pair, node), L)
    cut = T if L is None else L
    assert np.isfinite(lz)
    np.testing.assert_allclose(es[:cut].sum(-1), 1.0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(et[:cut - 1].sum(2), es[:cut - 1], rtol=0, atol=1e-13)
    np.testing.assert_allclose(et[:cut - 1].sum(1), es[1:cut], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(ei, es[0])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ("svae_hmm_perstep_workspace_bytes", "svae_hmm_perstep_estep_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_perstep_symbols_in_header_signatures_and_library_and_the_abi_number_stays():
    L, lib = _lib()
    raw = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", raw)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15


def _aligned():
    raw = (ctypes.c_double * 1024)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    return raw, base


def test_perstep_estep_rejects_bad_arguments_on_the_host():
    """every documented code comes back before any HIP call (safe without a GPU): the pointers are host addresses that
    must never be dereferenced"""
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_perstep_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, logZ=p, Ei=p, Et=p, Es=p, info=p, ws=p,
             ws_bytes=need):
        return lib.svae_hmm_perstep_estep_f64(B, T, K, pb, init, pair, node, lengths, logZ, Ei, Et, Es, info, ws, ws_bytes,
                                              None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(logZ=None) == -8
    assert call(Ei=None) == -9
    assert call(Es=None) == -10
    assert call(info=None) == -11
    assert call(ws=None) == -12
    assert call(ws_bytes=need - 1) == -13 and call(ws_bytes=0) == -13
    assert call(ws=ctypes.c_void_p(base + 8)) == -14
    for K in (17, 64):
        assert call(K=K, ws_bytes=lib.svae_hmm_perstep_workspace_bytes(2, 3, K) - 1) == -13
    # T = 1 reads no pair parameters: a NULL pair pointer passes that check (and the next failing one decides)
    assert call(T=1, pair=None, node=None) == -7
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(init=None, pair=None, node=None) == -5 and call(node=None, logZ=None, ws=None) == -7
    assert call(Ei=None, Es=None, info=None) == -9 and call(info=None, ws=None) == -11
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(node=None),
             call(logZ=None), call(Ei=None), call(Es=None), call(info=None), call(ws=None), call(ws_bytes=0),
             call(ws=ctypes.c_void_p(base + 8))}
    assert len(codes) == 14 and all(-100 < c < 0 for c in codes)        # one distinct code per bad argument


def test_perstep_empty_batch_returns_zero_after_the_shared_checks():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    e, n = lib.svae_hmm_perstep_estep_f64, None
    assert e(0, 3, 5, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == 0
    assert e(0, 3, 5, 1, p, p, p, p, p, p, p, p, p, p, 0, None) == 0
    assert e(0, 1, 5, 0, p, n, n, n, n, n, n, n, n, n, 0, None) == 0
    assert e(0, 0, 5, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == -2
    assert e(0, 3, 65, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == -3
    assert e(0, 3, 5, 3, p, p, n, n, n, n, n, n, n, n, 0, None) == -4
    assert e(0, 3, 5, 0, n, p, n, n, n, n, n, n, n, n, 0, None) == -5
    assert e(0, 3, 5, 0, p, n, n, n, n, n, n, n, n, n, 0, None) == -6


def test_perstep_workspace_bytes_is_monotone_and_holds_the_records():
    _, lib = _lib()
    f = lib.svae_hmm_perstep_workspace_bytes
    for K in (1, 8, 16, 17, 33, 64):
        prev = 0
        for B in (1, 2, 5, 64, 1000):
            row = [f(B, T, K) for T in (1, 2, 3, 50, 500)]
            assert all(a <= b for a, b in zip(row, row[1:])), (K, B, row)
            assert row[0] >= prev
            prev = row[0]
            for T, r in zip((1, 2, 3, 50, 500), row):
                assert r >= B * T * K * 8 and r % 16 == 0
        assert f(1000, 500, K) > f(1, 1, K)
    assert f(0, 3, 5) == 0 and f(2, 0, 5) == 0 and f(2, 3, 0) == 0 and f(2, 3, 65) == 0
    assert f(1 << 20, 4096, 64) == (1 << 20) * 4096 * 64 * 8            # past 2^31 and 2^32 bytes


# ---- Python: refusals from shapes alone (nothing here touches a device) -----------------------------------------------------
def test_perstep_python_refuses_bad_shapes_before_touching_the_device():
    from svae_amd.hmm import hmm_inference as H
    z = np.zeros
    B, T, K = 3, 4, 5
    good = (z(K), z((T - 1, K, K)), z((B, T, K)))
    for fn in (H.hmm_estep_perstep, H.hmm_logZ_perstep):
        with pytest.raises(ValueError, match="K=65"):
            fn((z(65), z((T - 1, 65, 65)), z((T, 65))))
        with pytest.raises(ValueError, match="K=0"):
            fn((z(0), z((T - 1, 0, 0)), z((T, 0))))
        with pytest.raises(ValueError, match="T-1"):
            fn((z(K), z((T, K, K)), z((T, K))))                          # T matrices for T steps
        with pytest.raises(ValueError, match="T-1"):
            fn((z(K), z((B, T - 2, K, K)), z((B, T, K))))
        with pytest.raises(ValueError, match="batch"):
            fn((z(K), z((B + 1, T - 1, K, K)), z((B, T, K))))
        with pytest.raises(ValueError, match="need batched"):
            fn((z(K), z((B, T - 1, K, K)), z((T, K))))                   # a 4-d pair with 2-d nodes
        with pytest.raises(ValueError):
            fn((z(K), z((K, K)), z((T, K))))                             # the uniform function's pair parameter
        with pytest.raises(ValueError):
            fn((z(K + 1), z((T - 1, K, K)), z((T, K))))
        with pytest.raises(ValueError):
            fn((z(K), z((T - 1, K, K + 1)), z((T, K))))
        with pytest.raises(ValueError):
            fn((z(K), z((T - 1, K, K)), z(K)))
        with pytest.raises(ValueError, match="shape"):
            fn(good, lengths=np.ones(B + 1, np.int64))
        with pytest.raises(ValueError, match="shape"):
            fn(good, lengths=np.ones((B, 1), np.int64))
        with pytest.raises(ValueError, match="integers"):
            fn(good, lengths=np.ones(B))
        with pytest.raises(ValueError, match="batched"):
            fn((z(K), z((T - 1, K, K)), z((T, K))), lengths=np.ones(1, np.int64))
    import torch
    with pytest.raises(ValueError, match="integers"):
        H.hmm_estep_perstep(good, lengths=torch.ones(B))
    with pytest.raises(ValueError, match="T-1"):
        H.hmm_logZ_perstep_differentiable((torch.zeros(K), torch.zeros(T, K, K), torch.zeros(T, K)))


# ---- the kernel unit --------------------------------------------------------------------------------------------------------
def test_perstep_unit_compiles_for_gfx950_without_scratch(tmp_path):
    import audit_dpp_hazards
    s = tmp_path / "hmm_estep_perstep.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "hmm_estep_perstep.hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "hmm_perstep_kernel" in l]
    assert len(names) == 4, names                                        # groups of 8, 16, 32 and 64 lanes
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 4 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == 4 and set(spills) == {"0"}, spills
    ops = {w[0] for w in (l.split(";")[0].split() for l in isa.splitlines()) if w}
    assert "global_atomic_or" in ops                                     # the status word: a vector atomic
    _, findings = audit_dpp_hazards.audit(str(s))                        # (no inline-asm DPP here; the audit still has to pass)
    assert findings == [], findings[:5]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hmm_estep_perstep.o" in mk and "estep_perstep.s" in mk       # in OBJS and in the audit target
