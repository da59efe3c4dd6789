"""CPU tests of HMM posterior sampling (svae_hmm_sample_*, include/svae_hip.h): the NumPy oracle
(tests/_hmm_sample_numpy.py) against the exact posterior, the margins of every case the GPU file compares exactly, and
the host side of the C ABI (symbols, workspace closed form, every error code in order)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _hmm_sample_numpy as smp  # noqa: E402
from oracle import hmm_numpy  # noqa: E402

NAMES = ("svae_hmm_sample_workspace_bytes", "svae_hmm_sample_f64", "svae_hmm_ragged_sample_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


# ---- the oracle against the truth ---------------------------------------------------------------------------------------
def test_oracle_samples_have_the_posterior_marginals_and_transition_counts():
    """K = 5, T = 20, B = 2, S = 4096: every cell of the empirical state marginals and of the empirical transition counts
    within 5 binomial standard deviations of hmm_estep's E_states / E_trans (measured for the marginals: worst 3.4)"""
    K, T, B, S = 5, 20, 2, 4096
    rng = np.random.default_rng(5)
    init, pair, node, u = smp.problem(B, T, K, S, rng, 1.0)
    states, logZ, _ = smp.sample_batch(init, pair, node, u)
    assert states.shape == (B, S, T) and states.dtype == np.int32
    for b in range(B):
        lz, (_, E_trans, E_states) = hmm_numpy.hmm_estep((init, pair, node[b]))
        assert logZ[b] == pytest.approx(lz, rel=1e-12)
        freq = np.stack([(states[b] == k).mean(0) for k in range(K)], -1)          # (T,K)
        sd = np.sqrt(E_states * (1 - E_states) / S)
        assert (np.abs(freq - E_states) <= 5 * sd).all(), np.abs((freq - E_states) / sd).max()
        # transition counts: cell (j, k) counts S (T-1) trials of mean probability E_trans[j,k] / (T-1)
        cnt = np.zeros((K, K))
        for t in range(T - 1):
            np.add.at(cnt, (states[b, :, t], states[b, :, t + 1]), 1.0)
        p = E_trans / (T - 1)
        sd = np.sqrt((T - 1) * p * (1 - p) / S)
        assert (np.abs(cnt / S - E_trans) <= 5 * sd).all(), np.abs((cnt / S - E_trans) / sd).max()


# ---- margins: a condition on the inputs of the exact comparisons, not a tolerance of the kernel ----------------------
@pytest.mark.parametrize("K", smp.GRID_K)
def test_margins_of_the_grid(K):
    worst = np.inf
    for T in smp.GRID_T:
        for B in smp.GRID_B:
            for scale in smp.GRID_SCALE:
                worst = min(worst, smp.grid_case(K, T, B, scale)[-1])
    print("grid K=%d worst margin %.3g" % (K, worst))
    assert worst >= smp.MARGIN, worst


@pytest.mark.parametrize("K", smp.PAIR_K)
def test_margins_of_the_batched_pair_and_ragged_cases(K):
    m1, m2 = smp.pair_case(K)[-1], smp.ragged_case(K)[-1]
    print("pair K=%d margin %.3g, ragged %.3g" % (K, m1, m2))
    assert m1 >= smp.MARGIN and m2 >= smp.MARGIN, (m1, m2)


@pytest.mark.parametrize("K", smp.LTR_K)
def test_margins_of_the_left_to_right_cases(K):
    init, pair, node, u, states, logZ, m = smp.ltr_case(K)
    print("left-to-right K=%d margin %.3g" % (K, m))
    assert m >= smp.MARGIN, m
    assert (np.diff(states, axis=2) >= 0).all() and np.isfinite(logZ).all()


def test_oracle_ragged_is_the_cut_sequence_and_never_reads_the_tail():
    init, pair, node, u, L, states, logZ, _ = smp.ragged_case(3)
    for b in (0, 1, 4):
        l = int(L[b])
        st, lz, _ = smp.sample_batch(init, pair[b], node[b:b + 1, :l], u[b:b + 1, :, :l])
        assert np.array_equal(states[b, :, :l], st[0]) and (states[b, :, l:] == -1).all() and logZ[b] == lz[0]
    assert np.isfinite(logZ).all()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def test_sample_symbols_in_header_signatures_and_library_and_abi_number():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s


@pytest.mark.parametrize("K,KP", [(1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)])
def test_sample_workspace_bytes_closed_form(K, KP):
    _, lib = _lib()
    for B, T in ((1, 1), (3, 2), (5, 7), (1, 3), (7, 5), (2048, 500)):
        got = lib.svae_hmm_sample_workspace_bytes(B, T, K)
        assert got == B * T * KP * 8 and got % 16 == 0


def test_sample_workspace_bytes_out_of_range_is_zero():
    _, lib = _lib()
    for B, T, K in ((0, 5, 3), (-1, 5, 3), (2, 0, 3), (2, -4, 3), (2, 5, 0), (2, 5, -1), (2, 5, 65), (2, 5, 1000)):
        assert lib.svae_hmm_sample_workspace_bytes(B, T, K) == 0


def _aligned():
    raw = (ctypes.c_double * 4096)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    return raw, base


def test_sample_rejects_bad_arguments_on_the_host_in_order():
    """every argument error comes back before any HIP call (safe without a GPU); the first failing check wins"""
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)                 # 16-byte aligned host address: must never be dereferenced
    need = lib.svae_hmm_sample_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, S=2, pb=0, init=p, pair=p, node=p, u=p, states=p, logZ=None, ws=p, ws_bytes=need):
        return lib.svae_hmm_sample_f64(B, T, K, S, pb, init, pair, node, u, states, logZ, ws, ws_bytes, None)

    bad = [dict(B=-1), dict(T=0), dict(K=0), dict(pb=2), dict(init=None), dict(pair=None), dict(node=None), dict(S=0),
           dict(u=None), dict(states=None), dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(base + 8))]
    for i, kw in enumerate(bad):
        assert call(**kw) == -(i + 1), kw
        # the first failing check decides: every later argument bad as well
        merged = {}
        for later in bad[i:]:
            merged = {**later, **merged}
        assert call(**merged) == -(i + 1), merged
    assert call(T=-3) == -2 and call(K=65) == -3 and call(pb=-1) == -4 and call(S=-2) == -8 and call(ws_bytes=0) == -12


def test_ragged_sample_rejects_bad_arguments_on_the_host_in_order():
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_sample_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, S=2, pb=0, init=p, pair=p, node=p, lengths=p, u=p, states=p, logZ=None, info=p, ws=p,
             ws_bytes=need):
        return lib.svae_hmm_ragged_sample_f64(B, T, K, S, pb, init, pair, node, lengths, u, states, logZ, info, ws,
                                              ws_bytes, None)

    bad = [dict(B=-1), dict(T=0), dict(K=0), dict(pb=2), dict(init=None), dict(pair=None), dict(node=None),
           dict(lengths=None), dict(S=0), dict(u=None), dict(states=None), dict(info=None), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(base + 8))]
    for i, kw in enumerate(bad):
        assert call(**kw) == -(i + 1), kw
        merged = {}
        for later in bad[i:]:
            merged = {**later, **merged}
        assert call(**merged) == -(i + 1), merged
    assert call(K=65) == -3 and call(S=-1) == -9 and call(ws_bytes=0) == -14


def test_sample_empty_batch_returns_zero_after_the_shared_checks():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, g = lib.svae_hmm_sample_f64, lib.svae_hmm_ragged_sample_f64
    assert f(0, 3, 5, 2, 0, p, p, None, None, None, None, None, 0, None) == 0
    assert f(0, 3, 5, 0, 1, p, p, None, None, None, None, None, 0, None) == 0
    assert f(0, 0, 5, 2, 0, p, p, None, None, None, None, None, 0, None) == -2
    assert f(0, 3, 65, 2, 0, p, p, None, None, None, None, None, 0, None) == -3
    assert f(0, 3, 5, 2, 0, None, p, None, None, None, None, None, 0, None) == -5
    assert f(0, 3, 5, 2, 0, p, None, None, None, None, None, None, 0, None) == -6
    assert g(0, 3, 5, 2, 0, p, p, None, None, None, None, None, None, None, 0, None) == 0
    assert g(0, 3, 5, 2, 2, p, p, None, None, None, None, None, None, None, 0, None) == -4
    assert g(0, 3, 5, 2, 0, p, None, None, None, None, None, None, None, None, 0, None) == -6
