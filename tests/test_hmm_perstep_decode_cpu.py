"""CPU tests of Viterbi decoding and posterior sampling with per-step transition potentials (hmm_viterbi_perstep,
hmm_sample_perstep; svae_hmm_perstep_viterbi_f64, svae_hmm_perstep_sample_f64): the NumPy oracles
(tests/_hmm_perstep_decode_numpy.py) against path enumeration and against the uniform oracles at constant P_t, the margins
of every sampling case the GPU file compares exactly, the C ABI's host-side checks, the Python layer's shape refusals and
the two kernel units' ISA."""
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
import _hmm_perstep_decode_numpy as pd  # noqa: E402
import _hmm_sample_numpy as sm  # noqa: E402
import _hmm_viterbi_numpy as vn  # noqa: E402


# ---- the Viterbi oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T", [(3, 4), (2, 6)])
def test_viterbi_oracle_path_is_a_brute_force_optimum_with_its_score_bit_for_bit(K, T):
    rng = np.random.default_rng(10 * K + T)
    init, pair, node, _ = pd.problem(4, T, K, 1, rng, True, 1.5)
    pair[1, 0][0, 1] = -np.inf                                           # a forbidden transition at one step only
    labels, score = pd.viterbi_perstep(init, pair, node)
    for b in range(4):
        best, paths = pd.brute_force(init, pair[b], node[b])
        assert tuple(labels[b]) in paths
        assert pd.bits(score[b]) == pd.bits(best)
        assert pd.bits(pd.path_score(init, pair[b], node[b], labels[b])) == pd.bits(best)


@pytest.mark.parametrize("K,T", [(3, 4), (2, 6)])
def test_viterbi_oracle_on_integer_potentials_meets_ties_and_keeps_the_best_score(K, T):
    rng = np.random.default_rng(40 + K)
    init, pair, node = pd.tie_problem(6, T, K, rng)
    labels, score = pd.viterbi_perstep(init, pair, node)
    tied = 0
    for b in range(6):
        best, paths = pd.brute_force(init, pair[b], node[b])
        tied += len(paths) > 1 and np.isfinite(best)
        assert score[b] == best
        if np.isfinite(best):
            assert tuple(labels[b]) in paths
    assert tied > 0                                                      # brute force found more than one optimal path


@pytest.mark.parametrize("K", [1, 3, 17])
def test_viterbi_oracle_equals_the_uniform_oracle_at_constant_matrices(K):
    rng = np.random.default_rng(50 + K)
    B, T = 4, 9
    init, pair, node, _ = sm.problem(B, T, K, 1, rng, 1.5, batched_pair=True)
    per = np.broadcast_to(pair[:, None], (B, T - 1, K, K)).copy()
    a, b = pd.viterbi_perstep(init, per, node), vn.viterbi_batch(init, pair, node)
    assert np.array_equal(a[0], b[0]) and np.array_equal(pd.bits(a[1]), pd.bits(b[1]))
    shared = pd.viterbi_perstep(init, per[0], node)
    ref = vn.viterbi_batch(init, pair[0], node)
    assert np.array_equal(shared[0], ref[0]) and np.array_equal(pd.bits(shared[1]), pd.bits(ref[1]))


# ---- the sampling oracle ----------------------------------------------------------------------------------------------------
def test_sampling_oracle_statistics_against_the_enumeration_of_all_paths():
    K, T, N = 3, 4, 4096
    rng = np.random.default_rng(77)
    init, pair, node, u = pd.problem(1, T, K, N, rng, False, 1.5)
    pair[1][0, 2] = -np.inf
    states, logZ, _ = pd.sample_perstep(init, pair, node, u)
    bz = pd.ps.brute_force((init, pair, node[0]))[0]
    assert abs(logZ[0] - bz) < 1e-12
    pd.statistics_within_5_sigma(states[0], (init, pair, node[0]))
    assert not ((states[0][:, 1] == 0) & (states[0][:, 2] == 2)).any()   # the forbidden transition is never drawn


@pytest.mark.parametrize("K", sm.PAIR_K)
def test_sampling_oracle_equals_the_uniform_oracle_at_constant_matrices(K):
    init, pair, node, u, states, logZ, margin = sm.pair_case(K)
    B, T = node.shape[:2]
    per = np.broadcast_to(pair[:, None], (B, T - 1, K, K))
    st, lz, mg = pd.sample_perstep(init, per, node, u)
    assert np.array_equal(st, states)
    np.testing.assert_allclose(lz, logZ, rtol=1e-13, atol=1e-13)
    assert margin >= pd.MARGIN and mg >= pd.MARGIN


# ---- the margins of every sampling case the GPU file compares label for label -----------------------------------------------
@pytest.mark.parametrize("K", pd.GRID_K)
def test_grid_cases_have_their_margin(K):
    cases = pd.grid_cases(K)
    assert len(cases) == len(pd.GRID_T) * len(pd.GRID_B) * 2
    worst = min(c.margin for c in cases)
    print("K = %d: worst margin %.3g" % (K, worst))
    assert worst >= pd.MARGIN
    assert all(np.isfinite(c.logZ).all() for c in cases)


@pytest.mark.parametrize("K", pd.LTR_K)
def test_left_to_right_cases_have_their_margin_and_non_decreasing_paths(K):
    c = pd.ltr_case(K)
    print("K = %d: margin %.3g" % (K, c.margin))
    assert c.margin >= pd.MARGIN and np.isfinite(c.logZ).all()
    assert (np.diff(c.states, axis=-1) >= 0).all()
    assert (np.diff(c.labels, axis=-1) >= 0).all()
    lo, hi, rel = pd.extreme_draws(*c.natparam)                          # what the GPU file expects of u = 0 and u = 1
    print("K = %d: smallest weight of a highest allowed state, relative to the total: %.3g" % (K, rel))
    assert rel >= pd.MARGIN and (lo <= hi).all() and (np.diff(hi, axis=-1) >= 0).all()


@pytest.mark.parametrize("K", [3, 8, 16, 17, 33, 64])
def test_ragged_cases_have_their_margin(K):
    r = pd.ragged_case(K)
    assert r["margin"] >= pd.MARGIN and r["shared"][1][2] >= pd.MARGIN
    for b, L in enumerate(r["L"]):
        assert (r["states"][b, :, L:] == -1).all() and (r["states"][b, :, :L] >= 0).all()
        assert (r["labels"][b, L:] == -1).all() and (r["labels"][b, :L] >= 0).all()


@pytest.mark.parametrize("K", pd.TIE_K)
def test_tie_cases_hold_ties(K):
    """a sequence of the case meets a step at which two source states attain the maximum exactly"""
    c = pd.tie_case(K)
    init, pair, node = c.natparam
    delta = init[None] + node[:, 0]
    ties = 0
    for t in range(1, node.shape[1]):
        v = delta[:, :, None] + pair[:, t - 1]
        best = v.max(1)
        ties += int((((v == best[:, None]) & np.isfinite(v)).sum(1) > 1).sum())
        delta = best + node[:, t]
    assert ties > 0
    for b in range(node.shape[0]):
        assert pd.bits(pd.path_score(init, pair[b], node[b], c.labels[b])) == pd.bits(c.score[b])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ("svae_hmm_perstep_viterbi_f64", "svae_hmm_perstep_sample_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_decode_symbols_in_header_signatures_and_library_and_the_abi_number_stays():
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


def test_perstep_viterbi_rejects_bad_arguments_on_the_host():
    """every documented code comes back before any HIP call: the pointers are host addresses that are never dereferenced"""
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_viterbi_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, states=p, score=p, info=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_perstep_viterbi_f64(B, T, K, pb, init, pair, node, lengths, states, score, info, ws, ws_bytes,
                                                None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(states=None) == -8
    assert call(info=None) == -9
    assert call(ws=None) == -10
    assert call(ws_bytes=need - 1) == -11 and call(ws_bytes=0) == -11
    assert call(ws=ctypes.c_void_p(base + 8)) == -12
    for K in (17, 64):
        assert call(K=K, ws_bytes=lib.svae_hmm_viterbi_workspace_bytes(2, 3, K) - 1) == -11
    assert call(T=1, pair=None, node=None) == -7                         # T = 1 reads no pair parameters
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(pb=2, init=None) == -4 and call(init=None, pair=None, node=None) == -5
    assert call(pair=None, node=None) == -6 and call(node=None, states=None, ws=None) == -7
    assert call(states=None, info=None) == -8 and call(info=None, ws=None) == -9
    assert call(ws=None, ws_bytes=0) == -10 and call(ws=ctypes.c_void_p(base + 8), ws_bytes=0) == -11
    # B = 0 returns 0 after the shared checks
    n = None
    v = lib.svae_hmm_perstep_viterbi_f64
    assert v(0, 3, 5, 0, p, p, n, n, n, n, n, n, 0, None) == 0
    assert v(0, 1, 5, 1, p, n, n, n, n, n, n, n, 0, None) == 0
    assert v(0, 0, 5, 0, p, p, n, n, n, n, n, n, 0, None) == -2
    assert v(0, 3, 65, 0, p, p, n, n, n, n, n, n, 0, None) == -3
    assert v(0, 3, 5, 3, p, p, n, n, n, n, n, n, 0, None) == -4
    assert v(0, 3, 5, 0, n, p, n, n, n, n, n, n, 0, None) == -5
    assert v(0, 3, 5, 0, p, n, n, n, n, n, n, n, 0, None) == -6


def test_perstep_sample_rejects_bad_arguments_on_the_host():
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_perstep_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, S=2, pb=0, init=p, pair=p, node=p, lengths=p, u=p, states=p, logZ=p, info=p, ws=p,
             ws_bytes=need):
        return lib.svae_hmm_perstep_sample_f64(B, T, K, S, pb, init, pair, node, lengths, u, states, logZ, info, ws,
                                               ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(S=0) == -8 and call(S=-2) == -8
    assert call(u=None) == -9
    assert call(states=None) == -10
    assert call(info=None) == -11
    assert call(ws=None) == -12
    assert call(ws_bytes=need - 1) == -13 and call(ws_bytes=0) == -13
    assert call(ws=ctypes.c_void_p(base + 8)) == -14
    for K in (17, 64):
        assert call(K=K, ws_bytes=lib.svae_hmm_perstep_workspace_bytes(2, 3, K) - 1) == -13
    assert call(T=1, pair=None, node=None) == -7
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(pb=2, init=None) == -4 and call(init=None, pair=None, node=None) == -5
    assert call(pair=None, node=None) == -6 and call(node=None, S=0, u=None) == -7
    assert call(S=0, u=None) == -8 and call(u=None, states=None) == -9 and call(states=None, info=None) == -10
    assert call(info=None, ws=None) == -11 and call(ws=None, ws_bytes=0) == -12
    assert call(ws=ctypes.c_void_p(base + 8), ws_bytes=0) == -13
    n = None
    s = lib.svae_hmm_perstep_sample_f64
    assert s(0, 3, 5, 2, 0, p, p, n, n, n, n, n, n, n, 0, None) == 0
    assert s(0, 3, 5, 0, 0, p, p, n, n, n, n, n, n, n, 0, None) == 0     # (S is checked after the empty batch returns)
    assert s(0, 1, 5, 2, 1, p, n, n, n, n, n, n, n, n, 0, None) == 0
    assert s(0, 0, 5, 2, 0, p, p, n, n, n, n, n, n, n, 0, None) == -2
    assert s(0, 3, 65, 2, 0, p, p, n, n, n, n, n, n, n, 0, None) == -3
    assert s(0, 3, 5, 2, 3, p, p, n, n, n, n, n, n, n, 0, None) == -4
    assert s(0, 3, 5, 2, 0, n, p, n, n, n, n, n, n, n, 0, None) == -5
    assert s(0, 3, 5, 2, 0, p, n, n, n, n, n, n, n, n, 0, None) == -6


# ---- Python: refusals from shapes alone (nothing here touches a device) -----------------------------------------------------
def test_decode_python_refuses_bad_shapes_before_touching_the_device():
    from svae_amd.hmm import hmm_inference as H
    from svae_amd import hmm as pkg
    assert pkg.hmm_viterbi_perstep is H.hmm_viterbi_perstep and pkg.hmm_sample_perstep is H.hmm_sample_perstep
    z = np.zeros
    B, T, K = 3, 4, 5
    good = (z(K), z((T - 1, K, K)), z((B, T, K)))
    for fn in (H.hmm_viterbi_perstep, H.hmm_sample_perstep):
        with pytest.raises(ValueError, match="K=65"):
            fn((z(65), z((T - 1, 65, 65)), z((T, 65))))
        with pytest.raises(ValueError, match="K=0"):
            fn((z(0), z((T - 1, 0, 0)), z((T, 0))))
        with pytest.raises(ValueError, match="T-1"):
            fn((z(K), z((T, K, K)), z((T, K))))
        with pytest.raises(ValueError, match="T-1"):
            fn((z(K), z((B, T - 2, K, K)), z((B, T, K))))
        with pytest.raises(ValueError, match="batch"):
            fn((z(K), z((B + 1, T - 1, K, K)), z((B, T, K))))
        with pytest.raises(ValueError, match="need batched"):
            fn((z(K), z((B, T - 1, K, K)), z((T, K))))
        with pytest.raises(ValueError, match="per-step"):
            fn((z(K), z((K, K)), z((T, K))))                             # the uniform function's pair parameter
        with pytest.raises(ValueError):
            fn((z(K + 1), z((T - 1, K, K)), z((T, K))))
        with pytest.raises(ValueError):
            fn((z(K), z((T - 1, K, K + 1)), z((T, K))))
        with pytest.raises(ValueError):
            fn((z(K), z((T - 1, K, K)), z(K)))
        with pytest.raises(ValueError, match="no steps"):
            fn((z(K), z((0, K, K)), z((0, K))))
        with pytest.raises(ValueError, match="shape"):
            fn(good, lengths=np.ones(B + 1, np.int64))
        with pytest.raises(ValueError, match="integers"):
            fn(good, lengths=np.ones(B))
        with pytest.raises(ValueError, match="batched"):
            fn((z(K), z((T - 1, K, K)), z((T, K))), lengths=np.ones(1, np.int64))
    S = H.hmm_sample_perstep
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="num_samples"):
            S(good, num_samples=bad)
    with pytest.raises(ValueError, match="u must have shape"):
        S(good, num_samples=2, u=z((B, 3, T)))
    with pytest.raises(ValueError, match="u must have shape"):
        S(good, num_samples=2, u=z((2, T)))                              # the unbatched shape with batched nodes
    with pytest.raises(ValueError, match="u must have shape"):
        S((z(K), z((T - 1, K, K)), z((T, K))), num_samples=2, u=z((1, 2, T)))

    class Shape:                                                         # shapes alone: nothing of this size is allocated
        def __init__(self, *s):
            self.shape = s

    with pytest.raises(ValueError, match="2\\^31"):
        S((Shape(4), Shape(1 << 12, 4, 4), Shape(1 << 10, (1 << 12) + 1, 4)), num_samples=1 << 9)


# ---- the kernel units -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,short,kernels", [("hmm_viterbi_perstep", "viterbi_perstep.s", 4),
                                                ("hmm_sample_perstep", "sample_perstep.s", 8)])
def test_decode_units_compile_for_gfx950_without_scratch(tmp_path, unit, short, kernels):
    import audit_dpp_hazards
    s = tmp_path / (unit + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", str(s)], check=True, cwd=CSRC)
    isa = s.read_text()
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == kernels and set(sizes) == {"0"}, sizes          # one per group width (the sampler: filter and draw)
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == kernels and set(spills) == {"0"}, spills
    ops = {w[0] for w in (l.split(";")[0].split() for l in isa.splitlines()) if w}
    assert "global_atomic_or" in ops                                     # the status word: a vector atomic
    _, findings = audit_dpp_hazards.audit(str(s))
    assert findings == [], findings[:5]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert unit + ".o" in mk and short in mk                             # in OBJS and in the audit target
