"""CPU tests of the HMM Viterbi entry (svae_hmm_viterbi_*, include/svae_hip.h): symbols, the workspace closed form,
host-side argument checks, the ISA of the kernel unit, and the NumPy restatement of the defined arithmetic
(tests/_hmm_viterbi_numpy.py) against a brute-force enumeration of every path."""
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

import _hmm_viterbi_numpy as vit  # noqa: E402

NAMES = ("svae_hmm_viterbi_workspace_bytes", "svae_hmm_viterbi_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_viterbi_symbols_in_header_signatures_and_library():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s


@pytest.mark.parametrize("K,KP", [(1, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64)])
def test_viterbi_workspace_bytes_closed_form(K, KP):
    _, lib = _lib()
    for B, T in ((1, 1), (3, 2), (5, 7), (1, 3), (7, 5), (2048, 500)):
        want = B * T * KP
        want = (want + 7) // 8 * 8
        assert lib.svae_hmm_viterbi_workspace_bytes(B, T, K) == want
        assert want % 8 == 0 and want >= B * T * KP


def test_viterbi_workspace_bytes_out_of_range_is_zero():
    _, lib = _lib()
    for B, T, K in ((0, 5, 3), (-1, 5, 3), (2, 0, 3), (2, -4, 3), (2, 5, 0), (2, 5, -1), (2, 5, 65), (2, 5, 1000)):
        assert lib.svae_hmm_viterbi_workspace_bytes(B, T, K) == 0


def test_viterbi_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU)"""
    _, lib = _lib()
    raw = (ctypes.c_double * 1024)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    p = ctypes.c_void_p(base)                 # 16-byte aligned host address: must never be dereferenced
    need = lib.svae_hmm_viterbi_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, states=p, score=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_viterbi_f64(B, T, K, pb, init, pair, node, states, score, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(states=None) == -8
    assert call(ws=None) == -10
    assert call(ws_bytes=need - 1) == -11 and call(ws_bytes=0) == -11
    assert call(ws=ctypes.c_void_p(base + 8)) == -12
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(init=None, pair=None, node=None) == -5 and call(node=None, states=None, ws=None) == -7
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(node=None),
             call(states=None), call(ws=None), call(ws_bytes=0), call(ws=ctypes.c_void_p(base + 8))}
    assert len(codes) == 11 and all(-100 < c < 0 for c in codes)     # one distinct code per bad argument


def test_viterbi_empty_batch_returns_zero_after_the_shared_checks():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.svae_hmm_viterbi_f64
    assert f(0, 3, 5, 0, p, p, None, None, None, None, 0, None) == 0
    assert f(0, 3, 5, 1, p, p, p, p, p, p, 0, None) == 0
    assert f(0, 0, 5, 0, p, p, None, None, None, None, 0, None) == -2
    assert f(0, 3, 65, 0, p, p, None, None, None, None, 0, None) == -3
    assert f(0, 3, 5, 0, None, p, None, None, None, None, 0, None) == -5
    assert f(0, 3, 5, 0, p, None, None, None, None, None, 0, None) == -6


def test_viterbi_unit_compiles_without_scratch_and_without_dpp_hazards(tmp_path):
    """every instance (K = 1..16 rows, KP = 32 and 64 wavefronts): no private segment, no scratch instruction, no
    fp64 multiply or FMA, and the DPP hazard audit passes"""
    s = tmp_path / "viterbi.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "hmm_viterbi.hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "hmm_viterbi" in l]
    assert sum("hmm_viterbi_row_kernel" in n for n in names) == 16, names
    assert sum("hmm_viterbi_wide_kernel" in n for n in names) == 2, names
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 18 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert spills and set(spills) == {"0"}, spills
    ops = {w[0] for w in (l.split(";")[0].split() for l in isa.splitlines()) if w}
    assert "v_fma_f64" not in ops and "v_mul_f64" not in ops          # adds and compares only: nothing to contract
    audit = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(s)],
                           capture_output=True, text=True)
    assert audit.returncode == 0, audit.stdout + audit.stderr
    flags = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in flags and "-Ofast" not in flags          # the definition is exact only without it
    assert "hmm_viterbi.o" in flags and "viterbi.s" in flags           # in OBJS and in the audit target


def test_numpy_restatement_equals_brute_force_enumeration():
    """all K <= 4, T <= 6 on seeded random potentials: scores exactly; labels wherever the maximum is unique"""
    rng = np.random.default_rng(20240611)
    cases = compared = 0
    for K in range(1, 5):
        for T in range(1, 7):
            for rep in range(3):
                scale = (1.0, 7.0, 50.0)[rep]
                init = scale * rng.standard_normal(K)
                pair = scale * rng.standard_normal((K, K))
                node = scale * rng.standard_normal((T, K))
                labels, score = vit.viterbi(init, pair, node)
                best, paths = vit.brute_force(init, pair, node)
                cases += 1
                assert vit.bits(score) == vit.bits(best), (K, T, rep)
                assert vit.bits(vit.path_score(init, pair, node, labels)) == vit.bits(score)
                assert labels.dtype == np.int32 and labels.shape == (T,)
                if len(paths) == 1:
                    compared += 1
                    assert tuple(int(x) for x in labels) == paths[0], (K, T, rep)
                else:
                    assert tuple(int(x) for x in labels) in paths
    assert cases == 72 and compared >= 0.95 * cases, (compared, cases)


def test_numpy_restatement_ties_and_minus_infinity():
    K, T = 3, 5
    z = np.zeros
    labels, score = vit.viterbi(z(K), z((K, K)), z((T, K)))
    assert labels.tolist() == [0] * T and score == 0.0
    node = z((T, K))
    node[2] = -np.inf                                                   # a forbidden step: score -inf, lowest indices
    labels, score = vit.viterbi(z(K), z((K, K)), node)
    assert score == -np.inf and labels.tolist() == [0] * T
    pair = np.where(np.tril(np.ones((K, K)), -1) > 0, -np.inf, 0.0)      # left-to-right
    node = np.array([[0, -5, -5], [-5, 0, -5], [0, -9, -9], [-5, -5, 0], [-5, 0, -5.0]])
    labels, _ = vit.viterbi(z(K), pair, node)
    assert (np.diff(labels) >= 0).all()

