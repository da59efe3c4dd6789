"""CPU tests of the per-sequence-length HMM entries (svae_hmm_ragged_estep_f64, svae_hmm_ragged_viterbi_f64,
include/svae_hip.h): symbols, the unchanged ABI number, host-side argument checks, and the metadata of the kernel units
(kernel counts, private segments, spills, fp64 multiplies in the Viterbi unit, the DPP hazard audit)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

NAMES = ("svae_hmm_ragged_estep_f64", "svae_hmm_ragged_viterbi_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_ragged_symbols_in_header_signatures_and_library():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s


def test_abi_version_is_still_15():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15


def _aligned():
    raw = (ctypes.c_double * 1024)()
    base = ctypes.addressof(raw)
    base += (-base) % 16
    return raw, base


def test_ragged_estep_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU): the pointers are host addresses that
    must never be dereferenced"""
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, logZ=p, Ei=p, Et=p, Es=p, info=p, ws=p,
             ws_bytes=need):
        return lib.svae_hmm_ragged_estep_f64(B, T, K, pb, init, pair, node, lengths, logZ, Ei, Et, Es, info, ws, ws_bytes,
                                             None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(lengths=None) == -8
    assert call(logZ=None) == -9
    assert call(Ei=None) == -10
    assert call(Et=None) == -11
    assert call(Es=None) == -12
    assert call(info=None) == -13
    assert call(ws=None) == -14
    assert call(ws_bytes=need - 1) == -15 and call(ws_bytes=0) == -15
    for K in (17, 64):                                                  # the wide records
        need_k = lib.svae_hmm_workspace_bytes(2, 3, K)
        assert call(K=K, ws_bytes=need_k - 1) == -15
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(init=None, pair=None, node=None) == -5 and call(node=None, lengths=None, info=None) == -7
    assert call(lengths=None, info=None, ws=None) == -8 and call(info=None, ws=None) == -13
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(node=None),
             call(lengths=None), call(logZ=None), call(Ei=None), call(Et=None), call(Es=None), call(info=None),
             call(ws=None), call(ws_bytes=0)}
    assert len(codes) == 15 and all(-100 < c < 0 for c in codes)       # one distinct code per bad argument


def test_ragged_viterbi_rejects_bad_arguments_on_the_host():
    _, lib = _lib()
    raw, base = _aligned()
    p = ctypes.c_void_p(base)
    need = lib.svae_hmm_viterbi_workspace_bytes(2, 3, 5)

    def call(B=2, T=3, K=5, pb=0, init=p, pair=p, node=p, lengths=p, states=p, score=p, info=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_ragged_viterbi_f64(B, T, K, pb, init, pair, node, lengths, states, score, info, ws, ws_bytes,
                                               None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(node=None) == -7
    assert call(lengths=None) == -8
    assert call(states=None) == -9
    assert call(info=None) == -10
    assert call(ws=None) == -11
    assert call(ws_bytes=need - 1) == -12 and call(ws_bytes=0) == -12
    assert call(ws=ctypes.c_void_p(base + 8)) == -13
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=65, init=None) == -3
    assert call(init=None, pair=None, node=None) == -5 and call(node=None, lengths=None, ws=None) == -7
    assert call(lengths=None, states=None, info=None) == -8 and call(info=None, ws=None) == -10
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(node=None),
             call(lengths=None), call(states=None), call(info=None), call(ws=None), call(ws_bytes=0),
             call(ws=ctypes.c_void_p(base + 8))}
    assert len(codes) == 13 and all(-100 < c < 0 for c in codes)


def test_ragged_empty_batch_returns_zero_after_the_shared_checks():
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    e, v = lib.svae_hmm_ragged_estep_f64, lib.svae_hmm_ragged_viterbi_f64
    n = None
    assert e(0, 3, 5, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == 0
    assert e(0, 3, 5, 1, p, p, p, p, p, p, p, p, p, p, 0, None) == 0
    assert e(0, 0, 5, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == -2
    assert e(0, 3, 65, 0, p, p, n, n, n, n, n, n, n, n, 0, None) == -3
    assert e(0, 3, 5, 3, p, p, n, n, n, n, n, n, n, n, 0, None) == -4
    assert e(0, 3, 5, 0, n, p, n, n, n, n, n, n, n, n, 0, None) == -5
    assert e(0, 3, 5, 0, p, n, n, n, n, n, n, n, n, n, 0, None) == -6
    assert v(0, 3, 5, 0, p, p, n, n, n, n, n, n, 0, None) == 0
    assert v(0, 3, 5, 1, p, p, p, p, p, p, p, p, 0, None) == 0
    assert v(0, 0, 5, 0, p, p, n, n, n, n, n, n, 0, None) == -2
    assert v(0, 3, 65, 0, p, p, n, n, n, n, n, n, 0, None) == -3
    assert v(0, 3, 5, 0, n, p, n, n, n, n, n, n, 0, None) == -5
    assert v(0, 3, 5, 0, p, n, n, n, n, n, n, n, 0, None) == -6


# ---- ISA metadata of the kernel units ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """the three units' gfx950 assembly, compiled concurrently on first use"""
    d = tmp_path_factory.mktemp("hmm_ragged_asm")
    jobs = {}
    for unit in ("hmm_viterbi_ragged", "hmm_estep", "hmm_estep_wide"):
        out = d / (unit + ".s")
        log = open(str(out) + ".log", "wb")
        jobs[unit] = (subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                                        "-S", os.path.join(CSRC, unit + ".hip"), "-o", str(out)],
                                       stdout=log, stderr=subprocess.STDOUT, cwd=CSRC), out)

    def get(unit):
        proc, out = jobs[unit]
        assert proc.wait() == 0, open(str(out) + ".log").read()[-2000:]
        return out
    yield get
    for proc, _ in jobs.values():
        if proc.poll() is None:
            proc.kill()


def _kernel_meta(text, key):
    """{kernel name: value of `key`} from the amdhsa.kernels metadata"""
    out, name = {}, None
    for l in text.splitlines():
        s = l.strip()
        if s.startswith(".name:"):                       # (keys are sorted: a kernel's .name is the last one before `key`)
            name = s.split()[-1]
        elif s.startswith(key + ":"):
            out[name] = int(s.split()[-1])
    return out


def _audit(path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_viterbi_unit_has_18_kernels_no_scratch_no_fp64_multiply(isa):
    s = isa("hmm_viterbi_ragged")
    text = s.read_text()
    names = [l.split()[-1] for l in text.splitlines() if l.strip().startswith(".name:") and "hmm_viterbi" in l]
    assert sum("hmm_viterbi_row_kernel" in n for n in names) == 16, names
    assert sum("hmm_viterbi_wide_kernel" in n for n in names) == 2, names
    assert len(names) == 18
    sizes = [l.split()[-1] for l in text.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 18 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in text.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == 18 and set(spills) == {"0"}, spills
    ops = {w[0] for w in (l.split(";")[0].split() for l in text.splitlines()) if w}
    assert "v_fma_f64" not in ops and "v_mul_f64" not in ops          # adds and compares only: nothing to contract
    _audit(s)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fast-math" not in mk and "-Ofast" not in mk
    assert "hmm_viterbi_ragged.o" in mk and "viterbi_ragged.s" in mk and "hmm_viterbi_kernel.hpp" in mk


def _template_bools(name):
    """the trailing bool template arguments of an Itanium-mangled kernel name: ...ILi8ELb0ELb1EE... -> (0, 1)"""
    return tuple(int(x) for x in re.findall(r"Lb([01])E", name))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_row_estep_kernels_need_no_more_scratch_than_the_uniform_ones(isa):
    s = isa("hmm_estep")
    _audit(s)
    priv = _kernel_meta(s.read_text(), ".private_segment_fixed_size")
    rows = {n: v for n, v in priv.items() if "hmm_estep_kernel" in n}
    by_k = {}
    for n, v in rows.items():
        K = int(re.search(r"ILi(\d+)E", n).group(1))
        by_k.setdefault(K, {})[_template_bools(n)] = v
    assert sorted(by_k) == list(range(1, 17))
    for K, d in by_k.items():
        assert (0, 0) in d and (0, 1) in d, (K, d)                     # <K, FUSED = false, RAG = false / true>
        assert d[(0, 1)] <= d[(0, 0)], (K, d)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_wide_estep_kernels_need_no_more_scratch_than_the_uniform_ones(isa):
    s = isa("hmm_estep_wide")
    _audit(s)
    priv = _kernel_meta(s.read_text(), ".private_segment_fixed_size")
    wide = {n: v for n, v in priv.items() if "hmm_estep_wide_kernel" in n}
    assert len(wide) == 8, sorted(wide)
    by = {}
    for n, v in wide.items():
        KP = int(re.search(r"ILi(\d+)E", n).group(1))
        logspace, rag = _template_bools(n)
        by[(KP, logspace, rag)] = v
    for KP in (32, 64):
        for logspace in (0, 1):
            assert by[(KP, logspace, 1)] <= by[(KP, logspace, 0)], by
