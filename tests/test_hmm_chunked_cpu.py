"""CPU tests of the time-chunked HMM E-step (svae_hmm_chunked_estep_f64, csrc/hmm_estep_chunked.hip): the NumPy
restatement of its three stages and range criterion (tests/_hmm_chunked_numpy.py) against the log-space oracle at
tests/test_hmm_hip.py's tolerances; the symbols, the unchanged ABI number, the workspace closed form, every host-side
argument check in order, the Python refusals, and the unit's ISA metadata."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_chunked_numpy as C  # noqa: E402
from oracle import hmm_numpy  # noqa: E402

NAMES = ("svae_hmm_chunked_default_chunk", "svae_hmm_chunked_workspace_bytes", "svae_hmm_chunked_estep_f64")
# beyond the GPU test's shapes: the smallest and a few hundred chunks
EXTRA_SHAPES = [(1, 3, 2, 2), (2, 2000, 8, 16), (1, 1024, 16, 128), (1, 50, 3, 49)]


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def _against_oracle(init, pair, node, chunk):
    flagged = []
    for b in range(node.shape[0]):
        pb = pair[b] if pair.ndim == 3 else pair
        lz, (oi, ot, os_) = hmm_numpy.hmm_estep((init, pb, node[b]))
        logZ, (Ei, Et, Es), bad = C.chunked_estep((init, pb, node[b]), chunk)
        assert logZ == pytest.approx(lz, rel=1e-10, abs=1e-10)
        np.testing.assert_allclose(Ei, oi, rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(Et, ot, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(Es, os_, rtol=1e-8, atol=1e-12)
        assert np.abs(Es.sum(-1) - 1).max() < 1e-12
        assert abs(Et.sum() - (node.shape[1] - 1)) < 1e-10 * node.shape[1]
        lz_only, none, bad_lz = C.chunked_estep((init, pb, node[b]), chunk, want_stats=False)
        assert lz_only == logZ and none is None and not bad_lz
        flagged.append(bad)
    return np.array(flagged)


@pytest.mark.parametrize("pair_batched", [False, True])
@pytest.mark.parametrize("B,T,K,chunk", C.PARITY_SHAPES + EXTRA_SHAPES)
def test_restatement_matches_the_oracle_and_flags_nothing(B, T, K, chunk, pair_batched):
    init, pair, node = C.parity_problem(B, T, K, chunk, pair_batched)
    assert not _against_oracle(init, pair, node, chunk).any()


def test_restatement_flags_the_hostile_sequences_of_the_range_batch_only():
    init, pair, node, hostile = C.range_batch()
    flagged = np.array([C.chunked_estep((init, pair[b], node[b]), 8)[2] for b in range(node.shape[0])])
    assert (flagged == hostile).all(), (flagged, hostile)
    for b in np.flatnonzero(~hostile):
        assert not _against_oracle(init, pair[b], node[b:b + 1], 8).any()
    for b in np.flatnonzero(hostile):                       # every one has a path of finite score
        assert np.isfinite(hmm_numpy.hmm_estep((init, pair[b], node[b]))[0])


def test_symbols_declared_bound_and_exported_with_abi_15():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert re.search(r"#define\s+SVAE_HIP_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and lib.svae_hip_abi_version() == 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.SIGNATURES and hasattr(lib, s), s
    import svae_amd.hmm as H
    from svae_amd.hmm import hmm_inference
    for s in ("hmm_estep_chunked", "hmm_logZ_chunked", "chunked_redone_sequences"):
        assert getattr(H, s) is getattr(hmm_inference, s)
    import inspect
    assert "lengths" not in inspect.signature(H.hmm_estep_chunked).parameters
    assert list(inspect.signature(H.hmm_estep_chunked).parameters) == ["natparam", "chunk", "workspace"]
    assert list(inspect.signature(H.hmm_logZ_chunked).parameters) == ["natparam", "chunk"]


def test_workspace_closed_form_and_default_chunk():
    _, lib = _lib()
    ws, dc = lib.svae_hmm_chunked_workspace_bytes, lib.svae_hmm_chunked_default_chunk
    for B, T, K, chunk in C.PARITY_SHAPES + EXTRA_SHAPES + [(8, 50000, 16, 184), (512, 500, 8, 32), (3, 10, 4, 10),
                                                            (3, 10, 4, 999)]:
        assert ws(B, T, K, chunk) == 8 * C.workspace_doubles(B, T, K, chunk), (B, T, K, chunk)
    assert ws(3, 10, 4, 10) == ws(3, 10, 4, 11)                           # one chunk holds the sequence
    assert ws(1, 7, 3, 2) >= lib.svae_hmm_workspace_bytes(1, 7, 3)        # the serial route's records are inside
    for bad in [(0, 7, 3, 2), (-1, 7, 3, 2), (1, 0, 3, 2), (1, 7, 0, 2), (1, 7, 17, 2), (1, 7, 64, 2), (1, 7, 3, 1),
                (1, 7, 3, 0), (1, 7, 3, -5)]:
        assert ws(*bad) == 0, bad
    for B in (1, 8, 128, 129, 512):
        for T in (1, 2, 499, 500, 5000, 50000, 10 ** 6):
            for K in (1, 8, 16):
                got = dc(B, T, K)
                assert got == C.default_chunk(B, T, K) and (got == T or 2 <= got < T), (B, T, K, got)
    assert dc(1, 5000, 17) == 5000 and dc(0, 5000, 8) == 5000 and dc(1, 5000, 0) == 5000      # refused: the serial T
    assert dc(512, 500, 8) == 500                                         # a batch that fills the chip stays serial
    assert (dc(1, 500, 8), dc(8, 5000, 16), dc(1, 50000, 8)) == (32, 64, 256)  # the measured minima


def test_chunked_estep_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU): the pointers are host addresses that
    must never be dereferenced"""
    _, lib = _lib()
    raw = (ctypes.c_double * 1024)()
    p = ctypes.c_void_p(ctypes.addressof(raw))
    need = lib.svae_hmm_chunked_workspace_bytes(2, 9, 5, 3)
    assert need > 0

    def call(B=2, T=9, K=5, pb=0, chunk=3, init=p, pair=p, node=p, logZ=p, Ei=p, Et=p, Es=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_chunked_estep_f64(B, T, K, pb, chunk, init, pair, node, logZ, Ei, Et, Es, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3 and call(K=17) == -3 and call(K=64) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(chunk=1) == -7 and call(chunk=0) == -7 and call(chunk=-4) == -7
    assert call(node=None) == -8
    assert call(logZ=None) == -9
    for mix in [dict(Ei=None), dict(Et=None), dict(Es=None), dict(Ei=None, Et=None), dict(Ei=None, Es=None),
                dict(Et=None, Es=None)]:
        assert call(**mix) == -10, mix
    assert call(ws=None) == -11 and call(ws=None, Ei=None, Et=None, Es=None) == -11
    assert call(ws_bytes=need - 1) == -12 and call(ws_bytes=0) == -12
    assert call(chunk=9, ws_bytes=lib.svae_hmm_chunked_workspace_bytes(2, 9, 5, 9) - 1) == -12     # one chunk: its own size
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=17, init=None) == -3
    assert call(init=None, pair=None, chunk=1) == -5 and call(chunk=1, node=None, logZ=None) == -7
    assert call(node=None, logZ=None, Ei=None) == -8 and call(logZ=None, Ei=None, ws=None) == -9
    assert call(Ei=None, ws=None, ws_bytes=0) == -10 and call(ws=None, ws_bytes=0) == -11
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(chunk=1),
             call(node=None), call(logZ=None), call(Ei=None), call(ws=None), call(ws_bytes=0)}
    assert len(codes) == 12 and all(-100 < c < 0 for c in codes)          # one distinct code per bad argument
    # B = 0 returns 0 right behind the shared checks and K > 16
    n = None
    e = lib.svae_hmm_chunked_estep_f64
    assert e(0, 9, 5, 0, 1, p, p, n, n, n, n, n, n, 0, None) == 0
    assert e(0, 9, 17, 0, 3, p, p, n, n, n, n, n, n, 0, None) == -3
    assert e(0, 0, 5, 0, 3, p, p, n, n, n, n, n, n, 0, None) == -2
    assert e(0, 9, 5, 0, 3, p, n, n, n, n, n, n, n, 0, None) == -6


def test_python_refusals_come_before_any_device():
    from svae_amd.hmm import hmm_estep_chunked, hmm_logZ_chunked, chunked_redone_sequences
    z = np.zeros
    for f in (hmm_estep_chunked, hmm_logZ_chunked):
        with pytest.raises(ValueError, match="hmm_estep"):
            f((z(17), z((17, 17)), z((40, 17))), chunk=4)
        with pytest.raises(ValueError, match="hmm_estep"):
            f((z(64), z((64, 64)), z((2, 40, 64))))
        for chunk in (1, 0, -3, 2.0, 2.5, "4", True):
            with pytest.raises(ValueError, match="chunk must be an integer >= 2"):
                f((z(3), z((3, 3)), z((40, 3))), chunk=chunk)
        with pytest.raises(ValueError, match="init/pair parameter shapes do not match the node potentials"):
            f((z(4), z((3, 3)), z((40, 3))), chunk=4)
        with pytest.raises(ValueError, match="init/pair parameter shapes do not match the node potentials"):
            f((z(3), z((5, 3, 3)), z((2, 40, 3))), chunk=4)
        with pytest.raises(ValueError, match=r"node_params must be \(T,K\) or \(B,T,K\)"):
            f((z(3), z((3, 3)), z(3)), chunk=4)
        with pytest.raises(ValueError, match="outside 1..64"):
            f((z(65), z((65, 65)), z((40, 65))), chunk=4)
        with pytest.raises(TypeError):
            f((z(3), z((3, 3)), z((40, 3))), chunk=4, lengths=[40])
    import torch
    ws = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError):
        chunked_redone_sequences(ws, 2, 40, 17, 4)
    with pytest.raises(ValueError, match="chunk must be an integer >= 2"):
        chunked_redone_sequences(ws, 2, 40, 3, 1)
    with pytest.raises(ValueError, match="smaller"):
        chunked_redone_sequences(ws, 2, 40, 3, 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_chunked_unit_has_no_scratch_no_spills_and_passes_the_hazard_audit(tmp_path):
    out = tmp_path / "hmm_estep_chunked.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hmm_estep_chunked.hip"), "-o", str(out)], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = [l.split()[-1] for l in text.splitlines() if l.strip().startswith(".name:") and "hmm_chunk" in l]
    for kern in ("hmm_chunk_ops_kernel", "hmm_chunk_scan_kernel", "hmm_chunk_estep_kernel"):
        assert sum(kern in n for n in names) == 16, (kern, names)         # K = 1 .. 16
    assert sum("hmm_chunk_combine_kernel" in n for n in names) == 1 and sum("hmm_chunk_index_kernel" in n for n in names) == 1
    sizes = [l.split()[-1] for l in text.splitlines() if ".private_segment_fixed_size:" in l]
    spills = [l.split()[-1] for l in text.splitlines() if ".vgpr_spill_count:" in l]
    assert len(sizes) == 50 and set(sizes) == {"0"}, sizes
    assert len(spills) == 50 and set(spills) == {"0"}, spills
    a = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(out)],
                       capture_output=True, text=True)
    assert a.returncode == 0, a.stdout + a.stderr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hmm_estep_chunked.o" in mk and "estep_chunked.s" in mk
