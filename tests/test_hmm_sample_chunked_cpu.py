"""CPU tests of time-chunked HMM posterior sampling (svae_hmm_chunked_sample_f64, svae_amd.hmm.hmm_sample_chunked): the
NumPy restatement of its stages (tests/_hmm_sample_chunked_numpy.py) against the log-space oracle and its draw margins on
the cases the GPU tests use; the long cases' margins against the long-double truth; the ABI's symbols, workspace closed
form, default chunk and error codes; the Python entry's signature and refusals; the new unit's ISA metadata."""
import ctypes
import inspect
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
import _hmm_sample_chunked_numpy as SC  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402
import _hmm_sample_range_numpy as SR  # noqa: E402

NAMES = ("svae_hmm_chunked_sample_default_chunk", "svae_hmm_chunked_sample_workspace_bytes", "svae_hmm_chunked_sample_f64")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


@pytest.mark.parametrize("B,T,K,S,chunk,pb", SC.CASES)
def test_restatement_equals_the_oracle_with_every_draw_counted(B, T, K, S, chunk, pb):
    init, pair, node, u, want, want_logZ, margin = SC.case(B, T, K, S, chunk, pb)
    print("margin %.3e" % margin)
    assert margin >= smp.MARGIN                                   # no draw is left out of any comparison
    states, logZ, flagged = SC.chunked_sample_batch(init, pair, node, u, chunk)
    assert not flagged.any()
    assert np.array_equal(states, want)
    assert np.allclose(logZ, want_logZ, rtol=1e-12, atol=1e-10)


def test_restatement_flags_the_hostile_sequences_of_the_range_batch():
    b = SR.gap_batch(8, 37)
    _, _, flagged = SC.chunked_sample_batch(b["init"], b["pair"], b["node"], b["u"], 8)
    assert b["extreme"].any() and not b["extreme"].all()
    assert flagged[b["extreme"]].all()


@pytest.mark.parametrize("K", [3, 8])
def test_long_truth_agrees_with_the_oracle_on_small_cases(K):
    for B, T, K_, S, chunk, pb in [c for c in SC.CASES if c[2] == K and not c[5]][:1] + [(1, 141, 3, 3, 2, 0)]:
        init, pair, node, u, want, want_logZ, _ = SC.case(B, T, K_, S, chunk, pb)
        for b in range(B):
            states, logZ, margin = SC.long_truth(init, pair, node[b], u[b])
            assert np.array_equal(states, want[b]) and abs(logZ - want_logZ[b]) <= 1e-10 * max(1.0, abs(logZ))
            assert margin >= smp.MARGIN


@pytest.mark.parametrize("B,T,K,S", SC.LONG_CASES)
def test_long_cases_have_their_margins(B, T, K, S):
    margin = SC.long_case(B, T, K, S)[6]
    print("margin %.3e" % margin)
    assert margin >= smp.MARGIN


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
    assert H.hmm_sample_chunked is hmm_inference.hmm_sample_chunked
    assert list(inspect.signature(H.hmm_sample_chunked).parameters) == [
        "natparam", "num_samples", "u", "generator", "chunk", "workspace", "return_logZ"]
    sig = inspect.signature(H.hmm_sample_chunked).parameters
    assert sig["num_samples"].default == 1 and sig["return_logZ"].default is False
    assert all(sig[k].default is None for k in ("u", "generator", "chunk", "workspace"))
    assert "hmm_sample_chunked" in hmm_inference.sample_redone_sequences.__doc__
    assert "sample_redone_sequences" in H.hmm_sample_chunked.__doc__


def test_workspace_closed_form_and_default_chunk():
    _, lib = _lib()
    ws, dc = lib.svae_hmm_chunked_sample_workspace_bytes, lib.svae_hmm_chunked_sample_default_chunk
    shapes = [c[:5] for c in SC.CASES] + [(8, 50000, 16, 8, 184), (512, 500, 8, 1, 32), (3, 10, 4, 2, 10), (3, 10, 4, 2, 999),
                                          (1, 22785, 16, 2, 256), (32, 50000, 16, 1, 32), (3, 7, 5, 3, 2)]
    for B, T, K, S, chunk in shapes:
        got = ws(B, T, K, S, chunk)
        lay = SC.layout(B, T, K, S, chunk)
        assert got == SC.workspace_bytes(B, T, K, S, chunk) == lay["total"] and got % 16 == 0, (B, T, K, S, chunk)
        assert all(v % 16 == 0 for v in lay.values() if v is not lay["C"])
        assert lay["rec"] == 0 and lay["cand"] - lay["maps"] == 16 * B * S * T         # the candidates: a buffer of their own
        assert got >= lib.svae_hmm_sample_workspace_bytes(B, T, K) > 0                 # the one-chunk route fits
    assert ws(3, 10, 4, 2, 10) == ws(3, 10, 4, 2, 11)                                  # one chunk holds the sequence
    for bad in [(0, 7, 3, 1, 2), (-1, 7, 3, 1, 2), (1, 0, 3, 1, 2), (1, 7, 0, 1, 2), (1, 7, 17, 1, 2), (1, 7, 64, 1, 2),
                (1, 7, 3, 0, 2), (1, 7, 3, -1, 2), (1, 7, 3, 1, 1), (1, 7, 3, 1, 0), (1, 7, 3, 1, -5)]:
        assert ws(*bad) == 0 and SC.workspace_bytes(*bad) == 0, bad
    for B in (1, 8, 32, 127, 128, 129, 512):
        for T in (1, 2, 3, 499, 500, 5000, 50000, 10 ** 6):
            for K in (1, 8, 16):
                for S in (1, 8):
                    got = dc(B, T, K, S)
                    assert got == SC.default_chunk(B, T, K, S) and (got == T or 2 <= got < T), (B, T, K, S, got)
    # refused arguments: the serial T
    assert dc(1, 5000, 17, 1) == 5000 and dc(0, 5000, 8, 1) == 5000 and dc(1, 5000, 0, 1) == 5000
    assert dc(-1, 5000, 8, 1) == 5000 and dc(1, 5000, 8, 0) == 5000 and dc(64, 10 ** 6, 8, 64) == 10 ** 6
    assert dc(512, 500, 8, 1) == 500 and dc(129, 5000, 16, 1) == 5000
    assert (dc(1, 500, 8, 1), dc(8, 5000, 16, 8), dc(32, 50000, 8, 1)) == (32, 64, 256)      # the chunked E-step's rule


def test_chunked_sample_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU): the pointers are host addresses that
    must never be dereferenced"""
    _, lib = _lib()
    raw = (ctypes.c_double * 1024)()
    base = ctypes.addressof(raw)
    base += -base % 16
    p = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 8)
    need = lib.svae_hmm_chunked_sample_workspace_bytes(2, 9, 5, 3, 3)
    assert need > 0

    def call(B=2, T=9, K=5, S=3, pb=0, chunk=3, init=p, pair=p, node=p, u=p, states=p, logZ=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_chunked_sample_f64(B, T, K, S, pb, chunk, init, pair, node, u, states, logZ, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3 and call(K=17) == -3 and call(K=64) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(chunk=1) == -7 and call(chunk=0) == -7 and call(chunk=-4) == -7
    assert call(node=None) == -8
    assert call(S=0) == -9 and call(S=-2) == -9
    assert call(B=2 ** 15, T=2 ** 15, S=2) == -10
    assert call(u=None) == -11
    assert call(states=None) == -12 and call(states=None, logZ=None) == -12
    assert call(ws=None) == -13
    assert call(ws_bytes=need - 1) == -14 and call(ws_bytes=0) == -14
    assert call(chunk=9, ws_bytes=lib.svae_hmm_chunked_sample_workspace_bytes(2, 9, 5, 3, 9) - 1) == -14
    assert call(ws=odd) == -15 and call(ws=odd, chunk=9) == -15 and call(ws=odd, logZ=None) == -15
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=17, init=None) == -3
    assert call(pb=2, init=None) == -4 and call(init=None, pair=None, chunk=1) == -5 and call(pair=None, chunk=1) == -6
    assert call(chunk=1, node=None, S=0) == -7 and call(node=None, S=0, u=None) == -8 and call(S=0, u=None) == -9
    assert call(u=None, states=None) == -11 and call(states=None, ws=None, ws_bytes=0) == -12
    assert call(ws=None, ws_bytes=0) == -13 and call(ws=odd, ws_bytes=0) == -14
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(chunk=1), call(node=None),
             call(S=0), call(B=2 ** 15, T=2 ** 15, S=2), call(u=None), call(states=None), call(ws=None), call(ws_bytes=0),
             call(ws=odd)}
    assert len(codes) == 15 and all(-100 < c < 0 for c in codes)          # one distinct code per bad argument
    # B = 0 returns 0 right behind the shared checks and K > 16
    n = None
    e = lib.svae_hmm_chunked_sample_f64
    assert e(0, 9, 5, 0, 0, 1, p, p, n, n, n, n, n, 0, None) == 0
    assert e(0, 9, 17, 1, 0, 3, p, p, n, n, n, n, n, 0, None) == -3
    assert e(0, 0, 5, 1, 0, 3, p, p, n, n, n, n, n, 0, None) == -2
    assert e(0, 9, 5, 1, 0, 3, p, n, n, n, n, n, n, 0, None) == -6


def test_python_refusals_come_before_any_device():
    from svae_amd.hmm import hmm_sample_chunked as f
    z = np.zeros
    with pytest.raises(ValueError, match="hmm_sample"):
        f((z(17), z((17, 17)), z((40, 17))), chunk=4)
    with pytest.raises(ValueError, match="use hmm_sample$"):
        f((z(64), z((64, 64)), z((2, 40, 64))))
    for chunk in (1, 0, 2.5, 2.0, "4", True):
        with pytest.raises(ValueError, match="chunk must be an integer >= 2"):
            f((z(3), z((3, 3)), z((40, 3))), chunk=chunk)
    with pytest.raises(ValueError, match="u must have shape"):
        f((z(3), z((3, 3)), z((2, 40, 3))), num_samples=2, u=z((2, 40)), chunk=4)
    with pytest.raises(ValueError, match="u must have shape"):
        f((z(3), z((3, 3)), z((40, 3))), num_samples=2, u=z((1, 2, 40)), chunk=4)
    with pytest.raises(ValueError, match="num_samples must be an integer >= 1"):
        f((z(3), z((3, 3)), z((40, 3))), num_samples=0, chunk=4)
    with pytest.raises(ValueError, match="init/pair parameter shapes do not match the node potentials"):
        f((z(4), z((3, 3)), z((40, 3))), chunk=4)
    with pytest.raises(TypeError):
        f((z(3), z((3, 3)), z((40, 3))), chunk=4, lengths=[40])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_chunked_sample_unit_has_no_scratch_no_spills_and_passes_the_hazard_audit(tmp_path):
    out = tmp_path / "hmm_sample_chunked.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hmm_sample_chunked.hip"), "-o", str(out)], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = sorted(set(re.findall(r"\.name:\s+(_ZN4svae\w+)", text)))
    want = sorted(["_ZN4svae22hmm_smpc_filter_kernelILi%dEEEvNS_17SampleChunkedArgsE" % k for k in range(1, 17)]
                  + ["_ZN4svae20hmm_smpc_maps_kernelILi%dEEEvNS_17SampleChunkedArgsE" % k for k in range(1, 17)]
                  + ["_ZN4svae20hmm_smpc_mark_kernelENS_17SampleChunkedArgsE", "_ZN4svae21hmm_smpc_chase_kernelENS_17SampleChunkedArgsE"])
    assert names == want, names
    sizes = [l.split()[-1] for l in text.splitlines() if ".private_segment_fixed_size:" in l]
    spills = [l.split()[-1] for l in text.splitlines() if ".vgpr_spill_count:" in l]
    sspills = [l.split()[-1] for l in text.splitlines() if ".sgpr_spill_count:" in l]
    assert len(sizes) == 34 and set(sizes) == {"0"}, sizes
    assert len(spills) == 34 and set(spills) == {"0"}, spills
    assert len(sspills) == 34 and set(sspills) == {"0"}, sspills
    a = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(out)],
                       capture_output=True, text=True)
    assert a.returncode == 0, a.stdout + a.stderr
