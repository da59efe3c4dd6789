"""CPU tests of the time-chunked Viterbi decoder (svae_hmm_chunked_viterbi_f64, csrc/hmm_viterbi_chunked.hip): the NumPy
restatement of its five stages (tests/_hmm_viterbi_chunked_numpy.py) against the serial restatement
(tests/_hmm_viterbi_numpy.py) and against brute force; the symbols, the unchanged ABI number, the workspace closed form,
the default chunk, every host-side argument check in order, the Python refusals, and the unit's ISA metadata."""
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
import _hmm_chunked_numpy as C  # noqa: E402
import _hmm_viterbi_chunked_numpy as VC  # noqa: E402
import _hmm_viterbi_numpy as V  # noqa: E402

NAMES = ("svae_hmm_chunked_viterbi_default_chunk", "svae_hmm_chunked_viterbi_workspace_bytes",
         "svae_hmm_chunked_viterbi_f64")
# beyond the GPU test's shapes: the smallest and a few hundred chunks
EXTRA_SHAPES = [(1, 3, 2, 2), (2, 2000, 8, 16), (1, 1024, 16, 128), (1, 50, 3, 49)]


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


@pytest.mark.parametrize("pair_batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("B,T,K,chunk", C.PARITY_SHAPES + EXTRA_SHAPES)
def test_restatement_matches_the_serial_restatement(B, T, K, chunk, pair_batched):
    init, pair, node = C.parity_problem(B, T, K, chunk, pair_batched)
    labels, score = VC.chunked_viterbi_batch(init, pair, node, chunk)
    want, want_score = V.viterbi_batch(init, pair, node)
    assert labels.dtype == np.int32 and labels.shape == (B, T)
    assert np.array_equal(labels, want)
    for b in range(B):
        pb = pair[b] if pair_batched else pair
        bound = VC.score_bound(init, pb, node[b])
        assert abs(score[b] - want_score[b]) <= bound, (b, score[b] - want_score[b], bound)
        assert abs(V.path_score(init, pb, node[b], labels[b]) - want_score[b]) <= bound


@pytest.mark.parametrize("T,K,chunk", [(7, 2, 2), (7, 2, 3), (5, 3, 2), (6, 3, 4), (4, 4, 3), (9, 2, 8)])
def test_restatement_finds_the_optimum_of_all_paths(T, K, chunk):
    rng = np.random.default_rng(T * 100 + K * 10 + chunk)
    for _ in range(3):
        init, pair, node = C.problem(1, T, K, rng, C.PARITY_SCALE)
        labels, score = VC.chunked_viterbi(init, pair, node[0], chunk)
        best, _ = V.brute_force(init, pair, node[0])
        bound = VC.score_bound(init, pair, node[0])
        assert abs(score - best) <= bound
        assert abs(V.path_score(init, pair, node[0], labels) - best) <= bound


def test_dyadic_problems_equal_the_serial_restatement_bit_for_bit():
    ties, neg_inf, inf_pair, dead = 0, 0, 0, 0
    for seed in VC.DYADIC_SEEDS:
        init, pair, node, chunk = VC.dyadic_problem(seed)
        B, T, K = node.shape
        assert 1 <= K <= 16 and 3 <= T <= 70 and 2 <= chunk < T
        for x in (init, pair, node):
            fin = x[np.isfinite(x)]
            assert (fin * 4 == np.round(fin * 4)).all() and fin.min(initial=0) >= -0.75 and fin.max(initial=-1) <= 0
            assert not np.isnan(x).any() and not (x == np.inf).any()
        labels, score = VC.chunked_viterbi_batch(init, pair, node, chunk)
        want, want_score = V.viterbi_batch(init, pair, node)
        assert np.array_equal(labels, want), seed
        assert np.array_equal(VC.bits(score), VC.bits(want_score)), seed
        ties += sum(VC.count_ties(init, pair[b] if pair.ndim == 3 else pair, node[b]) for b in range(B))
        neg_inf += int(np.isinf(pair).any() or np.isinf(node).any())
        inf_pair += int(np.isinf(pair).any() and np.isinf(node).any())
        dead += int((want_score == -np.inf).any())
    # on average at least one tied maximum per problem, a third with -inf entries (in both the transitions and the node
    # potentials wherever K > 1 leaves room for one), a chain with no finite path
    assert ties >= len(VC.DYADIC_SEEDS) and neg_inf >= len(VC.DYADIC_SEEDS) // 3 and dead >= 1, (ties, neg_inf, dead)
    assert inf_pair >= neg_inf // 2, (inf_pair, neg_inf)


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
    assert H.hmm_viterbi_chunked is hmm_inference.hmm_viterbi_chunked
    assert list(inspect.signature(H.hmm_viterbi_chunked).parameters) == ["natparam", "chunk", "workspace", "return_score"]


def test_workspace_closed_form_and_default_chunk():
    _, lib = _lib()
    ws, dc = lib.svae_hmm_chunked_viterbi_workspace_bytes, lib.svae_hmm_chunked_viterbi_default_chunk
    for B, T, K, chunk in C.PARITY_SHAPES + EXTRA_SHAPES + [(8, 50000, 16, 184), (512, 500, 8, 32), (3, 10, 4, 10),
                                                            (3, 10, 4, 999), (1, 4097, 4, 64), (32, 50000, 16, 32)]:
        got = ws(B, T, K, chunk)
        assert got == VC.workspace_bytes(B, T, K, chunk) and got % 16 == 0, (B, T, K, chunk)
        assert got >= lib.svae_hmm_viterbi_workspace_bytes(B, T, K) > 0     # the one-chunk route fits
    assert ws(3, 10, 4, 10) == ws(3, 10, 4, 11)                             # one chunk holds the sequence
    for bad in [(0, 7, 3, 2), (-1, 7, 3, 2), (1, 0, 3, 2), (1, 7, 0, 2), (1, 7, 17, 2), (1, 7, 64, 2), (1, 7, 3, 1),
                (1, 7, 3, 0), (1, 7, 3, -5)]:
        assert ws(*bad) == 0 and VC.workspace_bytes(*bad) == 0, bad
    for B in (1, 8, 32, 127, 128, 129, 256, 257, 512):
        for T in (1, 2, 3, 499, 500, 5000, 50000, 10 ** 6):
            for K in (1, 8, 16):
                got = dc(B, T, K)
                assert got == VC.default_chunk(B, T, K) and (got == T or 2 <= got < T), (B, T, K, got)
    assert dc(1, 5000, 17) == 5000 and dc(0, 5000, 8) == 5000 and dc(1, 5000, 0) == 5000      # refused: the serial T
    assert dc(-1, 5000, 8) == 5000 and dc(1, 5000, 64) == 5000
    assert dc(512, 500, 8) == 500 and dc(257, 5000, 16) == 5000           # a batch that fills the chip stays serial
    assert (dc(1, 500, 8), dc(8, 5000, 16), dc(32, 50000, 8)) == (32, 64, 256)                 # the measured minima ...
    assert (dc(128, 500, 16), dc(256, 500, 8), dc(128, 5000, 8), dc(256, 5000, 16)) == (64, 64, 128, 128)   # ... and from 128 sequences up


def test_chunked_viterbi_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU): the pointers are host addresses that
    must never be dereferenced"""
    _, lib = _lib()
    raw = (ctypes.c_double * 1024)()
    base = ctypes.addressof(raw)
    base += -base % 16
    p = ctypes.c_void_p(base)
    odd = ctypes.c_void_p(base + 8)
    need = lib.svae_hmm_chunked_viterbi_workspace_bytes(2, 9, 5, 3)
    assert need > 0

    def call(B=2, T=9, K=5, pb=0, chunk=3, init=p, pair=p, node=p, states=p, score=p, ws=p, ws_bytes=need):
        return lib.svae_hmm_chunked_viterbi_f64(B, T, K, pb, chunk, init, pair, node, states, score, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2 and call(T=-3) == -2
    assert call(K=0) == -3 and call(K=65) == -3 and call(K=17) == -3 and call(K=64) == -3
    assert call(pb=2) == -4 and call(pb=-1) == -4
    assert call(init=None) == -5
    assert call(pair=None) == -6
    assert call(chunk=1) == -7 and call(chunk=0) == -7 and call(chunk=-4) == -7
    assert call(node=None) == -8
    assert call(states=None) == -9 and call(states=None, score=None) == -9
    assert call(ws=None) == -10
    assert call(ws_bytes=need - 1) == -11 and call(ws_bytes=0) == -11
    assert call(chunk=9, ws_bytes=lib.svae_hmm_chunked_viterbi_workspace_bytes(2, 9, 5, 9) - 1) == -11    # one chunk: its own size
    assert call(ws=odd) == -12 and call(ws=odd, chunk=9) == -12 and call(ws=odd, score=None) == -12
    # the first failing check decides
    assert call(B=-1, T=0, K=0) == -1 and call(T=0, K=0, init=None) == -2 and call(K=17, init=None) == -3
    assert call(pb=2, init=None) == -4 and call(init=None, pair=None, chunk=1) == -5 and call(pair=None, chunk=1) == -6
    assert call(chunk=1, node=None, states=None) == -7 and call(node=None, states=None, ws=None) == -8
    assert call(states=None, ws=None, ws_bytes=0) == -9 and call(ws=None, ws_bytes=0) == -10
    assert call(ws=odd, ws_bytes=0) == -11
    codes = {call(B=-1), call(T=0), call(K=0), call(pb=2), call(init=None), call(pair=None), call(chunk=1),
             call(node=None), call(states=None), call(ws=None), call(ws_bytes=0), call(ws=odd)}
    assert len(codes) == 12 and all(-100 < c < 0 for c in codes)          # one distinct code per bad argument
    # B = 0 returns 0 right behind the shared checks and K > 16
    n = None
    e = lib.svae_hmm_chunked_viterbi_f64
    assert e(0, 9, 5, 0, 1, p, p, n, n, n, n, 0, None) == 0
    assert e(0, 9, 17, 0, 3, p, p, n, n, n, n, 0, None) == -3
    assert e(0, 0, 5, 0, 3, p, p, n, n, n, n, 0, None) == -2
    assert e(0, 9, 5, 0, 3, p, n, n, n, n, n, 0, None) == -6


def test_python_refusals_come_before_any_device():
    from svae_amd.hmm import hmm_viterbi_chunked as f
    z = np.zeros
    with pytest.raises(ValueError, match="hmm_viterbi"):
        f((z(17), z((17, 17)), z((40, 17))), chunk=4)
    with pytest.raises(ValueError, match="use hmm_viterbi$"):
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


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_chunked_viterbi_unit_has_no_scratch_no_spills_and_passes_the_hazard_audit(tmp_path):
    out = tmp_path / "hmm_viterbi_chunked.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "hmm_viterbi_chunked.hip"), "-o", str(out)], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = [l.split()[-1] for l in text.splitlines() if l.strip().startswith(".name:") and "hmm_v" in l]
    assert all("hmm_vchunk" in n for n in names), names               # no kernel of the serial decoder's is built here
    for kern in ("hmm_vchunk_ops_kernel", "hmm_vchunk_scan_kernel", "hmm_vchunk_decode_kernel"):
        assert sum(kern in n for n in names) == 16, (kern, names)     # K = 1 .. 16
    assert sum("hmm_vchunk_resolve_kernel" in n for n in names) == 1 and sum("hmm_vchunk_gather_kernel" in n for n in names) == 1
    sizes = [l.split()[-1] for l in text.splitlines() if ".private_segment_fixed_size:" in l]
    spills = [l.split()[-1] for l in text.splitlines() if ".vgpr_spill_count:" in l]
    assert len(sizes) == 50 and set(sizes) == {"0"}, sizes
    assert len(spills) == 50 and set(spills) == {"0"}, spills
    a = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(out)],
                       capture_output=True, text=True)
    assert a.returncode == 0, a.stdout + a.stderr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hmm_viterbi_chunked.o" in mk and "viterbi_chunked.s" in mk
