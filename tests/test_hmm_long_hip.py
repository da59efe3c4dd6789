"""GPU tests of the HMM routes on LONG sequences -- the regime the time-chunked E-step and decoder exist for -- against the
long-double truth of oracle/hmm_longdouble.py (the fp64 oracle is 3e-9 off at T = 22 785 and cannot referee it;
tests/test_hmm_long_cpu.py).  Shapes, problems and both bounds: tests/_hmm_long_numpy.py.  The chunked E-step on every
LONG_SHAPES case with no sequence redone; the library's own chunk pick; the serial kernels at length; the fallback's index
compaction beyond one ballot block of 64 sequences; a redone sequence of 22 785 steps; the chunked decoder at its own pick.
Every test prints its worst measured ratio to the bound.  Harness: tests/test_hmm_chunked_hip.py's (a workspace of exactly
the closed form, eight canary doubles behind it, the route words read back)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_chunked_numpy as C  # noqa: E402
import _hmm_long_numpy as L  # noqa: E402
import _hmm_viterbi_chunked_numpy as VC  # noqa: E402

CANARY = -12345.678
ALL_KEYS = [key for shape in L.LONG_SHAPES for key in L.parity_keys(shape)]


def _np(x):
    return x.detach().cpu().numpy()


def _flat(out):
    logZ, (Ei, Et, Es) = out
    return tuple(_np(x) for x in (logZ, Ei, Et, Es))


def _chunked(init, pair, node, chunk):
    """hmm_estep_chunked on a workspace of exactly the closed form (eight canary doubles behind it) -> numpy outputs,
    the route words"""
    from svae_amd import _lib
    from svae_amd.hmm import hmm_estep_chunked, chunked_redone_sequences
    B, T, K = node.shape
    need = int(_lib.load().svae_hmm_chunked_workspace_bytes(B, T, K, chunk))
    assert need == 8 * C.workspace_doubles(B, T, K, chunk)
    ws = torch.full((need // 8 + 8,), CANARY, dtype=torch.float64, device="cuda")
    got = _flat(hmm_estep_chunked((init, pair, node), chunk=chunk, workspace=ws[:need // 8]))
    redone = _np(chunked_redone_sequences(ws[:need // 8], B, T, K, chunk))
    assert (_np(ws[need // 8:]) == CANARY).all()                       # nothing written behind the closed form
    return got, redone


def _serial(init, pair, node, lengths=None):
    """hmm_estep on a workspace of its own -> numpy outputs, redone_sequences"""
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_estep, redone_sequences
    B, T, K = node.shape
    need = int(_lib.load().svae_hmm_workspace_bytes(B, T, K))
    ws = torch.full((need // 8 + 8,), CANARY, dtype=torch.float64, device="cuda")
    got = _flat(hmm_estep((init, pair, node), workspace=ws[:need // 8], lengths=lengths))
    redone = _np(redone_sequences(ws[:need // 8], B, T, K))
    assert (_np(ws[need // 8:]) == CANARY).all()
    return got, redone


def _problem(key):
    """(init, pair, node) of L.problem(key) as writable copies (the shared ones are read-only)"""
    return tuple(np.array(x) for x in L.problem(key)[:3])


def _seq(got, b):
    return tuple(x[b] for x in got)


def _assert_scaled(got, key, rows=None, what=""):
    """every sequence of `got` (rows: its indices in the problem `key`) within the scaled bound of truth; -> worst ratio"""
    assert all(np.isfinite(x).all() for x in got)
    rows = range(got[0].shape[0]) if rows is None else rows
    worst = (0.0, "", -1)
    for i, b in enumerate(rows):
        ratio, name = L.scaled_ratio(_seq(got, i), key, b)
        worst = max(worst, (ratio, name, b))
    print("%s%s: worst |error| = %.3f T eps (%s of sequence %d) = %.3f of the bound %g T eps"
          % (what, key, worst[0], worst[1], worst[2], worst[0] / L.C_SCALED, L.C_SCALED))
    assert worst[0] <= L.C_SCALED, worst
    return worst[0]


def _assert_redo(got, key, rows, what=""):
    """every sequence of `got` within the redo bound (8 x the fp64 oracle's own error against truth on that sequence)"""
    worst = 0.0
    for i, b in enumerate(rows):
        errs, bound = L.redo_errors(_seq(got, i), key, b), L.redo_bound(key, b)
        print("%s%s sequence %d: logZ rel %.2e (bound %.2e)  E_states abs %.2e (%.2e)  E_trans abs %.2e (%.2e)"
              % (what, key, b, errs[0], bound[0], errs[1], bound[1], errs[2], bound[2]))
        assert (errs <= bound).all(), (b, errs, bound)
        worst = max(worst, float((errs / bound).max()))
    print("%s%s: worst error / redo bound = %.3f" % (what, key, worst))
    return worst


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


# ---- 1. the chunked E-step on every LONG_SHAPES case ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_chunked_estep_within_the_scaled_bound_of_truth_without_fallback(key):
    from svae_amd.hmm import hmm_logZ_chunked
    init, pair, node = _problem(key)
    chunk = key[4]
    got, redone = _chunked(init, pair, node, chunk)
    # the cap on redone sequences is ZERO: the restatement flags none of these (test_hmm_long_cpu.py)
    assert not redone.any(), np.flatnonzero(redone)
    _assert_scaled(got, key)
    assert _bits_equal((_np(hmm_logZ_chunked((init, pair, node), chunk=chunk)),), got[:1])


# ---- 2. the library's own pick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K", [(1, 22785, 8), (3, 5700, 5), (128, 500, 8)])
def test_default_pick_is_the_explicit_call_with_the_rules_chunk(B, T, K):
    from svae_amd.hmm import hmm_estep_chunked, hmm_logZ_chunked
    pick = C.default_chunk(B, T, K)
    assert 2 <= pick < T and (B, T, K, pick) in L.LONG_SHAPES
    init, pair, node = _problem(("parity", B, T, K, pick, False))
    want, redone = _chunked(init, pair, node, pick)
    assert not redone.any()
    assert _bits_equal(_flat(hmm_estep_chunked((init, pair, node))), want)
    assert _bits_equal((_np(hmm_logZ_chunked((init, pair, node))),), want[:1])


def test_default_pick_above_128_sequences_is_the_serial_route():
    from svae_amd.hmm import hmm_estep_chunked, hmm_logZ_chunked
    from svae_amd.hmm.hmm_inference import hmm_estep
    assert C.default_chunk(129, 500, 8) == 500
    init, pair, node = C.parity_problem(129, 500, 8, 32, False)
    want = _flat(hmm_estep((init, pair, node)))
    assert _bits_equal(_flat(hmm_estep_chunked((init, pair, node))), want)
    assert _bits_equal((_np(hmm_logZ_chunked((init, pair, node))),), want[:1])


# ---- 3. the serial routes at length --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("parity", 1, 22785, 8, 256, False), ("parity", 1, 22785, 16, 256, False),
                                 ("parity", 1, 4096, 24, 0, False)], ids=["two-ended K=8", "two-ended K=16", "wide K=24"])
def test_serial_estep_at_length_within_the_scaled_bound(key):
    init, pair, node = _problem(key)
    got, redone = _serial(init, pair, node)
    assert not redone.any()
    _assert_scaled(got, key, what="hmm_estep ")


def test_ragged_estep_at_length_against_truth_of_the_cut_sequences():
    lengths = (4401, 4097)
    key = ("ragged", 2, 4401, 8, lengths)
    init, pair, node = _problem(key)
    padded = np.array(node)
    for b, n in enumerate(lengths):
        padded[b, n:] = np.nan
    got, redone = _serial(init, pair, padded, lengths=np.array(lengths))
    assert not redone.any()
    _assert_scaled(got, key, what="hmm_estep(lengths=) ")
    assert (got[3][1, lengths[1]:] == 0.0).all()


# ---- 4. the fallback beyond one ballot block -------------------------------------------------------------------------------------
def test_fallback_compaction_beyond_one_ballot_block():
    init, pair, node, hostile = L.long_range_batch()
    key = ("range",)
    got, redone = _chunked(init, pair, node, L.RANGE_CHUNK)
    assert (redone == hostile).all(), (np.flatnonzero(redone), np.flatnonzero(hostile))
    bad, keep = np.flatnonzero(hostile), np.flatnonzero(~hostile)
    assert all(np.isfinite(x).all() for x in got)
    _assert_redo(tuple(x[bad] for x in got), key, bad, what="redone ")
    _assert_scaled(tuple(x[keep] for x in got), key, rows=keep, what="benign ")
    # the benign sequences alone, a batch of 123: the same bits (the compaction is stable; no neighbour's route leaks)
    alone, redone_alone = _chunked(init, pair[keep], node[keep], L.RANGE_CHUNK)
    assert not redone_alone.any()
    assert _bits_equal(alone, tuple(x[keep] for x in got))


# ---- 5. a redone sequence of 22 785 steps ----------------------------------------------------------------------------------------
def test_redo_at_length_is_the_serial_route_and_within_the_oracles_own_error():
    init, pair, node = L.hostile_long()
    key = ("hostile",)
    chunked, route = _chunked(init, pair, node, L.HOSTILE_CHUNK)
    serial, redone = _serial(init, pair, node)
    assert route.all() and redone.all()
    _assert_redo(chunked, key, [0], what="hmm_estep_chunked ")
    _assert_redo(serial, key, [0], what="hmm_estep ")
    assert _bits_equal(chunked, serial)


# ---- 6. the chunked decoder at its own pick --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,K,chunk", [(1, 22785, 8, None), (1, 22785, 16, None), (1, 4401, 2, 2)])
def test_chunked_viterbi_at_length(B, T, K, chunk):
    from svae_amd import _lib
    from svae_amd.hmm import hmm_viterbi_chunked
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    pick = VC.default_chunk(B, T, K) if chunk is None else chunk
    assert (B, T, K, pick) in L.LONG_SHAPES
    init, pair, node = _problem(("parity", B, T, K, pick, False))
    need = int(_lib.load().svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, pick))
    assert need == VC.workspace_bytes(B, T, K, pick)
    ws = torch.full((need // 8 + 8,), CANARY, dtype=torch.float64, device="cuda")
    labels, score = (_np(x) for x in hmm_viterbi_chunked((init, pair, node), chunk=chunk, workspace=ws[:need // 8],
                                                         return_score=True))
    assert (_np(ws[need // 8:]) == CANARY).all()
    want, want_score = VC.chunked_viterbi_batch(init, pair, node, pick)
    assert np.array_equal(labels, want)
    assert np.array_equal(VC.bits(score), VC.bits(want_score))
    s_labels, s_score = (_np(x) for x in hmm_viterbi((init, pair, node), return_score=True))
    assert np.array_equal(labels, s_labels)
    bound = VC.score_bound(init, pair, node[0])
    print("(%d, %d, %d) chunk %d: |score - serial| = %.3e = %.3f of the bound %.3e"
          % (B, T, K, pick, abs(score[0] - s_score[0]), abs(score[0] - s_score[0]) / bound, bound))
    assert abs(score[0] - s_score[0]) <= bound
