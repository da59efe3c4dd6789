"""CPU tests of the long-sequence HMM test infrastructure (oracle/hmm_longdouble.py, tests/_hmm_long_numpy.py), which
tests/test_hmm_long_hip.py runs the kernels against: the long-double oracle is pinned by the 60-digit restatement of
tests/test_hmm_range_cpu.py and by a second long-double algorithm; the fp64 oracle's own error at T = 22 785 is on record
(it cannot referee that regime); the NumPy restatement of the chunked kernels stays within C_SCALED / 8 of truth on every
LONG_SHAPES problem and flags none, and flags exactly the hostile sequences; the default-chunk rules on both sides of
every switch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_chunked_numpy as C  # noqa: E402
import _hmm_long_numpy as L  # noqa: E402
import _hmm_range_numpy as R  # noqa: E402
import _hmm_viterbi_chunked_numpy as VC  # noqa: E402
from oracle import hmm_longdouble  # noqa: E402
from test_hmm_range_cpu import _mp_estep  # noqa: E402

LD = np.longdouble
ALL_KEYS = [key for shape in L.LONG_SHAPES for key in L.parity_keys(shape)]


def _mp_problems():
    init, pair, node = C.parity_problem(1, 37, 4, 0, False)
    return [("ordinary T = 37, K = 4", (init, pair, node[0])), ("gap_case(8, 460, 30, 37)", R.case("gap", 8, 460.0, 30, 37))]


@pytest.mark.parametrize("algorithm", ["hmm_estep", "hmm_estep_scaled"])
def test_long_double_oracle_agrees_with_the_60_digit_restatement(algorithm):
    """both long-double algorithms against _mp_estep, elementwise relative, to 50 eps_ld T (2.0e-16 at T = 37).
    _mp_estep hands back fp64 numbers, so up to 2^-53 = 1.1e-16 of every difference is ITS rounding: measured 1.4e-16
    worst (log-space, gap_case), 1.1e-16 (scaled), log Z 4.4e-17.  An entry that the restatement rounds to 0 (state 1 at
    step 0 of gap_case, e^-10000) must round to 0 here too."""
    worst = 0.0
    for name, (init, pair, node) in _mp_problems():
        T = node.shape[0]
        unit = 50 * hmm_longdouble.EPS * T
        mz, ms, mt = _mp_estep(init, pair, node)
        lz, (ei, et, es) = getattr(hmm_longdouble, algorithm)((init, pair, node))
        assert all(x.dtype == LD for x in (np.asarray(lz), ei, et, es))
        assert np.array_equal(ei, es[0])
        for what, got, want in (("logZ", np.asarray(lz), np.asarray(mz)), ("E_states", es, ms), ("E_trans", et, mt)):
            zero = want == 0
            assert (got[zero].astype(float) == 0).all(), (name, what)
            err = L.rel_err(got[~zero], want[~zero])
            print("%s %s %s: %.2e (bound %.2e)" % (algorithm, name, what, err, unit))
            worst = max(worst, err / unit)
            assert err <= unit, (name, what, err, unit)
    print("worst / bound = %.3f" % worst)


def test_hmm_logZ_is_the_estep_log_normaliser_and_minus_infinity_entries_are_zero_terms():
    init, pair, node = (np.array(x) for x in L.sequence(("parity", 1, 141, 3, 2, False), 0))
    nat = (init, pair, node)
    assert hmm_longdouble.hmm_logZ(nat) == hmm_longdouble.hmm_estep(nat)[0]
    assert hmm_longdouble.hmm_logZ_scaled(nat) == hmm_longdouble.hmm_estep_scaled(nat)[0]
    # a forbidden transition, a forbidden start and an impossible observation: no nan, exact zeros where the path is cut
    pair[1, 0] = -np.inf
    init[2] = -np.inf
    node[70, 0] = -np.inf
    with np.errstate(all="raise"):
        a = hmm_longdouble.hmm_estep((init, pair, node))
    b = hmm_longdouble.hmm_estep_scaled((init, pair, node))
    for x, y in zip((a[0], *a[1]), (b[0], *b[1])):
        assert np.isfinite(x).all() and L.rel_err(y, x) < 1e-15
    assert a[1][1][1, 0] == 0 and a[1][0][2] == 0 and a[1][2][70, 0] == 0
    # no path at all: log Z = -inf, not nan
    init[:] = -np.inf
    assert hmm_longdouble.hmm_logZ((init, pair, node)) == -np.inf
    assert (hmm_longdouble.hmm_estep((init, pair, node))[1][2] == 0).all()


@pytest.mark.parametrize("key", ALL_KEYS, ids=str)
def test_log_space_and_scaled_long_double_agree(key):
    """two algorithms, one precision: 1e-15 relative on every output (measured worst 8e-18, at T = 22 785)"""
    worst = 0.0
    for b in range(key[1]):
        worst = max(worst, max(L.rel_err(x, y) for x, y in zip(L.truth_scaled(key, b), L.truth(key, b))))
    print("%s: worst relative difference %.2e" % (key, worst))
    assert worst <= 1e-15


def test_fp64_oracle_cannot_referee_22785_steps():
    """oracle/hmm_numpy against truth at (1, 22785, 8, 256): measured 3.0e-9 relative on E_states -- its log-messages
    reach |log Z| = 56 722 and every step rounds at 6e-12.  Why the long-double oracle exists; TOL_ORD's rtol 1e-8 is 3x
    that, and a kernel error below it is invisible against this oracle."""
    key = ("parity", 1, 22785, 8, 256, False)
    got, want = L.oracle64(key, 0), L.truth(key, 0)
    errs = [L.rel_err(x, y) for x, y in zip(got, want)]
    print("fp64 oracle vs truth: logZ %.2e  E_init %.2e  E_trans %.2e  E_states %.2e" % tuple(errs))
    assert max(errs[2], errs[3]) > 1e-10
    assert max(errs) < 1e-8                              # (still the oracle: wrong by rounding, not by a bug)


def test_restatement_against_truth():
    """_hmm_chunked_numpy.chunked_estep against truth on every LONG_SHAPES problem: no sequence flagged, and the worst
    |error| / (|truth| T 2^-53) is the one C_SCALED was taken from -- 2.253 at (2, 769, 8, 256) with (B,K,K) pair
    parameters, which _hmm_long_numpy records to two decimals as 2.25 = C_SCALED / 8 (the assertion allows that rounding
    and nothing else, so the constant cannot drift from its measurement)."""
    assert L.C_SCALED == 8 * L.WORST_RESTATEMENT_RATIO == 18.0
    worst = 0.0
    for key in ALL_KEYS:
        shape, ratio = key[1:5], 0.0
        for b in range(key[1]):
            got, flagged = L.restatement(key, b, key[4])
            assert not flagged, (key, b)
            r, what = L.scaled_ratio(got, key, b)
            ratio = max(ratio, r)
        print("%s: %.3f T eps (recorded %.2f)" % (key, ratio, L.RESTATEMENT_RATIO[shape][int(key[5])]))
        assert round(ratio, 2) <= L.RESTATEMENT_RATIO[shape][int(key[5])], key
        worst = max(worst, ratio)
    assert worst < L.C_SCALED / 8 + 0.005
    assert worst > L.C_SCALED / 16                       # ... nor the measurement from the constant


def test_restatement_flags_hostile_long_and_the_hostile_sequences_of_the_long_range_batch_only():
    init, pair, node, hostile = L.long_range_batch()
    assert node.shape == (130, 40, 2) and tuple(np.flatnonzero(hostile)) == L.RANGE_HOSTILE == (0, 63, 64, 65, 127, 128, 129)
    key = ("range",)
    flagged = np.array([L.restatement(key, b, L.RANGE_CHUNK)[1] for b in range(130)])
    assert (flagged == hostile).all(), np.flatnonzero(flagged != hostile)
    worst = max(L.scaled_ratio(L.restatement(key, b, L.RANGE_CHUNK)[0], key, b)[0] for b in np.flatnonzero(~hostile))
    print("benign sequences: restatement %.3f T eps" % worst)
    assert worst <= L.C_SCALED / 8
    for b in np.flatnonzero(hostile):                    # every one has a path of finite score
        assert np.isfinite(L.truth(key, b)[0])
    # hostile_long: flagged; what the fp64 oracle gets wrong on it is the redo bound's unit
    assert L.restatement(("hostile",), 0, L.HOSTILE_CHUNK)[1]
    lz = float(L.truth(("hostile",), 0)[0])
    errs = L.redo_errors(L.oracle64(("hostile",), 0), ("hostile",), 0)
    print("hostile_long: logZ %.4f; fp64 oracle vs truth: logZ rel %.1e  E_states abs %.1e  E_trans abs %.1e" % (lz, *errs))
    assert lz == pytest.approx(-800.87, abs=0.01)
    assert errs[0] < 1e-13 and errs[1] < 1e-10 and errs[2] < 1e-6


def test_default_chunk_rules_on_both_sides_of_every_switch():
    from svae_amd import _lib
    lib = _lib.load()
    estep, viterbi = lib.svae_hmm_chunked_default_chunk, lib.svae_hmm_chunked_viterbi_default_chunk
    want = {499: 499, 500: 32, 1422: 32, 1423: 64, 5688: 64, 5689: 128, 22755: 128, 22756: 256}
    for K in (1, 8, 16):
        for T, pick in want.items():
            for B in (1, 128):
                assert estep(B, T, K) == C.default_chunk(B, T, K) == pick, (B, T, K)
            assert estep(129, T, K) == C.default_chunk(129, T, K) == T, (T, K)
            # the decoder doubles its pick from 128 sequences up and stays chunked up to 256
            for B, p in ((1, pick), (127, pick), (128, min(2 * pick, T)), (129, min(2 * pick, T)), (256, min(2 * pick, T)),
                         (257, T)):
                assert viterbi(B, T, K) == VC.default_chunk(B, T, K) == (p if T >= 500 else T), (B, T, K)
    # the picks of the LONG_SHAPES that name one
    assert (estep(3, 5700, 5), estep(1, 22785, 8), estep(1, 22785, 16), estep(128, 500, 8)) == (128, 256, 256, 32)
