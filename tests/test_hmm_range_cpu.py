"""CPU checks of the cases in tests/_hmm_range_numpy.py, which tests/test_hmm_range_hip.py runs through the kernels:
the oracle is accurate on them (against a 60-digit mpmath restatement), a plain scaled recursion gets them wrong with
ordinary normalisers (the cases have teeth), the bracketing cases are within a scaled recursion's range, and the
posterior really uses the deep transition.  (No sampler cases: hmm_sample's range is not part of this change.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_range_numpy as R  # noqa: E402

ALL_K = R.K_ROW + R.K_WIDE
LZ_REL, ST_RTOL, ST_ATOL, TR_ATOL = R.LZ_REL, R.ST_RTOL, R.ST_ATOL, R.TR_ATOL


def _mp_estep(init, pair, node, dps=60):
    """the log-space forward-backward of oracle/hmm_numpy.hmm_estep in `dps`-digit arithmetic"""
    import mpmath
    mp = mpmath.mp
    old = mp.dps
    mp.dps = dps
    try:
        T, K = node.shape
        f = lambda x: mpmath.mpf(float(x))
        ini, nd = [f(x) for x in init], [[f(x) for x in row] for row in node]
        pr = [[f(x) for x in row] for row in pair]

        def lse(xs):
            m = max(xs)
            return m + mpmath.log(sum(mpmath.exp(x - m) for x in xs))
        la = [[ini[k] + nd[0][k] for k in range(K)]]
        for t in range(1, T):
            la.append([lse([la[t - 1][j] + pr[j][k] for j in range(K)]) + nd[t][k] for k in range(K)])
        lb = [[mpmath.mpf(0)] * K for _ in range(T)]
        for t in range(T - 2, -1, -1):
            lb[t] = [lse([pr[j][k] + nd[t + 1][k] + lb[t + 1][k] for k in range(K)]) for j in range(K)]
        logZ = lse(la[T - 1])
        Es = np.array([[float(mpmath.exp(la[t][k] + lb[t][k] - logZ)) for k in range(K)] for t in range(T)])
        Et = np.zeros((K, K))
        for j in range(K):
            for k in range(K):
                Et[j, k] = float(sum(mpmath.exp(la[t][j] + pr[j][k] + nd[t + 1][k] + lb[t + 1][k] - logZ)
                                     for t in range(T - 1)))
        return float(logZ), Es, Et
    finally:
        mp.dps = old


ORACLE_SAMPLE = [("gap", 2, 800.0, 2, 4), ("gap", 3, 745.0, 5, 12), ("gap", 9, 3000.0, 8, 13), ("gap", 8, 460.0, 30, 37),
                 ("surprise", 3, 460.0, 140.0, 3, 10), ("surprise", 8, 600.0, 60.0, 2, 11),
                 ("sparse", 2, 1e-3, 200.0, 8, 24, 0), ("sparse", 9, 5e-4, 400.0, 8, 24, 1), ("sparse", 16, 1e-2, 20.0, 8, 24, 0),
                 ("sparse", 17, 1e-3, 200.0, 8, 24, 0), ("ramp", 3, 800.0, 50.0, 24, 3, 45), ("ramp", 8, 1200.0, 50.0, 36, 4, 45)]


def test_oracle_agrees_with_a_60_digit_restatement():
    """oracle/hmm_numpy.hmm_estep against _mp_estep on a sample of every family.  Worst figures over ORACLE_SAMPLE:
    log Z 5.1e-16 relative, E_states 1.8e-12 absolute, E_trans 1.7e-11 absolute -- the GPU file's tolerances (1e-9
    relative, 1e-10 and 1e-9 absolute) are more than 10x these, which is asserted."""
    worst = np.zeros(3)
    for key in ORACLE_SAMPLE:
        init, pair, node = R.case(*key)
        lz, (_, ot, os_) = R.reference(*key)
        mz, ms, mt = _mp_estep(init, pair, node)
        err = np.array([abs(lz - mz) / abs(mz), np.abs(os_ - ms).max(), np.abs(ot - mt).max()])
        print(key, "logZ rel %.1e  E_states abs %.1e  E_trans abs %.1e" % tuple(err))
        worst = np.maximum(worst, err)
    print("worst: logZ rel %.1e  E_states abs %.1e  E_trans abs %.1e" % tuple(worst))
    assert 10 * worst[0] <= LZ_REL and 10 * worst[1] <= ST_ATOL and 10 * worst[2] <= TR_ATOL


def _all_keys(K):
    keys = [k for T in R.GAP_T for k in R.gap_keys(K, T, R.GAP_G)] + R.sparse_keys(K) + R.ramp_keys(K)
    return keys + (R.surprise_keys(K) if K >= 3 else [])


_off = R.off


def test_minimal_case_is_the_documented_one():
    """K = 2, T = 4: log Z = -800 + log 3 and a last marginal of (1/3, 2/3); the scaled recursion says -800 and
    (1, 0) with a smallest normaliser of 1.9e-174"""
    key = ("gap", 2, 800.0, 2, 4)
    lz, (_, _, es) = R.reference(*key)
    assert lz == pytest.approx(-800 + np.log(3), rel=1e-14)
    np.testing.assert_allclose(es[-1], [1 / 3, 2 / 3], rtol=1e-12)
    slz, (_, _, ses), cmin = R.scaled_emulation(*R.case(*key))
    assert slz == -800.0 and cmin == pytest.approx(1.9e-174, rel=0.05)
    assert not np.isfinite(ses).all() or ses[-1, 0] == 1.0


@pytest.mark.parametrize("K", ALL_K)
def test_cases_have_teeth_and_their_story_is_real(K):
    """Every case whose story goes through a potential >= 745 nats below the maximum: the oracle's posterior puts more than
    0.1 of its mass on such transitions, the plain scaled recursion is non-finite or more than 100x the GPU tolerances
    off, and its smallest normaliser stays above 1e-200 -- the flag of a normaliser test would not fire.  (Not the last
    for gap_case with g = 1200 and 3000: their evidence of g / 2 per step drives the normaliser itself down to e^-g/2.)
    Every other case is within a per-step scaled recursion's range: it agrees to the GPU tolerances."""
    n_ext = 0
    for key in _all_keys(K):
        got, want = R.scaled_emulation(*R.case(*key)), R.reference(*key)
        deep = R.deep_mass(R.case(*key)[1], want[1][1])
        if key[0] == "surprise" and R.by_construction_extreme(*key):
            # no deep transition, but state 1's component e^-g meets a likelihood of e^-s in the surprise steps: below
            # 1e-308 of the step's best, whatever the renormalisation
            assert deep < 1e-9 and got[2] > 1e-200, key
            assert _off(got, want, 100.0), key
        elif R.by_construction_extreme(*key):
            n_ext += 1
            assert deep > 0.1, key
            assert _off(got, want, 100.0), key
            if not (key[0] == "gap" and key[2] > 800.0):
                assert got[2] > 1e-200, (key, got[2])
        else:
            assert deep < 1e-9, key
            assert not _off(got, want, 1.0), key
    assert n_ext >= 4 * 26 + 4 + 12


@pytest.mark.parametrize("K", [k for k in ALL_K if k >= 3])
def test_surprise_cases_bite_a_recursion_that_renormalises_every_fourth_step(K):
    """per-step renormalisation handles every surprise case (asserted above); with the two-ended kernel's schedule the
    component at e^-g meets an unnormalised total of e^-(r s): for s = 140, r = 3 some phase of the event start is off"""
    for g in R.SURPRISE_G:
        off = []
        for t0 in R.SURPRISE_T0:
            key = ("surprise", K, g, 140.0, 3, t0)
            lz4, lz = R.scaled_logZ(*R.case(*key)), R.reference(*key)[0]
            off.append(not np.isfinite(lz4) or abs(lz4 - lz) > 100 * LZ_REL * abs(lz))
        assert any(off), (K, g)


@pytest.mark.parametrize("K", ALL_K)
def test_mixed_batches_hold_what_they_say(K):
    """blocks of four rows with 0, 1, 2 and 4 extreme rows (K <= 16); the rows marked extreme are the oracle's own
    (deep mass > 0.1); the ragged variant cuts one extreme row before its event, one two steps after it"""
    counts = set()
    for variant in ("shared", "shared4", "batched", "ragged"):
        m = R.mixed_batch(K, variant)
        B = m["node"].shape[0]
        assert B == (11 if K <= 16 else 5)
        ext = np.zeros(B, bool)
        ext[list(m["ext"])] = True
        if variant != "ragged":
            assert np.array_equal(m["extreme"], ext)
            counts |= {int(ext[i:i + 4].sum()) for i in range(0, B, 4)}
        else:
            L = m["lengths"]
            assert L[m["ext"][0]] == 8 and L[m["ext"][1]] == 10 and not m["extreme"][m["ext"][0]]
            assert m["extreme"][list(m["ext"][2:])].all() and not m["extreme"][~ext].any()
            assert all(np.isnan(m["node"][b, L[b]:]).all() and np.isfinite(m["node"][b, :L[b]]).all() for b in range(B))
            assert {1, 2, 24} <= set(L.tolist())
    if K <= 16:
        assert counts == {0, 1, 2, 4}
