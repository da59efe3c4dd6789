"""The 50-digit arbiter of the global-step kernels (oracle/expfam_mp.py) checked on the CPU: against the NumPy restatement
and the reference's own golden values where fp64 is well conditioned, against itself at 80 digits where it is not, and the
validity of the comparison the GPU tests make (the fp64 host restatement within 1e-6 of the truth on every member of
tests/_global_step_families.py at the shapes checked here)."""
import os
import sys

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")
pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _global_step_families as F  # noqa: E402
from oracle import expfam_mp as em, expfam_numpy as ef, models_numpy  # noqa: E402


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert np.max(np.abs(got - want)) <= rel * max(np.max(np.abs(want)), 1e-300), (got, want)


def test_oracle_agrees_with_the_numpy_restatement_and_the_golden_values(golden_dir):
    g = np.load(os.path.join(golden_dir, "expfam.npz"))
    mniw = tuple(g["mniw_nat%d" % i] for i in range(4))
    for want in (g["dir_es"], ef.dirichlet_expectedstats(g["dir_nat"])):
        _close(em.dirichlet_expectedstats(g["dir_nat"]), want)
    for want in (g["niw_es"], ef.niw_expectedstats(g["niw_nat"])):
        _close(em.niw_expectedstats(g["niw_nat"]), want)
    got = em.mniw_expectedstats(mniw)
    for i, want in enumerate(ef.mniw_expectedstats(mniw)):
        _close(got[i], want)
        _close(got[i], g["mniw_es%d" % i])
    for got, key, fn in ((em.dirichlet_logZ(g["dir_nat"]), "dir_logZ", ef.dirichlet_logZ(g["dir_nat"])),
                         (em.niw_logZ(g["niw_nat"]), "niw_logZ", ef.niw_logZ(g["niw_nat"])),
                         (em.mniw_logZ(mniw), "mniw_logZ", ef.mniw_logZ(mniw))):
        _close(got, g[key])
        _close(got, fn)


def test_oracle_prior_kls_agree_with_the_numpy_restatement_on_well_conditioned_parameters(golden_dir):
    g = np.load(os.path.join(golden_dir, "expfam.npz"))
    K = g["niw_nat"].shape[0]
    glob, prior = (g["dir_nat"][0], g["niw_nat"]), (g["dir_nat"][1], g["niw_nat"][::-1].copy())
    kl = em.gmm_prior_kl(glob, prior)
    assert kl.full == pytest.approx(models_numpy.gmm_prior_kl(glob, prior), abs=1e-12 * kl.scale)
    es0 = ef.dirichlet_expectedstats(glob[0])[0]
    logZ = lambda q: ef.dirichlet_logZ(q[0]) + ef.niw_logZ(q[1])
    shipped = (glob[0][0] - prior[0][0]) * es0 - (logZ(glob) - logZ(prior))           # the reference AS SHIPPED
    assert kl.shipped == pytest.approx(shipped, abs=1e-12 * kl.scale)
    assert kl.scale >= abs(kl.full) and K == len(glob[0])
    lg, lp, _, _ = F.lds_truth(3, "A-M1e2")[:4]
    lkl = em.lds_prior_kl(lg, lp)
    assert lkl.full == pytest.approx(models_numpy.lds_prior_kl(lg, lp), abs=1e-12 * lkl.scale)
    assert lkl.shipped == lkl.full                    # lds.py:19 contracts with `contract`, not `flat`
    # a factor against itself: exactly the difference of two identical log-normalisers
    assert em.gmm_prior_kl(glob, glob).full == 0.0 and em.lds_prior_kl(lg, lg).full == 0.0


def _rel_mp(a, b):
    a, b = np.asarray(a, dtype=object).reshape(-1), np.asarray(b, dtype=object).reshape(-1)
    return max(abs(x - y) for x, y in zip(a, b)) / max(abs(y) for y in b)


@pytest.mark.parametrize("member", ["B-1e4-M1e8", "D-1e8", "F-1e-6"])
def test_fifty_digits_are_enough(member):
    """dps = 50 against dps = 80 on the members that cancel most (off-centre mean at nu = 1e8: 24 digits lost at worst;
    cond 1e8; units 1e-12): every output to 1e-30, so the float64 truths the GPU tests use are the correctly rounded maps"""
    (niw, mniw), prior = F.lds_case(10, member)
    glob_g, prior_g = F.gmm_case(5, 2, member)
    pairs = [(em.niw_expectedstats(niw, dps=d, as_float=False), em.mniw_expectedstats(mniw, dps=d, as_float=False),
              em.niw_logZ(niw, dps=d, as_float=False), em.mniw_logZ(mniw, dps=d, as_float=False),
              em.lds_prior_kl((niw, mniw), prior, dps=d), em.gmm_prior_kl(glob_g, prior_g, dps=d),
              em.dirichlet_expectedstats(glob_g[0], dps=d, as_float=False)) for d in (50, 80)]
    a, b = pairs
    old = mp.mp.dps
    mp.mp.dps = 80
    try:
        n = niw.shape[-1] - 2
        assert _rel_mp(a[0][:n, :n], b[0][:n, :n]) < 1e-30 and _rel_mp(a[0][:n, n], b[0][:n, n]) < 1e-30
        assert _rel_mp(a[0][n, n], b[0][n, n]) < 1e-30 and _rel_mp(a[0][n + 1, n + 1], b[0][n + 1, n + 1]) < 1e-30
        for i in range(3):
            assert _rel_mp(a[1][i], b[1][i]) < 1e-30
        assert _rel_mp(a[1][3], b[1][3]) < 1e-30 and _rel_mp(a[2], b[2]) < 1e-30 and _rel_mp(a[3], b[3]) < 1e-30
        for i in (4, 5):
            assert abs(a[i].full_mp - b[i].full_mp) < 1e-30 * b[i].scale_mp
            assert abs(a[i].shipped_mp - b[i].shipped_mp) < 1e-30 * b[i].scale_mp
        assert _rel_mp(a[6], b[6]) < 1e-30
    finally:
        mp.mp.dps = old


@pytest.mark.parametrize("K,N", [(5, 2), (3, 8), (3, 16)])
def test_every_gmm_member_is_a_valid_comparison(K, N):
    """e_ref <= 1e-6: the host restatement itself is a meaningful yardstick on every member (worst seen: 2.2e-8, E_h at
    |m| = 1e4, nu = 1e8), and at its floor of a few ulp on the centred ones"""
    for member in F.GMM_MEMBERS:
        e_ref = F.gmm_truth(K, N, member)[3]
        assert max(e_ref.values()) <= F.E_REF_MAX, (member, e_ref)
        if member.startswith("A-"):
            assert max(e_ref.values()) <= 1e-13, (member, e_ref)


@pytest.mark.parametrize("n", [10, 17])
def test_every_lds_member_is_a_valid_comparison(n):
    """the same for the (NIW, MNIW) pair (worst seen: 2.6e-7, the pair blocks of D-1e8 at n = 17; the D-1e8 member carries
    cond(K) = 1e2 -- with cond(K) = 1e4 the restatement is off by 1e-3 and with 1e8 by 100 %, see lds_case)"""
    for member in F.LDS_MEMBERS:
        e_ref = F.lds_truth(n, member)[3]
        assert max(e_ref.values()) <= F.E_REF_MAX, (member, e_ref)
        if member.startswith("A-"):
            assert max(e_ref.values()) <= 1e-13, (member, e_ref)
