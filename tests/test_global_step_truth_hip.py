"""The four global-step kernels (svae_gmm_global_step_f64, svae_gmm_wide_global_step_f64, svae_lds_global_step_f64,
svae_lds_global_step_multi_f64) against a 50-digit evaluation of the maps they implement (oracle/expfam_mp.py), away from
the one point of the parameter space -- alpha ~ 1, kappa ~ 1..3, nu ~ n + 3, centred mean -- the older tests sit at.

Parameters: tests/_global_step_families.py (families A-F: posteriors after up to 1e8 observations, off-centre means,
barely valid parameters, ill-conditioned scale matrices, unbalanced Dirichlets, units), handed as ONE float64 natural
parameter to kernel, host restatement and oracle.

The bound is relative to the fp64 host restatement's own error e_ref (oracle/expfam_numpy.py, pivoted LAPACK) against the
same truth under the same measure:

    e_kernel <= 16 max(e_ref, 64 eps)          and   e_ref <= 1e-6 (the comparison must not certify noise)

because the inherent fp64 error of these maps runs from 1e-16 (centred) to 1e-7 (|m| = 1e4 at nu = 1e8): the kernels
eliminate without pivoting in another order, a different sample of the same conditioning.  Measures: a matrix or vector
block max|got - truth| / max|truth|; a scalar ending in psi / log-det sums |got - truth| / max(|truth|, 1); a KL
|got - truth| / (|<d eta, E t>| + |log Z(q)| + |log Z(p)|).  Each output is held to its own e_ref.  Every figure is
printed before it is asserted (`GSTRUTH` lines, pytest -s); the worst per kernel and family are tabulated in DESIGN.md
section 4.6a, whose source these lines are.

Two outputs are over the bound on an MI355X and are named exceptions (_global_step_families.EXCEPTIONS, with the reason):
the MNIW's log-normaliser at n = 64, B-1e2-M1e4 (75 x its own e_ref) and at n = 16, B-1e2-M0 (16.3 x the floor).  They
alone are held to the worst e_ref of their factor instead.  Every other output of every case is within 13.3.

The digamma's non-terminating inputs (-inf, -1e16, ..) never come near a kernel here: tests/test_special_fn_cpu.py checks
them on the host.  The invalid parameters below are finite and <= 10 in magnitude."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("mpmath")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _global_step_families as F  # noqa: E402
from oracle import expfam_mp as em, expfam_numpy as ef  # noqa: E402  (checkers only)

GMM_SHAPES = [(1, 1), (5, 2), (64, 2), (3, 8), (2, 9), (3, 16)]      # N <= 8: one lane per component; N >= 9: the wide kernel
LDS_NS = [1, 10, 16, 17, 33]                                          # both sides of the n n <= 256 inverse split
DEV = "cuda:0"


def _d(x):
    if isinstance(x, (tuple, list)):
        return tuple(_d(y) for y in x)
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=DEV)


def _np(x):
    if isinstance(x, (tuple, list)):
        return tuple(_np(y) for y in x)
    return x.detach().cpu().numpy()


def _word():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _flagged_or_finite(info, *outputs):
    """no output of this module may hold a non-finite value while info == 0"""
    flat = [np.asarray(o, float).reshape(-1) for o in outputs if o is not None]
    if int(info.item()) == 0:
        assert all(np.all(np.isfinite(o)) for o in flat), "non-finite output with info == 0"


def _gmm_call(glob, prior):
    """-> (label_global, gaussian_globals, kl as spelled, kl as shipped, info) of gmm.global_step"""
    from svae_amd.models import gmm
    info = _word()
    lg, gg, kl = gmm.global_step(_d(glob), _d(prior), info=info, reference_compat=False)
    lg2, gg2, kls = gmm.global_step(_d(glob), _d(prior), info=info, reference_compat=True)
    bits = lambda x: _np(x).view(np.int64)               # (NaN potentials of an invalid component compare by bits)
    assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(bits(gg), bits(gg2))
    out = _np(lg), _np(gg), float(kl), float(kls)
    _flagged_or_finite(info, *out)
    return out + (info,)


def _lds_call(glob, prior):
    """-> (init, pair, niw_es, kl, info) of lds.global_step"""
    from svae_amd.models import lds as lds_model
    info = _word()
    (init, pair), kl, es = lds_model.global_step(_d(glob), _d(prior) if prior is not None else None, info=info)
    out = _np(init), _np(pair), _np(es), (float(kl) if kl is not None else None)
    _flagged_or_finite(info, *(out[0] + out[1] + (out[2], out[3])))
    return out + (info,)


# --- the kernels against the oracle ----------------------------------------------------------------------------------

@pytest.mark.parametrize("member", F.GMM_MEMBERS)
@pytest.mark.parametrize("K,N", GMM_SHAPES)
def test_gmm_global_step_against_the_50_digit_oracle(K, N, member):
    glob, prior, truth, e_ref = F.gmm_truth(K, N, member)
    lg, gg, kl, kls, info = _gmm_call(glob, prior)
    bad = F.check(F.gmm_errors(lg, gg, kl, kls, truth), e_ref,
                  "%s K=%d N=%d %s" % ("gmm" if N <= 8 else "gmm_wide", K, N, member))
    assert int(info.item()) == 0
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("member", F.LDS_MEMBERS)
@pytest.mark.parametrize("n", LDS_NS)
def test_lds_global_step_against_the_50_digit_oracle(n, member):
    glob, prior, truth, e_ref = F.lds_truth(n, member)
    init, pair, es, kl, info = _lds_call(glob, prior)
    bad = F.check(F.lds_errors(init, pair, es, kl, truth), e_ref, "lds n=%d %s" % (n, member))
    assert int(info.item()) == 0
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("member", F.N64_MEMBERS)
def test_lds_global_step_at_the_largest_dimension_against_stored_truths(member, golden_dir):
    """n = 64, one member per family: truths from tests/golden/make_golden_global_step.py (~10 s of mpmath each)"""
    g = np.load(os.path.join(golden_dir, "global_step_n64_%s.npz" % member))
    glob = (g["niw"], (g["A"], g["B"], g["C"], g["d"]))
    prior = (g["prior_niw"], (g["prior_A"], g["prior_B"], g["prior_C"], g["prior_d"]))
    truth = (g["es"], (g["J11"], g["J12"], g["J22"], float(g["logZ_pair"])), float(g["logZ"]),
             em.KL(float(g["kl_full"]), float(g["kl_shipped"]), float(g["kl_scale"]), None, None, None))
    e_ref = F.lds_reference_errors(glob, prior, truth)
    init, pair, es, kl, info = _lds_call(glob, prior)
    bad = F.check(F.lds_errors(init, pair, es, kl, truth), e_ref, "lds n=64 %s" % member)
    assert int(info.item()) == 0
    assert not bad, "\n".join(bad)


def _slds_maps(hmm_global, lds_global):
    from svae_amd.models import slds_svae
    out = slds_svae.global_to_local_maps((_d(hmm_global), [(_d(a), _d(m)) for a, m in lds_global]), torch.device(DEV))
    info = slds_svae.global_to_local_maps.last_info
    hmm_init, hmm_pair, dense_init, dense_pair = _np(out[0]), _np(out[1]), _np(out[2]), _np(out[3])
    _flagged_or_finite(info, hmm_init, hmm_pair, *(dense_init + dense_pair))
    return hmm_init, hmm_pair, dense_init, dense_pair, info


def _hmm_global(K, rng):
    """Dirichlet natural parameters (alpha - 1) of the initial state and the K rows; row K // 2 is family E's: one
    alpha = 1e8, the rest 1e-3"""
    init, rows = 0.5 + rng.random(K), 0.5 + rng.random((K, K))
    rows[K // 2] = 1e-3
    rows[K // 2, 0] = 1e8
    return init - 1., rows - 1.


@pytest.mark.parametrize("K,n", [(1, 4), (16, 10)])
def test_slds_multi_launch_against_the_50_digit_oracle_per_state(K, n):
    """svae_lds_global_step_multi_f64: state k carries member k of the LDS families (K = 16: all sixteen of them), each
    judged against the oracle like a single launch; the HMM rows (torch digamma on the device) against the oracle too"""
    members = F.LDS_MEMBERS[:K] if K > 1 else ["A-M1e4"]
    cases = [F.lds_truth(n, m) for m in members]
    hmm_global = _hmm_global(K, np.random.default_rng(K))
    hmm_init, hmm_pair, dense_init, dense_pair, info = _slds_maps(hmm_global, [c[0] for c in cases])
    assert int(info.item()) == 0
    bad = []
    for k, (glob, prior, truth, e_ref) in enumerate(cases):
        init = (dense_init[0][k], dense_init[1][k], dense_init[2][k] + dense_init[3][k])
        pair = tuple(x[k] for x in dense_pair)
        es = ef.pack_dense(dense_init[0][k], dense_init[1][k], dense_init[2][k], dense_init[3][k])
        e_ref = {q: v for q, v in e_ref.items() if q != "kl"}
        bad += F.check(F.lds_errors(init, pair, es, None, truth), e_ref, "lds_multi K=%d n=%d %s" % (K, n, members[k]))
    e = {"hmm_init": F.e_scalar(hmm_init, em.dirichlet_expectedstats(hmm_global[0])),
         "hmm_pair": F.e_scalar(hmm_pair, em.dirichlet_expectedstats(hmm_global[1]))}
    r = {"hmm_init": F.e_scalar(ef.dirichlet_expectedstats(hmm_global[0]), em.dirichlet_expectedstats(hmm_global[0])),
         "hmm_pair": F.e_scalar(ef.dirichlet_expectedstats(hmm_global[1]), em.dirichlet_expectedstats(hmm_global[1]))}
    bad += F.check(e, r, "slds_hmm_rows K=%d" % K)
    assert not bad, "\n".join(bad)


# --- identities ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,N", [(5, 2), (3, 8), (3, 16)])
def test_gmm_kl_of_a_factor_against_itself_is_zero_to_rounding(K, N):
    """KL(q || q) at nu = 1e8: the kernel inverts the global factor and only eliminates the prior (two variants of the same
    elimination), so the two log-normalisers ~ N nu log nu / 2 need not cancel exactly -- but to 16 x 64 eps of them"""
    glob = F.gmm_truth(K, N, "A-M1e8")[0]
    scale = em.gmm_prior_kl(glob, glob).scale
    _, _, kl, kls, info = _gmm_call(glob, glob)
    print("GSTRUTH gmm KL(q||q) K=%d N=%d: %.3e and %.3e of scale %.3e" % (K, N, kl, kls, scale))
    assert int(info.item()) == 0
    assert abs(kl) <= F.FACTOR * F.FLOOR * scale and abs(kls) <= F.FACTOR * F.FLOOR * scale


@pytest.mark.parametrize("n", [10, 17])
def test_lds_kl_of_a_factor_against_itself_is_zero_to_rounding(n):
    glob, _, truth, _ = F.lds_truth(n, "A-M1e8")
    scale = 2 * abs(truth[2])                       # |<0, E t>| + |log Z(q)| + |log Z(q)|
    _, _, _, kl, info = _lds_call(glob, glob)
    print("GSTRUTH lds KL(q||q) n=%d: %.3e of scale %.3e" % (n, kl, scale))
    assert int(info.item()) == 0
    assert abs(kl) <= F.FACTOR * F.FLOOR * scale


def _stats_step(n, rng, count=10):
    """the statistics of `count` observations, the direction a natural-gradient step moves a NIW along"""
    x = rng.standard_normal((count, n))
    return ef.pack_dense(x.T @ x, x.sum(0), np.array(float(count)), np.array(float(count)))


@pytest.mark.parametrize("K,N", [(5, 2), (3, 8), (3, 16)])
def test_gmm_kl_after_a_small_step(K, N):
    """q = p + 1e-3 x (statistics of a few observations) at p = A-M1e4: a KL of order 1e-6 .. 1e-3 out of log-normalisers
    of order 1e5 -- within the bound of the oracle's value, and not negative by more than the bound"""
    rng = np.random.default_rng(100 * K + N)
    p = F.gmm_truth(K, N, "A-M1e4")[0]
    q = (p[0] + 1e-3 * rng.random(K) * 10, p[1] + 1e-3 * np.stack([_stats_step(N, rng) for _ in range(K)]))
    truth = em.gmm_global_step(q, p)
    e_ref = F.gmm_reference_errors(q, p, truth)
    lg, gg, kl, kls, info = _gmm_call(q, p)
    e = F.gmm_errors(lg, gg, kl, kls, truth)
    assert int(info.item()) == 0 and truth[2].full > 0
    bad = F.check({k: e[k] for k in ("kl", "kl_shipped")}, e_ref, "gmm small step K=%d N=%d" % (K, N))
    assert not bad, "\n".join(bad)
    assert kl >= -F.FACTOR * max(e_ref["kl"], F.FLOOR) * truth[2].scale


@pytest.mark.parametrize("n", [10, 17])
def test_lds_kl_after_a_small_step(n):
    rng = np.random.default_rng(n)
    p = F.lds_truth(n, "A-M1e4")[0]
    x, y = rng.standard_normal((10, n)), rng.standard_normal((10, n))
    A, B, C, d = p[1]
    q = (p[0] + 1e-3 * _stats_step(n, rng), (A + 1e-3 * x.T @ x, B + 1e-3 * x.T @ y, C + 1e-3 * y.T @ y, d + 1e-3 * 10))
    truth = em.lds_global_step(q, p)
    e_ref = F.lds_reference_errors(q, p, truth)
    init, pair, es, kl, info = _lds_call(q, p)
    assert int(info.item()) == 0 and truth[3].full > 0
    bad = F.check({"kl": F.lds_errors(init, pair, es, kl, truth)["kl"]}, e_ref, "lds small step n=%d" % n)
    assert not bad, "\n".join(bad)
    assert kl >= -F.FACTOR * max(e_ref["kl"], F.FLOOR) * truth[3].scale


# --- invalid parameters: mildly so (finite, magnitude <= 10), one component or state among valid ones -------------------

def _gmm_invalid(glob, k, what):
    dn, nn = glob[0].copy(), glob[1].copy()
    N = nn.shape[-1] - 2
    if what == "nu":
        nn[k, N + 1, N + 1] = N - 1.5
    elif what == "kappa":
        nn[k, N, N] = -1.0                       # (S = A + b b' stays positive definite: only kappa is wrong)
    elif what == "alpha":
        dn[k] = -1.5                             # alpha = -0.5
    else:
        nn[k, :N, :N] = -nn[k, :N, :N]           # an indefinite scale matrix
    return dn, nn


@pytest.mark.parametrize("what", ["nu", "kappa", "alpha", "indefinite"])
@pytest.mark.parametrize("K,N", [(5, 2), (3, 9)])
def test_gmm_global_step_reports_an_invalid_component_and_leaves_the_valid_ones_alone(K, N, what):
    """nu <= N - 1, kappa <= 0 and alpha <= 0 pass every pivot test and used to come back as NaN or garbage potentials
    with info == 0; the valid components' outputs are those of the all-valid call bit for bit (the Dirichlet rows share
    sum alpha, so with an invalid alpha only the NIW outputs can be compared that way)"""
    glob, prior = F.gmm_case(K, N, "A-M0")
    k = K // 2
    lg0, gg0, _, _, info0 = _gmm_call(glob, prior)
    assert int(info0.item()) == 0
    lg, gg, kl, kls, info = _gmm_call(_gmm_invalid(glob, k, what), prior)
    assert int(info.item()) != 0
    valid = [j for j in range(K) if j != k]
    assert np.array_equal(gg[valid], gg0[valid])
    if what != "alpha":
        assert np.array_equal(lg[valid], lg0[valid])
    # the same defect in the PRIOR is reported too
    _, _, _, _, info_p = _gmm_call(glob, _gmm_invalid(prior, k, what))
    assert int(info_p.item()) != 0


def _lds_invalid(glob, what):
    niw, (A, B, C, d) = glob[0].copy(), glob[1]
    n = niw.shape[-1] - 2
    if what == "nu":
        niw[n + 1, n + 1] = n - 1.5
    elif what == "kappa":
        niw[n, n] = -1.0
    elif what == "mniw_nu":
        d = np.array(n - 1.5)
    else:
        A = -A                                   # K^-1 negative definite (the case the older tests have)
    return niw, (A, B, C, d)


@pytest.mark.parametrize("what", ["nu", "kappa", "mniw_nu", "indefinite"])
@pytest.mark.parametrize("n", [4, 17])
def test_lds_global_step_reports_invalid_parameters(n, what):
    glob, prior = F.lds_case(n, "A-M0")
    assert int(_lds_call(glob, prior)[4].item()) == 0
    assert int(_lds_call(_lds_invalid(glob, what), prior)[4].item()) != 0
    assert int(_lds_call(glob, _lds_invalid(prior, what))[4].item()) != 0      # the prior's pass reports as well
    assert int(_lds_call(_lds_invalid(glob, what), None)[4].item()) != 0       # and the launch without a prior


@pytest.mark.parametrize("what", ["nu", "kappa", "mniw_nu", "indefinite"])
def test_slds_multi_launch_reports_an_invalid_state_and_leaves_the_valid_ones_alone(what):
    from svae_amd.models import slds_svae
    K, n = 3, 4
    globs = [F.lds_case(n, m)[0] for m in ("A-M0", "A-M1e2", "A-M1e4")]
    rng = np.random.default_rng(3)
    hmm_global = (0.5 + rng.random(K) - 1., 0.5 + rng.random((K, K)) - 1.)
    good = _slds_maps(hmm_global, globs)
    assert int(good[4].item()) == 0
    broken = _slds_maps(hmm_global, [globs[0], _lds_invalid(globs[1], what), globs[2]])
    assert int(broken[4].item()) != 0
    with pytest.raises(FloatingPointError):
        slds_svae.check_info()                   # (reads and clears the persistent word)
    slds_svae.check_info()
    for k in (0, 2):
        for got, want in zip(broken[2] + broken[3], good[2] + good[3]):
            assert np.array_equal(got[k], want[k])
