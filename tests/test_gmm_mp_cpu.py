"""oracle/gmm_mp.py (the 50-digit GMM local step) pinned before it judges a kernel, and the conditions under which
tests/test_gmm_truth_hip.py's comparisons are valid, checked with the reference alone -- no GPU.

  * the oracle agrees with the fp64 restatement oracle/gmm_numpy.py on ordinary inputs, with itself at another working
    precision, and with one sweep at T = 3, K = 2, N = 1 written out by hand;
  * local_tail_jvp_mp agrees with torch double-precision autograd of tests/_gmm_torch.py;
  * for every case of the GPU file: the generator is deterministic, every Gaussian factor is positive definite, the
    restatement's own error e_ref is finite and small enough to be a yardstick, at most 5 % of the points are exempt from
    the `assign` comparison, and the six stopping cases are admissible."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("mpmath")
pytest.importorskip("scipy")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmm_families as F  # noqa: E402
from oracle import gmm_mp  # noqa: E402

E_REF_MAX = 1e-6        # beyond this the restatement is no yardstick (tests/_global_step_families.py's bound)


def _args(c):
    return c["label_global"], c["gaussian_globals"], (c["node_J"], c["node_h"]), c["label_init"]


# --- the oracle itself -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,T,m", [(1, 3, 7, 0), (2, 5, 24, 3), (3, 4, 9, 1), (9, 3, 5, 2)])
def test_oracle_agrees_with_the_fp64_restatement_on_ordinary_inputs(N, K, T, m):
    c, tr, ref, e = F.truth("plain", N, K, T, m)
    assert tr["iters"] == ref["iters"] == m
    for k, v in e.items():
        assert v < 1e-12, (k, v)
    if m:
        assert np.max(np.abs(tr["kl_hist"] - ref["kl_hist"])) < 1e-12 * np.max(np.abs(tr["kl_hist"]))


def test_oracle_agrees_with_itself_at_30_and_60_digits():
    import mpmath as mp
    c = F.case("plain", 3, 4, 6)
    a = gmm_mp.local_meanfield_mp(*_args(c), tol=0.0, max_iter=2, dps=30, as_float=False)
    b = gmm_mp.local_meanfield_mp(*_args(c), tol=0.0, max_iter=2, dps=60, as_float=False)
    with gmm_mp._digits(60):
        for k in gmm_mp.KEYS:
            if k == "iters":
                assert a[k] == b[k] == 2
                continue
            x, y = np.asarray(a[k], dtype=object).reshape(-1), np.asarray(b[k], dtype=object).reshape(-1)
            scale = max(abs(v) for v in y)
            assert max(abs(u - v) for u, v in zip(x, y)) <= mp.mpf("1e-25") * scale, k


def test_one_sweep_at_T3_K2_N1_equals_the_closed_form_written_out():
    """N = 1: J = -2 A, E x = h / J, E x^2 = 1 / J + (E x)^2, log Z = h^2 / (2 J) - log(J) / 2 + c + d"""
    import mpmath as mp
    c = F.case("plain", 1, 2, 3)
    out = gmm_mp.local_meanfield_mp(*_args(c), tol=0.0, max_iter=1, dps=50, as_float=False)
    with gmm_mp._digits(50):
        f = lambda x: mp.mpf(float(x))
        G = c["gaussian_globals"]
        Ak, bk, ck, dk = ([f(G[k][i, j]) for k in range(2)] for i, j in ((0, 0), (0, 1), (1, 1), (2, 2)))
        lg = [f(v) for v in c["label_global"]]

        def one_pass(t, r):
            nJ, nh = f(c["node_J"][t, 0]), f(c["node_h"][t, 0])
            A, h = nJ + r[0] * Ak[0] + r[1] * Ak[1], nh + r[0] * bk[0] + r[1] * bk[1]
            cc, dd = r[0] * ck[0] + r[1] * ck[1], r[0] * dk[0] + r[1] * dk[1]
            J = -2 * A
            Ex = h / J
            Exx = 1 / J + Ex * Ex
            logZ = h * h / (2 * J) - mp.log(J) / 2 + cc + dd
            l = [Exx * Ak[k] + Ex * bk[k] + ck[k] + dk[k] for k in range(2)]
            n = [l[k] + lg[k] for k in range(2)]
            lse = mp.log(mp.exp(n[0]) + mp.exp(n[1]))
            rn = [mp.exp(n[k] - lse) for k in range(2)]
            kl = nJ * Exx + nh * Ex - logZ + rn[0] * l[0] + rn[1] * l[1] - lse
            lin = (r[0] - rn[0]) * l[0] + (r[1] - rn[1]) * l[1]
            return rn, n, (A, h, cc, dd), (Exx, Ex), kl, lin

        hist, kl = mp.mpf(0), mp.mpf(0)
        close = lambda x, y: abs(x - y) <= mp.mpf("1e-40") * max(abs(y), 1)
        for t in range(3):
            r1, _, _, _, kl1, lin1 = one_pass(t, [f(v) for v in c["label_init"][t]])
            hist += kl1 + lin1
            r2, n2, (A, h, cc, dd), (Exx, Ex), kl2, _ = one_pass(t, r1)
            kl += kl2
            for k in range(2):
                assert close(out["label_fixed"][t, k], r1[k]) and close(out["label_stats"][t, k], r2[k])
                assert close(out["label_natparam"][t, k], n2[k])
            gn, gs = out["gaussian_natparam"][t], out["gaussian_stats"][t]
            assert close(gn[0, 0], A) and close(gn[0, 1], h) and close(gn[1, 1], cc) and close(gn[2, 2], dd)
            assert close(gs[0, 0], Exx) and close(gs[0, 1], Ex) and gs[1, 1] == 1 and gs[2, 2] == 1
            assert gn[1, 0] == 0 and gn[0, 2] == 0 and gs[1, 0] == 0
        assert close(out["kl_hist"][0], hist) and close(out["kl"], kl) and out["iters"] == 1
        assert out["kl_scale"] >= abs(out["kl"])


def test_sample_mp_is_the_mean_plus_the_whitened_noise():
    """x = J^-1 h + chol(J)^-T eps: J (x - mean) = L eps"""
    c = F.tail_case("plain", 3)
    x = gmm_mp.sample_mp(c["natparam"], c["eps"])
    N = 3
    for t in range(0, F.TAIL_T, 16):
        J = -2 * c["natparam"][t, :N, :N]
        L = np.linalg.cholesky(J)
        mean = np.linalg.solve(J, c["natparam"][t, :N, N])
        assert np.allclose(L.T @ (x[t] - mean).T, c["eps"][t].T, rtol=1e-12, atol=1e-12)


def test_tail_jvp_against_torch_autograd_and_its_own_step_size():
    """The difference's truncation is O(step^2) relative: steps 1e-20 and 1e-10 (at 60 digits) round to the same
    float64 here (measured difference 0; bound: 1e-18), so the oracle's result is the derivative rounded; torch fp64
    autograd of tests/_gmm_torch.py agrees with it to 7.5e-15 (bound: 1e-12, the rounding of the fp64 side alone)."""
    import torch
    N = 2
    c = F.tail_case("plain", N)
    args = (c["label_global"], c["gaussian_globals"], (c["node_J"], c["node_h"]), c["label_fixed"], c["eps"])
    d = c["dirs"][0]
    ds, dkl = gmm_mp.local_tail_jvp_mp(*args, direction=d, step=1e-20)
    ds2, dkl2 = gmm_mp.local_tail_jvp_mp(*args, direction=d, step=1e-10)
    trunc = max(np.max(np.abs(ds - ds2)) / np.max(np.abs(ds)), abs(dkl - dkl2) / abs(dkl))
    print("GMMTRUTH jvp step 1e-20 against 1e-10: %.3e" % trunc)
    assert trunc <= 1e-18
    nJ, nh = F._t64(c["node_J"]).requires_grad_(True), F._t64(c["node_h"]).requires_grad_(True)
    from torch.autograd.functional import jvp
    (x, kl), (tx, tkl) = jvp(lambda a, b: F.tail_torch(c, F.TAIL_S, a, b), (nJ, nh), (F._t64(d[0]), F._t64(d[1])))
    err = max(np.max(np.abs(tx.numpy() - ds)) / np.max(np.abs(ds)), abs(float(tkl) - dkl) / abs(dkl))
    print("GMMTRUTH jvp against torch autograd: %.3e" % err)
    assert err <= 1e-12


# --- every case of the GPU file, with the reference alone ------------------------------------------------------------

def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


@pytest.mark.parametrize("case", F.ACCURACY, ids=_ids(F.ACCURACY))
def test_accuracy_case_is_a_valid_comparison(case):
    family, N, K, T, m = case
    c, tr, ref, e_ref = F.truth(family, N, K, T, m)
    again = F.case(family, N, K, T)
    for k in ("label_global", "gaussian_globals", "node_J", "node_h", "label_init"):
        assert np.array_equal(c[k], again[k]), k                                 # deterministic
    assert np.all(np.isfinite(c["gaussian_globals"])) and np.all(c["node_J"] < 0)
    for k in range(c["gaussian_globals"].shape[0]):                              # every J is a positive combination of these
        assert np.all(np.linalg.eigvalsh(-2 * c["gaussian_globals"][k, :N, :N]) > 0)
    assert tr["iters"] == ref["iters"] == m
    for q, v in e_ref.items():
        assert np.isfinite(v) and v <= E_REF_MAX, (q, v)
    assert np.isfinite(tr["kl"]) and np.isfinite(ref["kl"]) and tr["kl_scale"] > 0
    want, held = F.expected_assign(tr, e_ref)
    assert np.mean(~held) <= 0.05
    assert np.array_equal(np.argmax(ref["label_stats"], -1)[held], want[held])   # the reference alone meets it
    if family == "far":
        assert np.any(tr["label_stats"] == 0.0)                                  # (responsibilities do underflow)
    if family == "tie":
        assert np.all(tr["label_stats"][:, 0] == tr["label_stats"][:, 1])


@pytest.mark.parametrize("case", F.OVERFLOW, ids=_ids(F.OVERFLOW))
def test_overflow_cases_leave_the_fp64_range_as_a_product_and_not_as_pivots(case):
    family, N, K, T, m = case
    tr = F.truth(family, N, K, T, m)[1]
    with np.errstate(over="ignore", under="ignore"):
        for t in range(T):
            d = np.linalg.eigvalsh(-2 * tr["gaussian_natparam"][t, :N, :N])
            assert np.all(d > 1e-60) and np.all(d < 1e60)
            assert not (np.isfinite(np.prod(d)) and np.prod(d) > np.finfo(float).tiny)


@pytest.mark.parametrize("case", F.STOPPING, ids=_ids(F.STOPPING))
def test_stopping_case_is_admissible(case):
    family, N, K, T, salt = case
    c, tr, ref, e_ref = F.truth(family, N, K, T, 100, F.TOL, salt)
    ok, margin, a = F.admissible(tr, ref)
    print("GMMTRUTH stopping %s: iters %d, min |d_i - tol| %.3e, restatement's KL error %.3e" % (case, tr["iters"], margin, a))
    assert ok and 1 < tr["iters"] == ref["iters"] < 100
    for q, v in e_ref.items():
        assert np.isfinite(v) and v <= E_REF_MAX, (q, v)


@pytest.mark.parametrize("case", F.TIE_STOP, ids=_ids(F.TIE_STOP))
def test_all_identical_components_stop_at_the_second_sweep(case):
    family, N, K, T, salt = case
    c, tr, ref, _ = F.truth(family, N, K, T, 100, F.TOL, salt)
    assert tr["iters"] == ref["iters"] == 2 and tr["kl_hist"][0] == tr["kl_hist"][1]


@pytest.mark.parametrize("family,N", sorted({(f, N) for f, N, _, _, _ in F.TAIL}))
def test_tail_case_is_a_valid_comparison(family, N):
    pytest.importorskip("torch")
    c = F.tail_case(family, N)
    again = F.tail_case.__wrapped__(family, N)
    for k in ("node_J", "node_h", "label_fixed", "natparam", "eps", "g_samples"):
        assert np.array_equal(c[k], again[k]), k
    for t in range(F.TAIL_T):
        assert np.all(np.linalg.eigvalsh(-2 * c["natparam"][t, :N, :N]) > 0)
    tt = F.tail_truth(family, N)
    e_s = F.e_block(tt["samples_ref"], tt["samples"])
    assert np.isfinite(e_s) and e_s <= E_REF_MAX
    for S in (1, 3):
        for mode in F.MODES:
            e_got, e_ref = F.grad_errors(family, N, S, mode, F.tail_want(family, N, S, mode))
            print("GMMTRUTH tail %s N=%d S=%d %s: e_ref %.3e" % (family, N, S, mode, e_ref))
            assert e_got == e_ref and np.isfinite(e_ref) and e_ref <= E_REF_MAX
