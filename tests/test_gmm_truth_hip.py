"""The GMM local-step kernels -- the mean-field fixed point on its four routes (csrc/gmm_meanfield.hip: single_wg,
persistent, sweeps; csrc/gmm_wide.hip: wide_sweeps), the per-point sampler and the derived adjoint (csrc/gmm_train.hip and
the wide pair) -- against a 50-digit evaluation of the same operation (oracle/gmm_mp.py), away from the one family
tests/test_gmm_hip.py and tests/test_gmm_wide_hip.py sit at.

The fixed point is not compared as a fixed point: the stopping rule |kl - kl_prev| < tol is a discontinuous function of
rounding.  With tol = 0.0 (accepted by the ABI, never true) the kernels run exactly max_iter sweeps and the final pass, a
smooth map of the inputs: all accuracy cases run that map.  The stopping DECISION is tested apart, on inputs shown clear
of the threshold by the oracle and the restatement alone (tests/test_gmm_mp_cpu.py asserts the condition, nothing is
skipped here).

The bound, per output array, is relative to the error e_ref of the fp64 host restatement oracle/gmm_numpy.py on the same
input and sweep count, both measured against the truth with the same normwise measure (tests/_gmm_families.py):

    e_kernel <= 16 max(e_ref, 64 eps)

Cases (tests/_gmm_families.py; workgroup boundaries read from the sources: 256 points per workgroup in the persistent and
per-sweep kernels, 1024 / 512 / 256 lanes in the one-workgroup kernel for N <= 3 / <= 5 / <= 8, 16 points per workgroup
and 4 per wavefront in the wide kernels; the responsibilities live in registers for K <= 8 and K <= 16 at N <= 4):

    family            N   K   T     sweeps     what the shape reaches
    plain             1   5   63    0, 1, 3    a partial wavefront; the final pass alone, one linear term, compounding
    plain             1   2   1025  1          one point over the one-workgroup kernel's 1024 lanes
    plain             2   5   257   1          a second workgroup of one point
    plain             2   8   64    3          K = 8 in registers, exactly one wavefront
    plain             2   9   65    1          K = 9 -> 16 registers, one lane over a wavefront
    plain             2   64  17    1          the largest K (responsibilities in memory)
    plain             3   16  255   1          K = 16 in registers, one workgroup less one point
    plain             3   17  256   0          K = 17 (in memory), exactly one workgroup
    plain             4   16  65    3          the largest register form
    plain             4   3   513   1          one point over the one-workgroup kernel's 512 lanes
    plain             5   5   64    1          N = 5: no register form
    plain             5   9   1     3          a single point
    plain             8   9   257   1          the largest N <= 8 kernel, two workgroups (one-workgroup kernel: 256 lanes)
    plain             8   3   1     3
    plain             9   5   15    3          wide: one workgroup less one point
    plain             12  17  16    1          wide: exactly one workgroup, K over one 16-lane row
    plain             16  5   17    0, 1, 3    wide: one point over a workgroup
    plain             16  64  5     1          wide: the largest N and K
    far, offset-1e4, tie, empty, K1, sharp-node, flat-node, aniso -- each at
                      2   5   65    0 and 3
                      4   16  33    1
                      8   5   17    3
                      16  9   17    1          (K1: K = 1 at every shape)
    scale-1e-3, scale-1e3 at N = 1, 2, 3, 4, 5, 8, 9, 12, 16 with K = 3, T = 17, 1 sweep
    scale-1e-21, scale-1e21 at N = 8 and scale-1e-11, scale-1e11 at N = 16 with K = 5, T = 17, 1 and 3 sweeps: the product
                      of the pivots leaves the fp64 range, every pivot is an ordinary number

Every case runs on each route that exists for its N: multi_wg=False (single_wg), the default (persistent),
multi_wg=True, persistent=False (sweeps) and wide=True (wide_sweeps) for N <= 8; wide_sweeps for N >= 9.

Sampler and adjoint: families plain, offset-1e4, aniso, sharp-node, scale-1e-3, scale-1e3 at N = 1, 4, 8, 9, 16, S = 1 and
3, T = 65, K = 5; samples against sample_mp with _gmm_torch.sample_torch on the CPU as e_ref; gradients through
<VJP(g), v> = <g, J v> with J v from local_tail_jvp_mp and torch-CPU autograd as e_ref (_gmm_families.grad_errors), the
cotangent on the KL alone, on the samples alone and on both.

Every figure is printed before it is asserted (`GMMTRUTH` lines, pytest -s): DESIGN.md section 4.6b is written from them.
Named exceptions (an output over the bound on an MI355X, pinned at 3 x its measured error, EXCEPTIONS below): none.  The
output closest to its bound is dirichlet_stats / niw_stats of offset-1e4 N=2 K=5 T=65 m=0 at 7.1 of the allowed 16; with
the factor at 1 instead of 16, 11 of the 88 accuracy cases fail (offset-1e4, aniso, K1's label natural parameter).

Before the fixes that came with this file: the eight scale-1e+-21 / 1e+-11 cases failed on `kl`
(inf, or off by 6 .. 11 % of its scale: the determinant was a plain product of the pivots) and on nothing else, and the
NaN and inf inputs of the status-word test came back with info == 0 on every route."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("mpmath")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmm_families as F  # noqa: E402

DEV = "cuda:0"
PER_POINT = ("label_stats", "label_fixed", "label_natparam", "gaussian_stats", "gaussian_natparam", "assign")
TOTALS = ("kl", "dirichlet_stats", "niw_stats")

# (case and route as printed, output) -> the bound that replaces 16 max(e_ref, 64 eps): 3 x the error measured on an MI355X
EXCEPTIONS = {}


def _d(x):
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device=DEV)


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _run(c, kw, tol, max_iter):
    from svae_amd.models import gmm
    return gmm.meanfield_from_globals(_d(c["label_global"]), _d(c["gaussian_globals"]), (_d(c["node_J"]), _d(c["node_h"])),
                                      _d(c["label_init"]), tol=tol, max_iter=max_iter, check=False, **kw)


def _host(out):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _judge(case_name, c, tr, e_ref, tol, max_iter, want_iters):
    """run the case on every route of its N; -> failures as text lines"""
    N = c["node_h"].shape[1]
    bad, outs = [], {}
    want, held = F.expected_assign(tr, e_ref)
    for route, (kw, path) in F.routes(N).items():
        out = _host(_run(c, kw, tol, max_iter))
        outs[route] = out
        what = "%s %s" % (case_name, route)
        assert out["path"] == path, (what, out["path"])
        bad += F.check(F.errors(out, tr), e_ref, what, EXCEPTIONS)
        if int(out["info"][0]) != 0:
            bad.append("%s: info %d on valid input" % (what, int(out["info"][0])))
        if int(out["iters"][0]) != want_iters:
            bad.append("%s: iters %d, the oracle's %d" % (what, int(out["iters"][0]), want_iters))
        wrong = np.flatnonzero((out["assign"] != want) & held)
        if len(wrong):
            bad.append("%s: assign differs from the oracle's argmax at points %s" % (what, wrong[:8]))
    if N <= 8:
        for k in PER_POINT:
            for route in ("persistent", "sweeps"):
                if not np.array_equal(outs["single_wg"][k], outs[route][k]):
                    bad.append("%s: %s differs in bits between single_wg and %s" % (case_name, k, route))
        for k in TOTALS:
            if not np.array_equal(outs["persistent"][k], outs["sweeps"][k]):
                bad.append("%s: %s differs in bits between persistent and sweeps" % (case_name, k))
    return bad


# --- accuracy of the smooth map: tol = 0, exactly m sweeps + the final pass --------------------------------------------

@pytest.mark.parametrize("case", F.ACCURACY, ids=_ids(F.ACCURACY))
def test_meanfield_against_the_50_digit_oracle(case):
    family, N, K, T, m = case
    c, tr, _, e_ref = F.truth(family, N, K, T, m)
    bad = _judge("%s N=%d K=%d T=%d m=%d" % case, c, tr, e_ref, 0.0, m, m)
    assert not bad, "\n".join(bad)


# --- the stopping decision, on inputs clear of the threshold ----------------------------------------------------------

@pytest.mark.parametrize("case", F.STOPPING, ids=_ids(F.STOPPING))
def test_stopping_decision_on_admissible_inputs(case):
    """tol = 1e-3, max_iter = 100: every |d_i - tol| of the oracle's KL history exceeds 1e3 x the restatement's absolute KL
    error (asserted on the CPU), so the sweep count is the oracle's; then the accuracy rule at that sweep count"""
    family, N, K, T, salt = case
    c, tr, ref, e_ref = F.truth(family, N, K, T, 100, F.TOL, salt)
    assert F.admissible(tr, ref)[0]
    bad = _judge("stop %s N=%d K=%d T=%d salt=%d" % case, c, tr, e_ref, F.TOL, 100, tr["iters"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", F.TIE_STOP, ids=_ids(F.TIE_STOP))
def test_identical_components_repeat_the_kl_bits_and_stop_at_the_second_sweep(case):
    family, N, K, T, salt = case
    c, tr, ref, e_ref = F.truth(family, N, K, T, 100, F.TOL, salt)
    assert tr["iters"] == 2
    bad = _judge("stop %s N=%d K=%d T=%d salt=%d" % case, c, tr, e_ref, F.TOL, 100, 2)
    assert not bad, "\n".join(bad)


# --- the status word --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,T", [(2, 5, 257), (4, 9, 65), (8, 17, 17), (9, 5, 17), (16, 5, 33)])
def test_status_word_reports_indefinite_and_non_finite_points_and_stays_zero_otherwise(N, K, T):
    """an indefinite factor: info = the LOWEST such point + 1; a NaN node potential passes every pivot test (it is in h, not
    in J) and used to come back as info == 0 with responsibilities of 0 (the exp's clamp): now the point's non-finite KL
    term raises the word too.  Every route; sweeps 0 (the final pass alone) and 2."""
    c = F.case("plain", N, K, T)
    lo, hi = T // 4, T - 1                                     # (T = 257: in different workgroups)
    for route, (kw, path) in F.routes(N).items():
        for m in (0, 2):
            clean = _run(c, kw, 0.0, m)
            assert clean["path"] == path and int(clean["info"].item()) == 0, (route, m)
            bent = dict(c, node_J=c["node_J"].copy())
            bent["node_J"][hi, 0] = -100.0 * bent["node_J"][hi, 0]             # precision < 0: the first pivot is <= 0
            bent["node_J"][lo, N - 1] = -100.0 * bent["node_J"][lo, N - 1]     # ... the last pivot
            assert int(_run(bent, kw, 0.0, m)["info"].item()) == lo + 1, (route, m)
            nan = dict(c, node_h=c["node_h"].copy())
            nan["node_h"][hi, N - 1] = np.nan
            out = _run(nan, kw, 0.0, m)
            assert int(out["info"].item()) > 0, (route, m)
            inf = dict(c, node_h=c["node_h"].copy())
            inf["node_h"][lo, 0] = np.inf
            assert int(_run(inf, kw, 0.0, m)["info"].item()) > 0, (route, m)


# --- sampler and adjoint ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", F.TAIL, ids=_ids(F.TAIL))
def test_sampler_against_the_50_digit_oracle(case):
    from svae_amd.models import gmm
    family, N, _, _, S = case
    c, tt = F.tail_case(family, N), F.tail_truth(family, N)
    got = gmm.gaussian_sample(_d(c["natparam"]), _d(c["eps"][:, :S])).cpu().numpy()
    what = "sample %s N=%d S=%d" % (family, N, S)
    bad = F.check({"samples": F.e_block(got, tt["samples"][:, :S])},
                  {"samples": F.e_block(tt["samples_ref"][:, :S], tt["samples"][:, :S])}, what, EXCEPTIONS)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("case", F.TAIL, ids=_ids(F.TAIL))
def test_local_adjoint_against_the_50_digit_oracle(case, mode):
    """gmm._LocalTail (svae_gmm_local_vjp_f64 / svae_gmm_wide_local_vjp_f64) on the final pass from the case's
    responsibilities: <VJP(g), v> against <g, J v> of the oracle along the two coordinates where kernel and torch-CPU
    autograd disagree most, the largest coordinate and two random directions"""
    from svae_amd.models import gmm
    family, N, K, T, S = case
    c = F.tail_case(family, N)
    lg, gg = _d(c["label_global"]), _d(c["gaussian_globals"])
    nJ, nh = _d(c["node_J"]).requires_grad_(True), _d(c["node_h"]).requires_grad_(True)
    o = gmm.meanfield_from_globals(lg, gg, (nJ.detach(), nh.detach()), _d(c["label_fixed"]), tol=0.0, max_iter=0, check=False)
    assert int(o["info"].item()) == 0 and torch.equal(o["label_fixed"], _d(c["label_fixed"]))
    x, kl = gmm._LocalTail.apply(nJ, nh, _d(c["eps"][:, :S]), lg, gg, o)
    gs, gk = F.cotangent(c, S, mode)
    gJ, gh = torch.autograd.grad([x, kl], [nJ, nh], [_d(gs), torch.tensor(gk, dtype=torch.float64, device=DEV)])
    e_got, e_ref = F.grad_errors(family, N, S, mode, (gJ.cpu().numpy(), gh.cpu().numpy()))
    what = "adjoint %s N=%d S=%d %s" % (family, N, S, mode)
    bad = F.check({"grad": e_got}, {"grad": e_ref}, what, EXCEPTIONS)
    assert not bad, "\n".join(bad)
