"""The MFMA LDS paths against the TRUTH: the tile kernels (lds_estep_tile.hip, lds_chol_tile.hip, lds_vjp_tile.hip,
n = 16 .. 64) and the XL kernel (lds_estep_xl.hip, n = 65 .. 128) on the precomputed 50-digit fixtures
tests/golden/lds_mfma_truth_*.npz (tests/golden/make_golden_lds_mfma_truth.py; draws, hash check and judge in
tests/_lds_mfma_truth.py).

Metric and rule are tests/test_lds_truth_hip.py's: normwise distance per output array, and
    HIP-vs-truth <= max(3 x comparator-vs-truth, 1e-11).
The comparator is the reference's compiled function of the same name on the same input (oracle.ref.estep,
ref.estep_vjp, ref.sample_backward).  The reference's sampler draws numpy.random.randn(T, S, n) itself when called
(cython_lds_inference.pyx:333) and applies it flipped in time: `_fixed_noise` hands it the fixture's eps through that
call (as tests/test_lds_truth_hip.py's host_entry_case does with zeros) -- so the comparator of the samples and of the
sampler's VJP is the reference's own compiled sampler, not the fp64 restatement.  That the compiled code took the noise
shows in the comparator's own distance to the mp samples and gradients, which every case holds below 1e-6
(COMPARATOR_SANITY: a sampler on other noise is O(1) off).  The reference runs on one BLAS thread.

Sizes: n = 17, 32 (NB = 2), 33, 48 (NB = 3), 63, 64 (NB = 4) at T = 4; n = 65, 96, 97, 128 (NB = 5 .. 8) at T = 3; an
ill draw (the worst cond(J22) of seeds 0 .. 99 on which fp64 still resolves 1e-9) and a median draw each, homogeneous
pair parameters everywhere, per-step ones at n = 33, 64, 65, 128; plus n128_perstep_s90, the seed of median cond(J22) at
n = 128 per-step, which is no median draw (ill-conditioned init block: the floor does not bind, tests/_lds_mfma_truth.py)
and on which the XL kernel misses the rule, and n64_perstep_illinit, the tile path's counterpart (largest cond(J0) of
the seeds).  Every case prints its distances (MFMATRUTH lines:
array HIP-vs-truth|comparator-vs-truth); DESIGN section 2 has the table measured on MI355X.

Open gaps (GAPS): an array that misses the rule but stays within max(30 x comparator-vs-truth, 1e-10) -- one decimal
digit more than the reference loses -- is listed per array with its measured distance and held to THAT bound.
Beyond that bound (BEYOND) nothing is pinned: the array is a strict expected failure with its cause and distance."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import _lds_mfma_truth as M
from oracle import ref
from test_lds_truth_hip import _dev_model, _dist, _distances, _np, _stats_arrays

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]

COMPARATOR_SANITY = 1e-6
TILE = [f[0] for f in M.fixture_names("tile")]
XL = [f[0] for f in M.fixture_names("xl")]
TWO_PER_CU = ["n17_homog_ill", "n33_perstep_ill", "n64_homog_ill", "n64_perstep_ill"]
XL_BATCHED = ["n65_homog_ill", "n65_perstep_ill", "n128_homog_ill", "n128_perstep_ill"]
VJP = [f[0] for f in M.fixture_names("tile") if f[4] == "homog" or f[2] in (33, 64)]
VJP_NO_SAMPLER = ["n33_homog_ill", "n33_perstep_ill", "n64_homog_ill", "n64_perstep_ill"]

# (test, fixture) -> {array: HIP-vs-truth measured on MI355X}: arrays held to max(30 x comparator, 1e-10) (module docstring)
GAPS = {
    # comparator 1.1e-10, 1.3e-10, 3.0e-10, 3.2e-10, 2.3e-10
    ("tile_estep", "n32_homog_ill"): {"ExxT0": 2.5e-09, "Ex0": 1.8e-09, "Epair_xx": 9.2e-10, "Epair_xxn": 1.2e-09,
        "Enode_x": 1.1e-09},
    # comparator 4.7e-12, 8.6e-12, 4.6e-12
    ("tile_estep", "n33_homog_ill"): {"Epair_xx": 1.7e-11, "Epair_xxn": 2.8e-11, "Epair_xnxn": 1.6e-11},
    # comparator 6.4e-12
    ("tile_estep", "n33_perstep_ill"): {"Ex0": 2.4e-11},
    # comparator 4.5e-12, 8.8e-11, 9.5e-11, 8.9e-11, 1.2e-10, 1.1e-10
    ("tile_estep", "n63_homog_ill"): {"lognorm": 1.6e-11, "ExxT0": 1.1e-09, "Ex0": 1.1e-09, "Epair_xx": 2.8e-10,
        "Epair_xxn": 6.2e-10, "Enode_x": 5.5e-10},
    # comparator 6.4e-12
    ("tile_estep_2wg", "n33_perstep_ill"): {"Ex0": 2.4e-11},
    # comparator 8.9e-12, 9.6e-12, 9.2e-12
    ("xl_estep", "n96_homog_ill"): {"Epair_xx": 3.4e-11, "Epair_xnxn": 3.4e-11, "Enode_diagxx": 3.4e-11},
    # comparator 1.1e-10, 1.3e-10, 3.0e-10, 3.2e-10, 2.3e-10
    ("tile_sampler", "n32_homog_ill"): {"ExxT0": 2.5e-09, "Ex0": 1.8e-09, "Epair_xx": 9.2e-10, "Epair_xxn": 1.2e-09,
        "Enode_x": 1.1e-09},
    # comparator 4.7e-12, 8.6e-12, 4.6e-12
    ("tile_sampler", "n33_homog_ill"): {"Epair_xx": 1.7e-11, "Epair_xxn": 2.8e-11, "Epair_xnxn": 1.6e-11},
    # comparator 6.4e-12
    ("tile_sampler", "n33_perstep_ill"): {"Ex0": 2.4e-11},
    # comparator 5.9e-12
    ("tile_sampler", "n48_homog_ill"): {"samples": 2.4e-11},
    # comparator 4.5e-12, 8.8e-11, 9.5e-11, 8.9e-11, 1.2e-10, 1.1e-10
    ("tile_sampler", "n63_homog_ill"): {"lognorm": 1.6e-11, "ExxT0": 1.1e-09, "Ex0": 1.1e-09, "Epair_xx": 2.8e-10,
        "Epair_xxn": 6.2e-10, "Enode_x": 5.5e-10},
    # comparator 5.7e-11
    ("tile_sampler", "n64_homog_ill"): {"samples": 2.4e-10},
    # comparator 2.3e-10, 3.0e-10
    ("tile_vjp", "n32_homog_ill"): {"Enode_x": 1.1e-09, "grad_h": 1.3e-09},
    # comparator 2.8e-12
    ("tile_vjp", "n33_homog_ill"): {"grad_J": 2.0e-11},
    # comparator 5.9e-12
    ("tile_vjp", "n48_homog_ill"): {"samples": 2.4e-11},
    # comparator 4.5e-12, 1.1e-10
    ("tile_vjp", "n63_homog_ill"): {"lognorm": 1.6e-11, "Enode_x": 5.5e-10},
    # comparator 5.7e-11
    ("tile_vjp", "n64_homog_ill"): {"samples": 2.4e-10},
    # comparator 2.6e-12
    ("tile_vjp_nosampler", "n33_homog_ill"): {"grad_J": 2.3e-11},
    # comparator 5.1e-11
    ("tile_vjp_nosampler", "n33_perstep_ill"): {"grad_h": 1.7e-10},
    # comparator 5.4e-11
    ("tile_vjp", "n33_perstep_ill"): {"grad_h": 1.9e-10},
    # the ill-conditioned init block (_INIT_CAUSE): comparator 2.7e-11, 1.7e-11, 2.7e-11, 1.7e-11, 2.7e-11, 1.7e-11[, 1.8e-11]
    ("tile_estep", "n64_perstep_illinit"): {"ExxT0": 5.1e-10, "Ex0": 3.6e-10, "Epair_xx": 5.1e-10, "Epair_xxn": 4.3e-10,
                                            "Enode_diagxx": 5.1e-10, "Enode_x": 3.6e-10},
    ("tile_sampler", "n64_perstep_illinit"): {"ExxT0": 5.1e-10, "Ex0": 3.6e-10, "Epair_xx": 5.1e-10, "Epair_xxn": 4.3e-10,
                                              "Enode_diagxx": 5.1e-10, "Enode_x": 3.6e-10, "samples": 3.0e-10},
    # comparator 2.7e-11, 1.7e-11, 1.8e-11, 1.1e-11, 3.9e-11
    ("tile_vjp", "n64_perstep_illinit"): {"Enode_diagxx": 5.1e-10, "Enode_x": 3.6e-10, "samples": 3.0e-10,
                                          "grad_h": 2.6e-10, "grad_J": 2.0e-10},
}

# Arrays beyond max(30 x comparator, 1e-10): nothing is pinned there.  (test, fixture) -> ({array: measured}, cause); the
# case is an expected failure for THESE arrays only (_report judges the others first) and fails again once one of them
# comes within the open-gap bound.
_NOISE_CAUSE = ("lds_chol_tile.hip takes the noise factor chol(P_t)^-T as the UL Cholesky factor of the hand-off's COMPUTED "
                "P_t^-1, not from P_t: the rounding of the inverse (cond(P_t) eps) is amplified once more in its small "
                "directions, where the reference factors P_t and solves (cond(P_t) 1.5e7 at n64_perstep_ill, 3.6e6 at n63)")
_XL_CAUSE = ("lds_estep_xl.hip forms c_t = P_t^-1 h_t as a dot product with the EXPLICIT inverse its block Gauss-Jordan (16 x 16 "
             "LDL' pivots, unpivoted) leaves in registers.  That inverse is within 7e-12 of the truth (normwise: cond(P_0) eps, "
             "cond(P_0) = 3.6e6), but on this draw h_0 = 1.4e5 cancels to |c_0| = 5.6 (cond(J0) 3.2e8; |P^-1||h|/|c| = 1.3e5, "
             "<= 1e3 on every other fixture), so the inverse's error comes through multiplied by 1.3e5.  The kernel's blocked "
             "order replayed in fp64 on the CPU gives c_0 at 1.8e-7 and the whole E-step at 1e-7 .. 2.5e-7 (lognorm 3e-10); the "
             "true inverse rounded to fp64 times h_0 gives 1.1e-11 (so not the dot product), and h_0 carried through the SAME "
             "elimination as one more right-hand-side column, as the tile path's [P | R | c] panel does, gives 8.7e-12: that "
             "is the fix, one more column in the register panel of the forward sweep (DESIGN section 2)")
_INIT_CAUSE = ("the tile kernel too forms c_t = P_t^-1 h_t with the finished explicit inverse (lds_estep_tile.hip, the hand-off "
               "copy) and the quadratic term of lognorm as h_t . c_t: on this draw (cond(J0) 8.7e7, h_0 = 1.2e5 against |c_0| = "
               "7.9, |P^-1||h|/|c| = 9.5e4, cond(P_0) 2.1e6) c_0 is 3.6e-10 off -- 20x the reference, within the open-gap "
               "bound -- and h_0 . c_0 multiplies that by |h_0| again, where the reference takes |L^-1 h|^2 from the Cholesky "
               "factor; the error of c_0 then (supposed, not localised) travels forward through h_1 = node_h + J12' c_0 into the later steps (E_pair "
               "x'x' at 4.8e-10, the reference at 4e-12 there).  Same fix as _XL_CAUSE: h as a column of the elimination")
BEYOND = {
    ("tile_estep", "n64_perstep_illinit"): ({"lognorm": 1.5e-08, "Epair_xnxn": 4.8e-10}, _INIT_CAUSE),   # comparator 1.5e-12, 4.1e-12
    ("tile_sampler", "n64_perstep_illinit"): ({"lognorm": 1.5e-08, "Epair_xnxn": 4.8e-10}, _INIT_CAUSE),
    ("tile_vjp", "n64_perstep_illinit"): ({"lognorm": 1.5e-08}, _INIT_CAUSE),
    ("tile_sampler", "n63_homog_ill"): ({"samples": 4.8e-09}, _NOISE_CAUSE),            # comparator 1.3e-10
    ("tile_sampler", "n64_perstep_ill"): ({"samples": 9.6e-08}, _NOISE_CAUSE),          # comparator 4.8e-10
    ("tile_vjp", "n63_homog_ill"): ({"samples": 4.8e-09}, _NOISE_CAUSE),
    ("tile_vjp", "n64_perstep_ill"): ({"samples": 9.6e-08}, _NOISE_CAUSE),
    # comparator 2.4e-14, 3.8e-11, 3.2e-11, 3.0e-11, 1.9e-11, 2.0e-12, 1.4e-11, 1.9e-11
    ("xl_estep", "n128_perstep_s90"): ({"lognorm": 1.8e-09, "ExxT0": 1.3e-07, "Ex0": 1.4e-07, "Epair_xx": 1.0e-07,
                                           "Epair_xxn": 8.0e-08, "Epair_xnxn": 6.2e-09, "Enode_diagxx": 3.6e-08,
                                           "Enode_x": 8.0e-08}, _XL_CAUSE),
}


@functools.lru_cache(maxsize=None)
def _fx(name):
    return M.load(name)


@contextlib.contextmanager
def _fixed_noise(eps):
    """numpy.random.randn returns the fixture's noise as the compiled sampler indexes it (flipud: eps[T-1] first)"""
    randn = np.random.randn

    def fixed(*shape):
        assert tuple(shape) == eps.shape, (shape, eps.shape)
        return eps[::-1].copy()
    np.random.randn = fixed
    try:
        yield
    finally:
        np.random.randn = randn


@functools.lru_cache(maxsize=None)
def _ref_estep(name):
    fx = _fx(name)
    with M.threadpool_limits(limits=1):          # (the comparator's last digits move with the number of BLAS threads)
        return _distances(_stats_arrays(*ref.estep(fx["natparam"], fx["node"])), M.truth_arrays(fx))


@functools.lru_cache(maxsize=None)
def _ref_samples(name):
    fx = _fx(name)
    with _fixed_noise(fx["eps"]), M.threadpool_limits(limits=1):
        samples, _ = ref.sample_backward(fx["natparam"], fx["node"], M.NUM_SAMPLES, 0)
    return _dist(samples, fx["samples"])


def _device(fx, B=1):
    return _dev_model(fx["natparam"][0], fx["natparam"][1], tuple(x[None] for x in fx["node"]), B)


def _report(test, name, hip, want, where=""):
    print("MFMATRUTH %s%s %s cond %.1e: " % (test, where, name, _fx(name)["cond"])
          + ", ".join("%s %.2e|%.2e" % (k, hip[k], want[k]) for k in hip))
    # the comparator itself is sane: every fixture keeps fp64 within 1e-9 of the truth on the statistics, so a comparator
    # beyond 1e-6 is broken (a reference sampler that did not take the fixture's noise is O(1) off) and would pass anything
    assert all(v <= COMPARATOR_SANITY for v in want.values()), ("comparator off", test, name, want)
    beyond, cause = BEYOND.get((test, name), ({}, None))
    M.judge({k: v for k, v in hip.items() if k not in beyond}, want, (test, name), GAPS.get((test, name), ()))
    if beyond:              # a strict expected failure per ARRAY: every other array of the case has been judged above
        for k in beyond:
            assert hip[k] > max(M.GAP_FACTOR * want[k], M.GAP_FLOOR), \
                ("now within the open-gap bound: take it out of BEYOND", test, name, k, hip[k], want[k])
        pytest.xfail("%s: %s" % (", ".join("%s %.1e against %.1e" % (k, hip[k], want[k]) for k in beyond), cause))


def _estep(name, B=1):
    from svae_amd.lds.lds_inference import natural_lds_estep_general
    nat, nodes = _device(_fx(name), B)
    with torch.no_grad():
        return _stats_arrays(*natural_lds_estep_general(nat, nodes, check=True))


def _batched_case(test, name):
    """the draw replicated to CU count + 37 sequences: every sequence the same bits, three of them judged"""
    B = torch.cuda.get_device_properties(0).multi_processor_count + 37
    got = _estep(name, B)
    for k, a in got.items():
        assert a.shape[0] == B and torch.equal(a, a[:1].expand_as(a)), (name, k)
    truth = M.truth_arrays(_fx(name))
    for b in sorted({0, (2 * B) // 3, B - 1}):
        _report(test, name, _distances({k: a[b] for k, a in got.items()}, truth), _ref_estep(name), "[b=%d of %d]" % (b, B))


@pytest.mark.parametrize("name", TILE)
def test_tile_estep_against_truth(name):
    """all eight output arrays at B = 1: the one-workgroup-per-CU instances launch_tile<NB>, NB = 2, 3, 4"""
    _report("tile_estep", name, _distances(_estep(name), M.truth_arrays(_fx(name))), _ref_estep(name))


@pytest.mark.parametrize("name", TWO_PER_CU)
def test_tile_estep_two_workgroups_per_cu_against_truth(name):
    """B = CU count + 37: the forward-half and backward-half launches of the <NB, INHOMOG, 2, 1> / <.., 2, 2> instances"""
    _batched_case("tile_estep_2wg", name)


@pytest.mark.parametrize("name", XL)
def test_xl_estep_against_truth(name):
    """all eight output arrays at B = 1: lds_estep_xl.hip, NB = 5 .. 8"""
    _report("xl_estep", name, _distances(_estep(name), M.truth_arrays(_fx(name))), _ref_estep(name))


@pytest.mark.parametrize("name", XL_BATCHED)
def test_xl_estep_batched_against_truth(name):
    _batched_case("xl_estep_batched", name)


@pytest.mark.parametrize("name", TILE)
def test_tile_sampler_real_noise_against_truth(name):
    """S = 2 samples on the fixture's non-zero noise: the noise factor chol(P_t)^-T eps_t of lds_chol_tile.hip"""
    from svae_amd.lds.lds_inference import natural_lds_inference_general
    fx = _fx(name)
    nat, nodes = _device(fx)
    eps = torch.as_tensor(fx["eps"][None], dtype=torch.float64, device="cuda")
    with torch.no_grad():
        samples, stats, lognorm = natural_lds_inference_general(nat, nodes, num_samples=M.NUM_SAMPLES, eps=eps)
    assert tuple(samples.shape) == (1,) + fx["samples"].shape
    hip = _distances(_stats_arrays(lognorm, stats), M.truth_arrays(fx))
    hip["samples"] = _dist(samples, fx["samples"])
    _report("tile_sampler", name, hip, dict(_ref_estep(name), samples=_ref_samples(name)))


def _vjp_case(name, sampler):
    """forward values, node-h gradient (closed form) and node-J gradient (<VJP(g), v> = <g, J v> along the fixture's
    directions) of lds_inference_differentiable under the fixture's cotangents -> HIP-vs-truth, reference-vs-truth"""
    from svae_amd.lds.lds_inference import lds_inference_differentiable
    fx = _fx(name)
    g_l, g_d, g_x, g_s = float(fx["g_l"]), fx["g_d"], fx["g_x"], fx["g_s"]
    nat, _ = _device(fx)
    cu = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda")
    nJ, nh, nz = (cu(x[None]).requires_grad_(True) for x in fx["node"])
    ln, (dxx, x), smp, _ = lds_inference_differentiable(nat, (nJ, nh, nz), eps=cu(fx["eps"][None]) if sampler else None)
    loss = (ln * g_l).sum() + (dxx * cu(g_d)[None]).sum() + (x * cu(g_x)[None]).sum()
    if sampler:
        loss = loss + (smp * cu(g_s)[None]).sum()
    loss.backward()
    zero_pair = (np.zeros_like(fx["natparam"][1][0]),) * 3          # (n,n), or (T-1,n,n) with per-step pair parameters
    with _fixed_noise(fx["eps"]), M.threadpool_limits(limits=1):
        (wJ, wh, _), _ = ref.estep_vjp(fx["natparam"], fx["node"], g_l, (g_d, g_x), g_samples=g_s if sampler else None,
                                          g_E_pair=zero_pair)
    keys = ("lognorm", "Enode_diagxx", "Enode_x")
    truth = M.truth_arrays(fx)
    hip = _distances({"lognorm": ln, "Enode_diagxx": dxx, "Enode_x": x}, {k: truth[k] for k in keys})
    want = {k: _ref_estep(name)[k] for k in keys}
    tJ = fx["jvp_estep"] + (fx["jvp_sampler"] if sampler else 0.0)
    th = fx["grad_h"] if sampler else fx["grad_h_nosampler"]
    scale = float(fx["scale_J"] if sampler else fx["scale_J_nosampler"])
    if sampler:
        hip["samples"], want["samples"] = _dist(smp, fx["samples"]), _ref_samples(name)
    hip["grad_h"], want["grad_h"] = _dist(nh.grad, th), _dist(wh, th)
    hip["grad_J"] = M.direction_distance(_np(nJ.grad[0]), fx["dirs"], tJ, scale)
    want["grad_J"] = M.direction_distance(wJ, fx["dirs"], tJ, scale)
    return hip, want


@pytest.mark.parametrize("name", VJP)
def test_tile_training_forward_and_vjp_against_truth(name):
    """with the sampler on the fixture's noise: the three VJP phases of lds_vjp_tile.hip and the noise factor's adjoint"""
    _report("tile_vjp", name, *_vjp_case(name, True))


@pytest.mark.parametrize("name", VJP_NO_SAMPLER)
def test_tile_training_vjp_without_sampler_against_truth(name):
    _report("tile_vjp_nosampler", name, *_vjp_case(name, False))
