"""GPU tests of the training path of the ragged SLDS (svae_amd/models/slds_svae.py: run_inference_ragged_differentiable,
run_inference_withlabels_ragged_differentiable).  Forward values: those of run_inference(lengths=) /
run_inference_withlabels(lengths=) on the same noise, with the bounds of tests/test_slds_ragged_hip.py (1e-6 in that file's
measure, the bounds to rel 1e-7).  Gradients: with the mean-field parameters of the ragged ascent frozen, the existing uniform
final pass (final_pass_differentiable / run_inference_withlabels_differentiable, pinned to the reference by
tests/test_slds_hip.py) on every sequence cut to [:L] with B = 1, T = L; the gradient of local_vlb + <random, samples> w.r.t.
nn_potentials agrees on [:L] at 1e-6 in the metric of tests/test_lds_ragged_hip.py and is exactly 0 beyond L; NaN in the
padding of the potentials and of both noise arrays changes nothing."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _slds_ragged_numpy as sr  # noqa: E402

SHAPES = [(3, 4, 12, 5), (8, 10, 17, 5)]          # (K, n, T, B)


def _np(x):
    return x.detach().cpu().numpy()


def _rel(a, b):
    a = _np(a) if hasattr(a, "detach") else np.asarray(a, float)
    b = _np(b) if hasattr(b, "detach") else np.asarray(b, float)
    if not b.size:
        return 0.0
    scale = np.maximum(np.abs(b), 1e-3 * max(np.max(np.abs(b)), 1e-300))
    return float(np.max(np.abs(a - b) / scale))


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


@functools.lru_cache(maxsize=None)
def _case(K, n, T, B):
    c = sr.slds_case(K, n, T, B, 1000 * K + 10 * n + T)
    rng = np.random.default_rng(K + n + T)
    c["r"] = rng.standard_normal((B, T, c["S"], n))                # the random functional of the samples
    c["prior"] = sr.slds_globals(K, n, np.random.default_rng(1))
    return c


def _padded(x, c, nan_pad, L=None):
    x = x.copy()
    if nan_pad:
        for b, l in enumerate(c["L"] if L is None else L):
            x[b, max(int(l), 2):] = np.nan
    return _t(x)


def _cut_reference(c, L=None):
    """the frozen mean field of the ragged ascent, then the uniform final pass on every cut sequence -> per-sequence
    (g_J, g_h) of local_vlb + <r, samples> (computed per call: device state, not cached across tests)"""
    from svae_amd.models import slds_svae
    L = c["L"] if L is None else L
    dev = "cuda:0"
    node = (_t(c["J"]), _t(c["h"]))
    maps = slds_svae.global_to_local_maps(c["glob"], torch.device(dev))
    (hmm_stats, _), (hmm_nat, (lds_init, lds_pair)), _, _ = slds_svae.optimize_local_meanfield(
        c["glob"], node, _t(c["init_eps"]), pair_stats=False, local_maps=maps, lengths=L)
    out = []
    for b in range(c["B"]):
        l = min(max(int(L[b]), 2), c["T"])
        nJ = node[0][b:b + 1, :l].clone().requires_grad_(True)
        nh = node[1][b:b + 1, :l].clone().requires_grad_(True)
        cut_nat = (tuple(x[b:b + 1].contiguous() for x in lds_init), tuple(x[b:b + 1, :l - 1].contiguous() for x in lds_pair))
        samples, _, local_vlb = slds_svae.final_pass_differentiable(
            c["glob"], hmm_nat, cut_nat, (nJ, nh), _t(c["eps"][b:b + 1, :l]), True, maps)
        (local_vlb + (_t(c["r"][b:b + 1, :l]) * samples).sum()).backward()
        out.append((_np(nJ.grad[0]), _np(nh.grad[0])))
    return out


def _ragged_grads(c, nan_pad, L=None):
    from svae_amd.models import slds_svae
    L = c["L"] if L is None else L
    nJ = _padded(c["J"], c, nan_pad, L).requires_grad_(True)
    nh = _padded(c["h"], c, nan_pad, L).requires_grad_(True)
    samples, stats, global_vlb, local_vlb = slds_svae.run_inference_ragged_differentiable(
        c["prior"], c["glob"], (nJ, nh), L, c["S"], init_eps=_padded(c["init_eps"], c, nan_pad, L),
        eps=_padded(c["eps"], c, nan_pad, L))
    live = torch.arange(c["T"], device="cuda:0")[None, :] < torch.as_tensor(np.maximum(L, 2), device="cuda:0")[:, None]
    r = torch.where(live[..., None, None], _t(c["r"]), torch.zeros((), dtype=torch.float64, device="cuda:0"))
    (local_vlb + (r * samples).sum()).backward()
    return dict(samples=samples.detach(), stats=stats, global_vlb=global_vlb.detach(), local_vlb=local_vlb.detach(),
                gJ=nJ.grad.clone(), gh=nh.grad.clone())


def _check_grads(got, want, c, rows=None, L=None):
    L = c["L"] if L is None else L
    worst = {"g_J": 0.0, "g_h": 0.0}
    for b in (range(c["B"]) if rows is None else rows):
        l = int(L[b])
        worst["g_J"] = max(worst["g_J"], _rel(got["gJ"][b, :l], want[b][0]))
        worst["g_h"] = max(worst["g_h"], _rel(got["gh"][b, :l], want[b][1]))
        assert bool((got["gJ"][b, l:] == 0).all()) and bool((got["gh"][b, l:] == 0).all()), b
        assert bool(torch.isfinite(got["gJ"][b]).all()) and bool(torch.isfinite(got["gh"][b]).all()), b
    print("worst relative errors:", {k: "%.2e" % v for k, v in worst.items()})
    assert worst["g_J"] < 1e-6 and worst["g_h"] < 1e-6, worst


def _flat(stats):
    (Ei, Et), (g_init, g_pair) = stats
    return [Ei, Et] + list(g_init) + list(g_pair)


@pytest.mark.parametrize("K,n,T,B", SHAPES)
def test_forward_values_are_those_of_run_inference_with_lengths(K, n, T, B):
    from svae_amd.models import slds_svae
    c = _case(K, n, T, B)
    got = _ragged_grads(c, True)
    samples, stats, global_vlb, local_vlb = slds_svae.run_inference(
        c["prior"], c["glob"], (_padded(c["J"], c, True), _padded(c["h"], c, True)), c["S"],
        init_eps=_padded(c["init_eps"], c, True), eps=_padded(c["eps"], c, True), lengths=c["L"])
    slds_svae.check_info()
    assert _rel(got["samples"], samples) < 1e-6
    for b, l in enumerate(c["L"]):
        assert bool((got["samples"][b, l:] == 0).all())
    for a, w in zip(_flat(got["stats"]), _flat(stats)):
        assert _rel(a, w) < 1e-6
    assert float(got["local_vlb"]) == pytest.approx(float(local_vlb), rel=1e-7)
    assert float(got["global_vlb"]) == pytest.approx(float(global_vlb), rel=1e-7)


@pytest.mark.parametrize("K,n,T,B", SHAPES)
def test_gradients_match_the_uniform_final_pass_on_every_cut_sequence(K, n, T, B):
    from svae_amd.models import slds_svae
    c = _case(K, n, T, B)
    assert {2, T} <= set(c["L"].tolist())
    want = _cut_reference(c)
    clean = _ragged_grads(c, False)
    slds_svae.check_info()
    _check_grads(clean, want, c)
    dirty = _ragged_grads(c, True)
    for k in ("gJ", "gh", "samples", "local_vlb"):
        assert bool(torch.isfinite(dirty[k]).all()), k
        assert torch.equal(dirty[k], clean[k]), k


@pytest.mark.parametrize("K,n,T,B", SHAPES)
def test_labelled_path(K, n, T, B):
    """labels from viterbi_labels(lengths=), -1 beyond L included: values of run_inference_withlabels(lengths=), gradients of
    the uniform labelled call on every cut sequence"""
    from svae_amd.models import slds_svae
    c = _case(K, n, T, B)
    S = c["S"]
    labels, _ = slds_svae.viterbi_labels(c["glob"], (_t(c["J"]), _t(c["h"])), init_eps=_t(c["init_eps"]), lengths=c["L"])
    for b, l in enumerate(c["L"]):
        assert bool((labels[b, l:] == -1).all())
    res = {}
    for nan_pad in (False, True):
        nJ = _padded(c["J"], c, nan_pad).requires_grad_(True)
        nh = _padded(c["h"], c, nan_pad).requires_grad_(True)
        samples, stats, global_vlb, local_vlb = slds_svae.run_inference_withlabels_ragged_differentiable(
            c["prior"], c["glob"], ((nJ, nh), labels), c["L"], S, eps=_padded(c["eps"], c, nan_pad))
        live = torch.arange(T, device="cuda:0")[None, :] < _t(c["L"])[:, None]
        r = torch.where(live[..., None, None], _t(c["r"]), torch.zeros((), dtype=torch.float64, device="cuda:0"))
        (local_vlb + (r * samples).sum()).backward()
        res[nan_pad] = dict(samples=samples.detach(), stats=stats, local_vlb=local_vlb.detach(), gJ=nJ.grad.clone(),
                            gh=nh.grad.clone())
    slds_svae.check_info()
    for k in ("gJ", "gh", "samples", "local_vlb"):
        assert torch.equal(res[True][k], res[False][k]), k
    samples, stats, global_vlb, local_vlb = slds_svae.run_inference_withlabels(
        c["prior"], c["glob"], ((_t(c["J"]), _t(c["h"])), labels), S, eps=_t(c["eps"]), lengths=c["L"])
    assert _rel(res[False]["samples"], samples) < 1e-6
    for a, w in zip(_flat(res[False]["stats"]), _flat(stats)):
        assert _rel(a, w) < 1e-6
    assert float(res[False]["local_vlb"]) == pytest.approx(float(local_vlb), rel=1e-7)
    want = []
    for b, l in enumerate(c["L"]):
        l = int(l)
        nJ = _t(c["J"][b:b + 1, :l]).requires_grad_(True)
        nh = _t(c["h"][b:b + 1, :l]).requires_grad_(True)
        smp, _, _, lv = slds_svae.run_inference_withlabels_differentiable(
            c["prior"], c["glob"], ((nJ, nh), labels[b:b + 1, :l]), S, eps=_t(c["eps"][b:b + 1, :l]))
        (lv + (_t(c["r"][b:b + 1, :l]) * smp).sum()).backward()
        want.append((_np(nJ.grad[0]), _np(nh.grad[0])))
    _check_grads(res[False], want, c)


def test_a_length_of_one_raises_the_status_word_and_the_other_gradients_are_right():
    from svae_amd.models import slds_svae
    c = _case(3, 4, 12, 5)
    L = c["L"].copy()
    L[1] = 1
    want = _cut_reference(c, L)
    with pytest.raises(FloatingPointError, match="sequence lengths"):      # (the reference's ascent saw the same length)
        slds_svae.check_info()
    got = _ragged_grads(c, False, L)
    with pytest.raises(FloatingPointError, match="sequence lengths"):
        slds_svae.check_info()
    slds_svae.check_info()
    _check_grads(got, want, c, rows=[b for b in range(c["B"]) if b != 1], L=L)
    assert bool(torch.isfinite(got["gJ"]).all()) and bool(torch.isfinite(got["gh"]).all())


def test_the_old_names_still_refuse_lengths():
    from svae_amd.models import slds_svae
    c = _case(3, 4, 12, 5)
    node = (_t(c["J"]), _t(c["h"]))
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_differentiable(c["glob"], c["glob"], node, 1, lengths=c["L"])
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_withlabels_differentiable(c["glob"], c["glob"], (node, None), 1, lengths=c["L"])
    with pytest.raises(ValueError, match="latent dimension"):
        rng = np.random.default_rng(0)
        wide = tuple(_t(x) for x in sr.slds_nodes(5, 12, 16, rng))
        slds_svae.run_inference_ragged_differentiable(sr.slds_globals(3, 16, rng), sr.slds_globals(3, 16, rng), wide, c["L"], 1)
    with pytest.raises(ValueError, match="shape"):
        slds_svae.run_inference_withlabels_ragged_differentiable(c["glob"], c["glob"], (node, None), c["L"][:2], 1)
    slds_svae.check_info()
