"""GPU tests of `lengths=` on the SLDS model layer (svae_amd/models/slds_svae.py): one padded batch of sequences of
different lengths against oracle/slds_numpy.py run on every sequence cut at its own length -- node[b, :L], init_eps[b, :L],
eps[b, :L] -- with the bounds of tests/test_slds_hip.py: equal sweep counts, the two bounds to rel 1e-7, marginals and
statistics to 1e-6 in that file's measure, exact zeros beyond L.

Equal sweep counts mean something only where the reference's own stopping test is not marginal: the seeds below were
chosen on the CPU so that the oracle's count of every test sequence is the same at tol (1 - 1e-3), tol and tol (1 + 1e-3);
tests/_slds_ragged_numpy.py asserts that from the oracle alone each time the reference is built."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _slds_ragged_numpy as sr  # noqa: E402
from oracle import slds_numpy  # noqa: E402  (checker only)

# (K, n, T, B) -> seed; K = 20: more states than a DPP row holds, the HMM step runs its wide ragged kernel
SEEDS = {(3, 4, 12, 5): 304, (8, 10, 20, 6): 810, (5, 15, 6, 4): 515, (20, 3, 10, 3): 2003}
SHAPES = list(SEEDS)


def _np(x):
    return x.detach().cpu().numpy()


def _err(got, want):
    """relative to max(|want_ij|, 1e-3 max|want|): entries that cancel to ~0 are judged on the array's scale"""
    got, want = _np(got), np.asarray(want, float)
    if not want.size:
        return 0.0
    scale = np.maximum(np.abs(want), 1e-3 * max(np.max(np.abs(want)), 1e-300))
    return float(np.max(np.abs(got - want) / scale))


def _close(got, want, tol=1e-6):
    err = _err(got, want)
    assert err < tol, err


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


@functools.lru_cache(maxsize=None)
def _case(K, n, T, B, compat=True, full=False):
    """inputs and the oracle's ascent on every cut sequence (computed once, shared, left unchanged)"""
    c = sr.slds_case(K, n, T, B, SEEDS[(K, n, T, B)])
    if full:
        c["L"] = np.full(B, T, dtype=np.int64)
    c["refs"] = sr.slds_cut_ascent(c["glob"], c["J"], c["h"], c["init_eps"], c["L"], compat=compat)
    return c


def _node(c, nan_pad=True):
    """device node potentials, NaN from each sequence's length on"""
    J, h = c["J"].copy(), c["h"].copy()
    if nan_pad:
        for b, L in enumerate(c["L"]):
            J[b, L:] = np.nan
            h[b, L:] = np.nan
    return _t(J), _t(h)


def _noise(x, c):
    x = x.copy()
    for b, L in enumerate(c["L"]):
        x[b, L:] = np.nan
    return _t(x)


@pytest.mark.parametrize("K,n,T,B,compat", [s + (True,) for s in SHAPES] + [(3, 4, 12, 5, False)])
def test_optimize_local_meanfield_with_lengths_matches_oracle(K, n, T, B, compat):
    from svae_amd.models import slds_svae
    c = _case(K, n, T, B, compat)
    assert B < 4 or {2, 3, T - 1, T} <= set(c["L"].tolist())
    (hmm_stats, lds_stats), _, (hmm_vlb, lds_vlb), iters = slds_svae.optimize_local_meanfield(
        c["glob"], _node(c), _noise(c["init_eps"], c), reference_compat=compat, lengths=c["L"])
    slds_svae.check_info()
    print("sweeps:", iters.tolist(), "oracle:", [r["iters"] for r in c["refs"]])
    for b, ref in enumerate(c["refs"]):
        L = int(c["L"][b])
        assert int(iters[b]) == ref["iters"]
        assert float(hmm_vlb[b]) == pytest.approx(ref["hmm_vlb"], rel=1e-7, abs=1e-7)
        assert float(lds_vlb[b]) == pytest.approx(ref["lds_vlb"], rel=1e-7, abs=1e-7)
        _close(hmm_stats[0][b], ref["hmm_stats"][0])
        _close(hmm_stats[1][b], ref["hmm_stats"][1])
        _close(hmm_stats[2][b, :L], ref["hmm_stats"][2])
        assert bool((hmm_stats[2][b, L:] == 0).all())
        for got, want in zip(lds_stats[0], ref["init_stats"]):
            _close(got[b], want)
        for got, want in zip(lds_stats[1], ref["pair_stats"]):
            _close(got[b, :L - 1], want)
            assert bool((got[b, L - 1:] == 0).all())
        for got, want in zip(lds_stats[2], ref["node_stats"]):
            _close(got[b, :L], want)
            assert bool((got[b, L:] == 0).all())


@pytest.mark.parametrize("K,n,T,B", SHAPES)
def test_run_inference_with_lengths(K, n, T, B):
    """global statistics = the sum over the sequences of the oracle's get_global_stats on the cut sequences (1e-6); the
    pair count is the marginals summed over each sequence's own L-1 pairs; samples beyond L are 0; local_vlb is finite and
    the per-sequence sum, with NaN in the padding of the node potentials and of both noise arrays"""
    from svae_amd.models import slds_svae
    from svae_amd.lds.lds_inference import LDSEStepPlan
    c = _case(K, n, T, B)
    S = c["S"]
    prior = sr.slds_globals(K, n, np.random.default_rng(1))
    node = _node(c)
    samples, (hmm_g, (g_init, g_pair)), global_vlb, local_vlb = slds_svae.run_inference(
        prior, c["glob"], node, S, init_eps=_noise(c["init_eps"], c), eps=_noise(c["eps"], c), lengths=c["L"])
    slds_svae.check_info()
    (Ei, Et), (want_init, want_pair) = sr.slds_global_stats_sum(c["refs"])
    np.testing.assert_allclose(_np(hmm_g[0]), Ei, rtol=1e-6)
    _close(hmm_g[1], Et)
    for got, want in zip(g_init, want_init):
        _close(got, want)
    for got, want in zip(g_pair, want_pair):
        _close(got, want)
    count = sum(r["hmm_stats"][2][1:].sum(0) for r in c["refs"])
    _close(g_pair[3], count)
    assert float(g_pair[3].sum()) == pytest.approx(float(sum(int(L) - 1 for L in c["L"])), rel=1e-9)
    assert tuple(samples.shape) == (B, T, S, n)
    want_vlb = 0.0
    for b, ref in enumerate(c["refs"]):
        L = int(c["L"][b])
        assert bool(torch.isfinite(samples[b, :L]).all()) and bool((samples[b, L:] == 0).all())
        # the sequence's own final pass in the oracle: the LDS step on the converged marginals, the HMM bound on its statistics
        glob = c["glob"]
        inits, pairs = slds_numpy.get_all_lds_local_natparams(glob[1])
        nodes = (c["J"][b, :L], c["h"][b, :L])
        lognorm, init_stats, pair_stats, node_stats, nat = slds_numpy.lds_meanfield(inits, pairs, nodes, ref["hmm_stats"][2])
        from oracle import expfam_numpy as ef, hmm_numpy, lds_numpy
        node_hmm = slds_numpy.get_arhmm_local_nodeparams(inits, pairs, init_stats, pair_stats)
        hmm_vlb, _ = hmm_numpy.hmm_estep((ef.dirichlet_expectedstats(glob[0][0]), ef.dirichlet_expectedstats(glob[0][1]),
                                          node_hmm))
        want_vlb += hmm_vlb + lognorm - (np.sum(nodes[0] * node_stats[0]) + np.sum(nodes[1] * node_stats[1]))
        messages, _ = lds_numpy.natural_filter_forward_general(nat[0][:3], nat[1], lds_numpy._canonical_node_params(nodes))
        smp = lds_numpy.natural_sample_backward_general(messages, nat[1], c["eps"][b, :L])
        _close(samples[b, :L], smp)
    assert np.isfinite(float(local_vlb)) and np.isfinite(float(global_vlb))
    assert float(local_vlb) == pytest.approx(want_vlb, rel=1e-7)


def test_padding_is_not_a_substitute():
    """on a batch with some L < T the marginals of the ragged call differ from the uniform call's by more than 1e-3"""
    from svae_amd.models import slds_svae
    c = _case(3, 4, 12, 5)
    node = _node(c, nan_pad=False)
    eps = _t(c["init_eps"])
    (hs_r, _), _, _, _ = slds_svae.optimize_local_meanfield(c["glob"], node, eps, lengths=c["L"])
    (hs_u, _), _, _, _ = slds_svae.optimize_local_meanfield(c["glob"], node, eps, fused=False)
    worst = 0.0
    for b, L in enumerate(c["L"]):
        d = float((hs_r[2][b, :L] - hs_u[2][b, :L]).abs().max())
        if L == c["T"]:
            assert d < 1e-10
        else:
            worst = max(worst, d)
    assert worst > 1e-3, worst


def test_viterbi_labels_round_trip_with_lengths():
    """viterbi_labels(lengths=) gives -1 beyond L; fed unchanged to run_inference_withlabels(lengths=) the labelled step
    matches the oracle's on the cut sequences: HMM statistics 1e-12, pair / node statistics 1e-6"""
    from svae_amd.models import slds_svae
    K, n, T, B = 3, 4, 12, 5
    c = _case(K, n, T, B)
    node = _node(c)
    labels, score = slds_svae.viterbi_labels(c["glob"], node, init_eps=_noise(c["init_eps"], c), lengths=c["L"])
    lab = _np(labels)
    assert bool(torch.isfinite(score).all())
    for b, L in enumerate(c["L"]):
        assert np.all(lab[b, L:] == -1) and np.all((lab[b, :L] >= 0) & (lab[b, :L] < K))
    (hmm_stats, lds_stats), _, (_, lds_vlb) = slds_svae.optimize_local_meanfield_withlabels(c["glob"], node, labels,
                                                                                        lengths=c["L"])
    prior = sr.slds_globals(K, n, np.random.default_rng(1))
    samples, (hmm_g, (g_init, g_pair)), global_vlb, local_vlb = slds_svae.run_inference_withlabels(
        prior, c["glob"], (node, labels), c["S"], eps=_noise(c["eps"], c), lengths=c["L"])
    slds_svae.check_info()
    tot_pair, tot_trans, tot_vlb = None, 0.0, 0.0
    for b, L in enumerate(c["L"]):
        L = int(L)
        ref = slds_numpy.optimize_local_meanfield_withlabels(c["glob"], (c["J"][b, :L], c["h"][b, :L]), lab[b, :L])
        assert float(lds_vlb[b]) == pytest.approx(ref["lds_vlb"], rel=1e-8)
        np.testing.assert_allclose(_np(hmm_stats[0][b]), ref["hmm_stats"][0])
        np.testing.assert_allclose(_np(hmm_stats[1][b]), ref["hmm_stats"][1])
        np.testing.assert_allclose(_np(hmm_stats[2][b, :L]), ref["hmm_stats"][2], rtol=1e-12)
        assert bool((hmm_stats[2][b, L:] == 0).all())
        for got, want in zip(lds_stats[1], ref["pair_stats"]):
            _close(got[b, :L - 1], want)
            assert bool((got[b, L - 1:] == 0).all())
        for got, want in zip(lds_stats[2], ref["node_stats"]):
            _close(got[b, :L], want)
            assert bool((got[b, L:] == 0).all())
        assert bool((samples[b, L:] == 0).all()) and bool(torch.isfinite(samples[b, :L]).all())
        (_, Et), (_, gp) = slds_numpy.get_global_stats(ref["hmm_stats"], ref["init_stats"], ref["pair_stats"])
        tot_pair = gp if tot_pair is None else tuple(x + y for x, y in zip(tot_pair, gp))
        tot_trans = tot_trans + Et
        tot_vlb += ref["lds_vlb"] - (np.sum(c["J"][b, :L] * ref["node_stats"][0]) + np.sum(c["h"][b, :L] * ref["node_stats"][1]))
    np.testing.assert_allclose(_np(hmm_g[1]), tot_trans, rtol=1e-12)
    for got, want in zip(g_pair, tot_pair):
        _close(got, want)
    assert float(local_vlb) == pytest.approx(tot_vlb, rel=1e-7)


def test_all_lengths_T_agree_with_the_uniform_materialised_call():
    from svae_amd.models import slds_svae
    K, n, T, B = 3, 4, 12, 5
    c = _case(K, n, T, B, True, True)
    node = _node(c, nan_pad=False)
    eps = _t(c["init_eps"])
    (hs_r, ls_r), _, (hv_r, lv_r), it_r = slds_svae.optimize_local_meanfield(c["glob"], node, eps, lengths=c["L"])
    (hs_u, ls_u), _, (hv_u, lv_u), it_u = slds_svae.optimize_local_meanfield(c["glob"], node, eps, fused=False)
    assert torch.equal(it_r.cpu(), it_u.cpu())
    assert [int(i) for i in it_r] == [r["iters"] for r in c["refs"]]
    pairs = [(hv_r, hv_u), (lv_r, lv_u)] + list(zip(hs_r, hs_u)) + list(zip(ls_r[0], ls_u[0])) + \
        list(zip(ls_r[1], ls_u[1])) + list(zip(ls_r[2], ls_u[2]))
    for got, want in pairs:
        _close(got, _np(want), 1e-10)


def test_lengths_errors_come_before_any_launch():
    from svae_amd.models import slds_svae
    c = _case(3, 4, 12, 5)
    node = _node(c, nan_pad=False)
    eps = _t(c["init_eps"])
    L = c["L"]
    with pytest.raises(ValueError, match="fused"):
        slds_svae.optimize_local_meanfield(c["glob"], node, eps, fused=True, lengths=L)
    with pytest.raises(ValueError, match="shape"):
        slds_svae.optimize_local_meanfield(c["glob"], node, eps, lengths=L[:2])
    with pytest.raises(ValueError, match="integers"):
        slds_svae.run_inference(c["glob"], c["glob"], node, 1, lengths=L.astype(float))
    with pytest.raises(ValueError, match="integers"):
        slds_svae.viterbi_labels(c["glob"], node, lengths=torch.as_tensor(L, device="cuda:0").double())
    rng = np.random.default_rng(0)
    wide = tuple(_t(x) for x in sr.slds_nodes(5, 12, 16, rng))
    with pytest.raises(ValueError, match="latent dimension"):
        slds_svae.run_inference(sr.slds_globals(3, 16, rng), sr.slds_globals(3, 16, rng), wide, 1, lengths=L)
    glob65 = (c["glob"][0], [c["glob"][1][0]] * 65)
    with pytest.raises(ValueError, match="discrete states"):
        slds_svae.optimize_local_meanfield(glob65, node, eps, lengths=L)
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_differentiable(c["glob"], c["glob"], node, 1, lengths=L)
    with pytest.raises(ValueError, match="lengths"):
        slds_svae.run_inference_withlabels_differentiable(c["glob"], c["glob"], (node, None), 1, lengths=L)
    slds_svae.check_info()


def test_a_length_of_one_raises_the_slds_status_word():
    """the SLDS has no one-step sequence: the length is clamped to 2 on the device, the status word is raised, and the
    other sequences are right"""
    from svae_amd.models import slds_svae
    c = _case(3, 4, 12, 5)
    L = c["L"].copy()
    L[1] = 1
    (hmm_stats, lds_stats), _, (hmm_vlb, lds_vlb), iters = slds_svae.optimize_local_meanfield(
        c["glob"], _node(c, nan_pad=False), _t(c["init_eps"]), lengths=torch.as_tensor(L, device="cuda:0"))
    with pytest.raises(FloatingPointError, match="sequence lengths"):
        slds_svae.check_info()
    slds_svae.check_info()
    for b, ref in enumerate(c["refs"]):
        if b == 1:
            continue
        assert int(iters[b]) == ref["iters"]
        assert float(lds_vlb[b]) == pytest.approx(ref["lds_vlb"], rel=1e-7, abs=1e-7)
        _close(hmm_stats[2][b, :int(L[b])], ref["hmm_stats"][2])
    assert bool(torch.isfinite(lds_vlb).all()) and bool(torch.isfinite(hmm_stats[2]).all())
