"""GPU tests of HMM posterior sampling (svae_hmm_sample_f64 / svae_hmm_ragged_sample_f64, csrc/hmm_sample.hip) against
the NumPy oracle tests/_hmm_sample_numpy.py.  Paths are compared EXACTLY: every compared case has a margin of at least
1e-8 between each draw and its nearest decision boundary (asserted in tests/test_hmm_sample_cpu.py), four orders above
the 1e-10 to which the kernels' filtered sums agree with the oracle's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_sample_numpy as smp  # noqa: E402


def _np(x):
    return x.detach().cpu().numpy()


def _check_exact(init, pair, node, u, want, want_lz, **kw):
    from svae_amd.hmm.hmm_inference import hmm_sample
    states, logZ = hmm_sample((init, pair, node), num_samples=u.shape[1], u=u, return_logZ=True, **kw)
    assert states.dtype == torch.int32 and tuple(states.shape) == u.shape
    assert logZ.dtype == torch.float64 and tuple(logZ.shape) == node.shape[:1]
    got, lz = _np(states), _np(logZ)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    np.testing.assert_allclose(lz, want_lz, rtol=1e-10, atol=0)
    return got, lz


@pytest.mark.parametrize("T", smp.GRID_T)
@pytest.mark.parametrize("K", smp.GRID_K)
def test_sampled_paths_match_the_oracle_exactly(K, T):
    """S = 3: B S is never a multiple of the four chains a wavefront takes at K <= 16"""
    for B in smp.GRID_B:
        for scale in smp.GRID_SCALE:
            init, pair, node, u, want, want_lz, margin = smp.grid_case(K, T, B, scale)
            assert margin >= smp.MARGIN
            got, _ = _check_exact(init, pair, node, u, want, want_lz)
            assert got.min() >= 0 and got.max() < K


@pytest.mark.parametrize("K", smp.PAIR_K)
def test_batched_pair_params_unbatched_call_device_input_and_generator(K):
    from svae_amd.hmm.hmm_inference import hmm_sample
    init, pairs, node, u, want, want_lz, _ = smp.pair_case(K)
    B, S, T = u.shape
    got, lz = _check_exact(init, pairs, node, u, want, want_lz)
    # unbatched: (S,T) labels, 0-d logZ; labels alone without return_logZ
    lab, z1 = hmm_sample((init, pairs[1], node[1]), num_samples=S, u=u[1], return_logZ=True)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == (S, T) and z1.dim() == 0 and z1.dtype == torch.float64
    assert np.array_equal(_np(lab), want[1]) and float(z1) == lz[1]
    only = hmm_sample((init, pairs[1], node[1]), num_samples=S, u=u[1])
    assert isinstance(only, torch.Tensor) and np.array_equal(_np(only), want[1])
    # device tensors
    dev = lambda x: torch.as_tensor(x, device="cuda")
    only_b = hmm_sample((init, dev(pairs), dev(node)), num_samples=S, u=dev(u))
    assert tuple(only_b.shape) == (B, S, T) and np.array_equal(_np(only_b), want)
    # u=None: torch.rand with the generator -- the same labels twice, and those of the uniforms it draws
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + K)
    a = hmm_sample((init, pairs, node), num_samples=5, generator=g)
    g.manual_seed(1234 + K)
    b = hmm_sample((init, pairs, node), num_samples=5, generator=g)
    assert tuple(a.shape) == (B, 5, T) and a.dtype == torch.int32 and torch.equal(a, b)
    g.manual_seed(1234 + K)
    ug = torch.rand(B, 5, T, dtype=torch.float64, device="cuda", generator=g)
    assert torch.equal(hmm_sample((init, pairs, node), num_samples=5, u=ug), a)
    assert int(a.min()) >= 0 and int(a.max()) < K


@pytest.mark.parametrize("K", smp.PAIR_K)
def test_per_sequence_lengths(K):
    from svae_amd.hmm.hmm_inference import hmm_sample, check_lengths_status
    init, pairs, node, u, L, want, want_lz, _ = smp.ragged_case(K)
    B, S, T = u.shape
    assert np.isnan(node[0, 1:]).all() and np.isnan(u[0, :, 1:]).all()
    got, lz = _check_exact(init, pairs, node, u, want, want_lz, lengths=L, check=True)
    for b in range(B):
        l = int(L[b])
        assert (got[b, :, l:] == -1).all() and got[b, :, :l].min() >= 0
        alone, z1 = hmm_sample((init, pairs[b], node[b, :l]), num_samples=S, u=u[b, :, :l], return_logZ=True)
        assert np.array_equal(_np(alone), got[b, :, :l]) and float(z1) == pytest.approx(lz[b], rel=1e-12)
    # shared pair parameters, lengths as a device tensor
    w2, z2, _ = smp.sample_ragged(init, pairs[3], node, u, L)
    _check_exact(init, pairs[3], node, u, w2, z2, lengths=torch.as_tensor(L, device="cuda"))
    # a length of 0 and one of T + 1: clamped to 1 and T, and the status raised under check=True
    L2 = L.copy()
    L2[0], L2[1] = 0, T + 1
    with pytest.raises(FloatingPointError):
        hmm_sample((init, pairs, node), num_samples=S, u=u, lengths=L2, check=True)
    check_lengths_status()                                               # (cleared by the read above)
    clamped = _np(hmm_sample((init, pairs, node), num_samples=S, u=u, lengths=L2))
    with pytest.raises(FloatingPointError):
        check_lengths_status()
    assert np.array_equal(clamped, want)


@pytest.mark.parametrize("K", smp.LTR_K)
def test_forbidden_transitions_are_never_drawn(K):
    init, pair, node, u, want, want_lz, _ = smp.ltr_case(K)
    got, lz = _check_exact(init, pair, node, u, want, want_lz)
    assert (np.diff(got, axis=2) >= 0).all() and np.isfinite(lz).all()


@pytest.mark.parametrize("K", smp.LTR_K)
def test_forbidden_observations_and_the_ends_of_the_unit_interval(K):
    """states 0 and K-1 have -inf node potentials throughout; columns of u at 0, 1 - 2^-53, -1, 2 and NaN"""
    from svae_amd.hmm.hmm_inference import hmm_sample
    rng = np.random.default_rng(11 * K + 1)
    B, T, S = 7, 90, 8
    init, pair, node, u = smp.problem(B, T, K, S, rng, 2.0)
    node[:, :, 0] = -np.inf
    node[:, :, K - 1] = -np.inf
    u[:, 0, :] = 0.0
    u[:, 1, :] = 1.0 - 2.0 ** -53
    u[:, 2, :] = -1.0
    u[:, 3, :] = 2.0
    u[:, 4, :] = np.nan
    u[:, 5, ::3] = 0.0
    u[:, 5, 1::3] = 2.0
    states, logZ = hmm_sample((init, pair, node), num_samples=S, u=u, return_logZ=True)
    got = _np(states)
    assert np.isfinite(_np(logZ)).all()
    assert got.min() >= 1 and got.max() <= K - 2
    for s in (0, 2, 4):
        assert (got[:, s] == 1).all()                                    # the lowest allowed state
    for s in (1, 3):
        assert (got[:, s] == K - 2).all()                                # the highest
    np.testing.assert_allclose(_np(logZ), smp.sample_batch(init, pair, node, u)[1], rtol=1e-10)


@pytest.mark.parametrize("K", smp.PAIR_K)
def test_a_chain_with_an_impossible_step_leaves_its_neighbours_alone(K):
    from svae_amd.hmm.hmm_inference import hmm_sample
    init, pair, node, u, want, want_lz, _ = smp.pair_case(K)
    B, S, T = u.shape
    node2 = node.copy()
    node2[2, T // 2, :] = -np.inf
    states, logZ = hmm_sample((init, pair, node2), num_samples=S, u=u, return_logZ=True)
    got, lz = _np(states), _np(logZ)
    assert got.min() >= 0 and got.max() < K
    keep = np.arange(B) != 2
    assert np.array_equal(got[keep], want[keep])
    np.testing.assert_allclose(lz[keep], want_lz[keep], rtol=1e-10)
    assert lz[2] == -np.inf or np.isnan(lz[2])
    # NaN potentials: labels in range, neighbours untouched
    node3 = node.copy()
    node3[2, T // 3, :] = np.nan
    node3[2, :, K // 2] = np.nan
    got3 = _np(hmm_sample((init, pair, node3), num_samples=S, u=u))
    assert got3.min() >= 0 and got3.max() < K and np.array_equal(got3[keep], want[keep])


def _forced(K):
    """the forced-transition model of tests/test_hmm_hip.py: state 0 is the only possible state up to t = 5, impossible
    afterwards, and its only exit is an entry of log-potential -800; padded to K states forbidden by -1e4 potentials"""
    T = 12
    init = np.full(K, -1e4)
    init[0] = 0.0
    pair = np.zeros((K, K))
    pair[:3, :3] = np.array([[0.0, -800.0, -1e4], [-1e4, 0.0, -1.0], [-1e4, -1.0, 0.0]])
    node = np.zeros((2, T, K))
    node[0, :6, 1:] = -1e4
    node[0, 6:, 0] = -1e4
    node[1, :, :3] = 0.3 * np.random.default_rng(0).standard_normal((T, 3))     # an ordinary sequence next to it
    node[:, :, 3:] = -1e4
    return init, pair, node


@pytest.mark.parametrize("K", [3, 20])
def test_draws_through_a_transition_that_underflows(K):
    from svae_amd.hmm.hmm_inference import hmm_sample
    init, pair, node = _forced(K)
    S = 4
    u = np.random.default_rng(K).random((2, S, node.shape[1]))
    want, want_lz, margin = smp.sample_batch(init, pair, node, u)
    states, logZ = hmm_sample((init, pair, node), num_samples=S, u=u, return_logZ=True)
    got, lz = _np(states), _np(logZ)
    assert (got[0, :, :6] == 0).all() and (got[0, :, 6:] != 0).all() and got.max() < 3
    np.testing.assert_allclose(lz, want_lz, rtol=1e-9)
    assert lz[0] < -790
    assert np.array_equal(got[1], want[1])                               # the neighbour is exact


def test_samples_have_the_posterior_marginals():
    """K = 5, T = 20, B = 2, S = 4096, u drawn on the device: every cell within 5 binomial standard deviations of
    hmm_estep's E_states"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_sample
    K, T, B, S = 5, 20, 2, 4096
    init, pair, node, _ = smp.problem(B, T, K, 1, np.random.default_rng(5), 1.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    states = hmm_sample((init, pair, node), num_samples=S, generator=g)
    _, (_, _, Es) = hmm_estep((init, pair, node))
    Es = _np(Es)
    got = _np(states)
    freq = np.stack([(got == k).mean(1) for k in range(K)], -1)          # (B,T,K)
    sd = np.sqrt(Es * (1 - Es) / S)
    print("worst cell: %.2f sd" % np.abs((freq - Es) / sd).max())
    assert (np.abs(freq - Es) <= 5 * sd).all()


def test_shape_state_count_and_sample_checks_raise_value_error_before_any_launch():
    from svae_amd.hmm.hmm_inference import hmm_sample
    z = np.zeros
    bad = [dict(nat=(z(65), z((65, 65)), z((3, 65)))),
           dict(nat=(z(3), z((3, 3)), z(3))),
           dict(nat=(z(4), z((3, 3)), z((5, 3)))),
           dict(nat=(z(3), z((3, 4)), z((5, 3)))),
           dict(nat=(z(3), z((2, 3, 3)), z((4, 5, 3)))),
           dict(nat=(z(3), z((3, 3)), z((2, 0, 3)))),
           dict(nat=(z(3), z((3, 3)), z((2, 5, 3))), num_samples=0),
           dict(nat=(z(3), z((3, 3)), z((2, 5, 3))), num_samples=-1),
           dict(nat=(z(3), z((3, 3)), z((2, 5, 3))), num_samples=2, u=z((2, 3, 5))),
           dict(nat=(z(3), z((3, 3)), z((2, 5, 3))), num_samples=2, u=z((2, 5))),
           dict(nat=(z(3), z((3, 3)), z((5, 3))), num_samples=2, u=z((1, 2, 5))),
           dict(nat=(z(3), z((3, 3)), z((2, 5, 3))), lengths=np.array([1, 2, 3])),
           dict(nat=(z(3), z((3, 3)), z((5, 3))), lengths=np.array([1]))]
    for kw in bad:
        nat = kw.pop("nat")
        with pytest.raises(ValueError):
            hmm_sample(nat, **kw)
    ok = hmm_sample((z(3), z((3, 3)), z((5, 3))), num_samples=2, u=z((2, 5)))
    assert tuple(ok.shape) == (2, 5) and int(ok.abs().max()) == 0


def _slds_model(seed=3):
    from oracle import expfam_numpy as ef
    K, n, B, T = 3, 4, 5, 12
    rng = np.random.default_rng(seed)

    def globals_():
        lds = []
        for k in range(K):
            nu, Sm = n + 1. + rng.random(), 2. * (n + 1) * np.eye(n)
            M = 0.95 * np.eye(n)
            th = 0.4 * (k + 1)
            M[:2, :2] = 0.95 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            lds.append((ef.niw_standard_to_natural(Sm, 0.3 * rng.standard_normal(n), np.array(0.5), np.array(nu)),
                        ef.mniw_standard_to_natural(nu, Sm, M, 0.2 * np.eye(n))))
        return (rng.random(K) * 2., rng.random((K, K)) * 2. + 3. * np.eye(K)), lds

    glob, prior = globals_(), globals_()
    J = -0.5 * (0.5 + rng.random((B, T, n)))
    h = rng.standard_normal((B, T, n)) * 2.
    node = (torch.as_tensor(J, device="cuda"), torch.as_tensor(h, device="cuda"))
    return prior, glob, node, (K, n, B, T)


@pytest.mark.parametrize("ragged", [False, True])
def test_slds_sample_labels_draws_from_the_converged_hmm_factor(ragged):
    from svae_amd.hmm.hmm_inference import hmm_sample
    from svae_amd.models import slds_svae
    prior, glob, node, (K, n, B, T) = _slds_model()
    rng = np.random.default_rng(9)
    S = 3
    init_eps = torch.as_tensor(rng.standard_normal((B, T, 1, n)), device="cuda")
    u = torch.as_tensor(rng.random((B, S, T)), device="cuda")
    lengths = np.array([T, 2, 7, T - 1, 3]) if ragged else None
    labels = slds_svae.sample_labels(glob, node, num_samples=S, init_eps=init_eps, u=u, lengths=lengths)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (B, S, T)
    _, (hmm_nat, _), _, _ = slds_svae.optimize_local_meanfield(glob, node, init_eps, 1e-2, pair_stats=False,
                                                               lengths=lengths)
    want = hmm_sample(hmm_nat, num_samples=S, u=u, lengths=lengths)
    assert torch.equal(labels, want)
    lab = _np(labels)
    if ragged:
        for b in range(B):
            assert (lab[b, :, lengths[b]:] == -1).all() and lab[b, :, :lengths[b]].min() >= 0
    else:
        assert lab.min() >= 0
    assert lab.max() < K
    samples, _, global_vlb, local_vlb = slds_svae.run_inference_withlabels(
        prior, glob, (node, labels[:, 0]), 1, eps=torch.as_tensor(rng.standard_normal((B, T, 1, n)), device="cuda"),
        lengths=lengths)
    assert tuple(samples.shape) == (B, T, 1, n)
    assert bool(torch.isfinite(local_vlb)) and bool(torch.isfinite(global_vlb))
