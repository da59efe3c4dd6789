"""GPU tests of HMM Viterbi decoding (svae_hmm_viterbi_f64, csrc/hmm_viterbi.hip) against the NumPy restatement of the
arithmetic include/svae_hip.h defines (tests/_hmm_viterbi_numpy.py): labels and score are compared EXACTLY."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_viterbi_numpy as vit  # noqa: E402


def _np(x):
    return x.detach().cpu().numpy()


def _problem(B, T, K, rng, scale=1.0, batched_pair=False):
    init = np.log(rng.dirichlet(np.ones(K)))
    shape = (B, K, K) if batched_pair else (K, K)
    pair = np.log(rng.dirichlet(np.ones(K), size=shape[:-1])) + 0.3 * rng.standard_normal(shape)
    node = scale * rng.standard_normal((B, T, K))
    return init, pair, node


def _check_exact(init, pair, node):
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    labels, score = hmm_viterbi((init, pair, node), return_score=True)
    want_l, want_s = vit.viterbi_batch(init, pair, node)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == node.shape[:2]
    assert score.dtype == torch.float64 and tuple(score.shape) == node.shape[:1]
    got_l, got_s = _np(labels), _np(score)
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(vit.bits(got_s), vit.bits(want_s))
    return got_l, got_s


@pytest.mark.parametrize("T", [1, 2, 7, 500])
@pytest.mark.parametrize("K", [1, 2, 5, 8, 15, 16, 17, 31, 32, 33, 48, 64])
def test_viterbi_matches_the_restatement_exactly(K, T):
    """B covers batches that are not a multiple of the four sequences a wavefront takes at K <= 16"""
    for B in (1, 3, 4, 5, 64, 513):
        for scale in (1.0, 50.0):
            rng = np.random.default_rng(100000 * K + 1000 * T + B + int(scale))
            init, pair, node = _problem(B, T, K, rng, scale)
            _check_exact(init, pair, node)


@pytest.mark.parametrize("K", [3, 16, 20, 64])
def test_viterbi_batched_pair_params_and_unbatched_call(K):
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    rng = np.random.default_rng(K)
    B, T = 6, 37
    init, pairs, node = _problem(B, T, K, rng, 2.0, batched_pair=True)
    got_l, got_s = _check_exact(init, pairs, node)
    # the shared-parameter call on one sequence's matrix gives that sequence's row
    l2, s2 = _check_exact(init, pairs[2], node)
    assert np.array_equal(l2[2], got_l[2]) and vit.bits(s2[2]) == vit.bits(got_s[2])
    # unbatched: (T,) int32 labels, 0-d score; labels alone without return_score
    lab, sc = hmm_viterbi((init, pairs[1], node[1]), return_score=True)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == (T,) and sc.dim() == 0 and sc.dtype == torch.float64
    assert np.array_equal(_np(lab), got_l[1]) and vit.bits(_np(sc)) == vit.bits(got_s[1])
    only = hmm_viterbi((init, pairs[1], node[1]))
    assert isinstance(only, torch.Tensor) and np.array_equal(_np(only), got_l[1])
    only_b = hmm_viterbi((init, pairs, torch.as_tensor(node, device="cuda")))
    assert tuple(only_b.shape) == (B, T) and np.array_equal(_np(only_b), got_l)


def test_viterbi_shape_and_state_count_checks_raise_value_error():
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    z = np.zeros
    with pytest.raises(ValueError):
        hmm_viterbi((z(65), z((65, 65)), z((3, 65))))
    with pytest.raises(ValueError):
        hmm_viterbi((z(3), z((3, 3)), z(3)))
    with pytest.raises(ValueError):
        hmm_viterbi((z(4), z((3, 3)), z((5, 3))))
    with pytest.raises(ValueError):
        hmm_viterbi((z(3), z((3, 4)), z((5, 3))))
    with pytest.raises(ValueError):
        hmm_viterbi((z(3), z((2, 3, 3)), z((4, 5, 3))))
    with pytest.raises(ValueError):
        hmm_viterbi((z(3), z((3, 3)), z((2, 0, 3))))


@pytest.mark.parametrize("K", [1, 4, 16, 17, 40, 64])
def test_engineered_ties_resolve_to_the_lowest_index(K):
    B, T = 5, 70
    z = np.zeros
    # all-zero potentials: every path ties
    labels, score = _check_exact(z(K), z((K, K)), z((B, T, K)))
    assert (labels == 0).all() and (score == 0.0).all()
    if K < 2:
        return
    # two identical states (c is a copy of a < c): every tie between them goes to a, so c never appears
    rng = np.random.default_rng(7 + K)
    init, pair, node = _problem(B, T, K, rng, 3.0)
    a, c = (1, K - 1) if K > 2 else (0, 1)
    init[c] = init[a]
    pair[c, :] = pair[a, :]
    pair[:, c] = pair[:, a]
    node[:, :, c] = node[:, :, a]
    labels, _ = _check_exact(init, pair, node)
    assert not (labels == c).any()
    # a tie only at the final step: a deterministic chain into state K-1, whose last observation allows 0 and K-1 alike
    node = np.full((B, T, K), -100.0)
    node[:, :, K - 1] = 0.0
    node[:, T - 1, :] = -100.0
    node[:, T - 1, 0] = 0.0
    node[:, T - 1, K - 1] = 0.0
    labels, _ = _check_exact(z(K), z((K, K)), node)
    assert (labels[:, :-1] == K - 1).all() and (labels[:, -1] == 0).all()


@pytest.mark.parametrize("K", [4, 16, 24, 64])
def test_minus_infinity_entries(K):
    B, T = 7, 90
    rng = np.random.default_rng(11 * K)
    init, pair, node = _problem(B, T, K, rng, 2.0)
    # left-to-right transition matrix: the lower triangle is forbidden
    pair = np.where(np.tril(np.ones((K, K)), -1) > 0, -np.inf, pair)
    labels, score = _check_exact(init, pair, node)
    assert (np.diff(labels, axis=1) >= 0).all() and np.isfinite(score).all()
    # one chain with a forbidden observation: its score is -inf, the chains next to it (same wavefront at K <= 16) are
    # what they are without it
    base_l, base_s = labels.copy(), score.copy()
    node2 = node.copy()
    node2[2, T // 2, :] = -np.inf
    labels, score = _check_exact(init, pair, node2)
    assert score[2] == -np.inf
    keep = np.arange(B) != 2
    assert np.array_equal(labels[keep], base_l[keep]) and np.array_equal(vit.bits(score[keep]), vit.bits(base_s[keep]))
    assert np.isfinite(score[keep]).all()
    # -inf in the initial potentials
    init2 = init.copy()
    init2[0] = -np.inf
    labels, _ = _check_exact(init2, pair, node)
    assert (labels[:, 0] != 0).all()


@pytest.mark.parametrize("K", [6, 16, 29, 64])
def test_nan_inputs_return_labels_in_range(K):
    """NaN potentials: the labels are unspecified but lie in 0..K-1, and the call completes"""
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    rng = np.random.default_rng(K)
    B, T = 6, 150
    init, pair, node = _problem(B, T, K, rng)
    node[1, 40, :] = np.nan
    node[3, :, K // 2] = np.nan
    pair[0, K - 1] = np.nan
    labels, score = hmm_viterbi((init, pair, node), return_score=True)
    torch.cuda.synchronize()
    lab = _np(labels)
    assert lab.min() >= 0 and lab.max() < K


@pytest.mark.parametrize("K,T,B", [(3, 9, 4), (8, 500, 6), (16, 33, 5), (17, 40, 3), (64, 130, 3)])
def test_score_is_the_sum_along_the_returned_path(K, T, B):
    rng = np.random.default_rng(K + T)
    init, pair, node = _problem(B, T, K, rng, 5.0, batched_pair=True)
    labels, score = _check_exact(init, pair, node)
    for b in range(B):
        assert vit.bits(vit.path_score(init, pair[b], node[b], labels[b])) == vit.bits(score[b])


@pytest.mark.parametrize("K", [3, 8, 16, 32, 64])
def test_labels_agree_with_the_estep_marginals_on_near_deterministic_chains(K):
    """potential gap >= 40 between the planted state and every other at every step: the posterior marginals put all but
    e^-40 on the planted path, which is then both the Viterbi path and the argmax of E_states"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_viterbi
    rng = np.random.default_rng(5 * K)
    B, T = 6, 120
    init, pair, _ = _problem(B, T, K, rng)
    planted = rng.integers(0, K, size=(B, T))
    node = rng.standard_normal((B, T, K))
    node[np.arange(B)[:, None], np.arange(T)[None, :], planted] += \
        40.0 + 4 * np.abs(pair).max() + 2 * np.abs(node).max() + 2 * np.abs(init).max()
    labels = hmm_viterbi((init, pair, node))
    _, (_, _, Es) = hmm_estep((init, pair, node))
    assert np.array_equal(_np(labels), planted)
    assert np.array_equal(_np(Es.argmax(-1)), planted)


@pytest.mark.parametrize("K", [8, 40])
def test_viterbi_under_graph_capture_replays_on_new_inputs(K):
    from svae_amd import _lib
    rng = np.random.default_rng(K)
    B, T = 9, 61
    init, pair, node = _problem(B, T, K, rng, 3.0)
    dev = torch.device("cuda")
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    d_init, d_pair, d_node = t(init), t(pair), t(node)
    lib = _lib.load()
    wsb = int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = torch.zeros(B, T, dtype=torch.int32, device=dev)
    score = torch.zeros(B, dtype=torch.float64, device=dev)
    p = _lib.ptr

    def launch():
        rc = lib.svae_hmm_viterbi_f64(B, T, K, 0, p(d_init), p(d_pair), p(d_node), p(states), p(score), p(ws), wsb,
                                      _lib.current_stream(dev))
        assert rc == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    g.replay()
    torch.cuda.synchronize()
    want_l, want_s = vit.viterbi_batch(init, pair, node)
    assert np.array_equal(_np(states), want_l) and np.array_equal(vit.bits(_np(score)), vit.bits(want_s))
    init2, pair2, node2 = _problem(B, T, K, np.random.default_rng(K + 1), 3.0)
    d_init.copy_(t(init2)); d_pair.copy_(t(pair2)); d_node.copy_(t(node2))
    g.replay()
    torch.cuda.synchronize()
    want_l2, want_s2 = vit.viterbi_batch(init2, pair2, node2)
    assert not np.array_equal(want_l2, want_l)
    assert np.array_equal(_np(states), want_l2) and np.array_equal(vit.bits(_np(score)), vit.bits(want_s2))


@pytest.mark.parametrize("K", [5, 33])
def test_caller_supplied_workspace(K):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    rng = np.random.default_rng(K)
    B, T = 5, 23
    init, pair, node = _problem(B, T, K, rng)
    need = int(_lib.load().svae_hmm_viterbi_workspace_bytes(B, T, K))
    want_l, want_s = vit.viterbi_batch(init, pair, node)
    for ws in (torch.empty(need, dtype=torch.uint8, device="cuda"),
               torch.empty(need // 8 + 3, dtype=torch.float64, device="cuda")):
        labels, score = hmm_viterbi((init, pair, node), workspace=ws, return_score=True)
        assert np.array_equal(_np(labels), want_l) and np.array_equal(vit.bits(_np(score)), vit.bits(want_s))
    with pytest.raises(RuntimeError, match="svae_hmm_viterbi_f64"):
        hmm_viterbi((init, pair, node), workspace=torch.empty(need - 16, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
