"""GPU tests of Viterbi decoding and posterior sampling with per-step transition potentials (hmm_viterbi_perstep,
hmm_sample_perstep; svae_hmm_perstep_viterbi_f64, svae_hmm_perstep_sample_f64) against the NumPy oracles of
tests/_hmm_perstep_decode_numpy.py.

Viterbi: every comparison is bit for bit (the arithmetic is defined: fp64 additions in a fixed order, strict compares).
Sampling: label for label on cases whose smallest margin is >= 1e-8 (asserted here again and in
tests/test_hmm_perstep_decode_cpu.py; no draw is excluded); log Z bit for bit against hmm_logZ_perstep (the sweep is
shared) and against the oracle at TOL_LOG of tests/test_hmm_perstep_hip.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_perstep_decode_numpy as pd  # noqa: E402
import _hmm_sample_numpy as sm  # noqa: E402

TOL_LOG_LZ = dict(rel=1e-9, abs=1e-9)                                   # TOL_LOG["lz"] of tests/test_hmm_perstep_hip.py


def _np(x):
    return x.detach().cpu().numpy()


def _viterbi(natparam, **kw):
    from svae_amd.hmm.hmm_inference import hmm_viterbi_perstep
    labels, score = hmm_viterbi_perstep(natparam, return_score=True, **kw)
    assert labels.dtype == torch.int32 and score.dtype == torch.float64
    return _np(labels), _np(score)


def _sample(natparam, u, **kw):
    from svae_amd.hmm.hmm_inference import hmm_sample_perstep
    states, logZ = hmm_sample_perstep(natparam, num_samples=u.shape[-2], u=u, return_logZ=True, **kw)
    assert states.dtype == torch.int32 and logZ.dtype == torch.float64
    return _np(states), _np(logZ)


def _assert_viterbi(case, got):
    labels, score = got
    assert labels.shape == case.labels.shape and score.shape == case.score.shape
    assert np.array_equal(labels, case.labels)
    assert np.array_equal(pd.bits(score), pd.bits(case.score))
    pair = np.broadcast_to(case.pair, (case.node.shape[0],) + case.pair.shape[-3:])
    for b in range(case.node.shape[0]):
        assert pd.bits(score[b]) == pd.bits(pd.path_score(case.init, pair[b], case.node[b], labels[b]))


# ---- Viterbi ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", pd.GRID_K)
def test_perstep_viterbi_grid_bit_for_bit(K):
    for case in pd.grid_cases(K):
        _assert_viterbi(case, _viterbi(case.natparam))
    if K in pd.LONG_K:                                                   # T across the backtrace's block sizes
        for case in pd.long_cases(K):
            _assert_viterbi(case, _viterbi(case.natparam))
    # the unbatched call: the batch's sequence
    from svae_amd.hmm.hmm_inference import hmm_viterbi_perstep
    case = pd.grid_cases(K)[-1]                                          # T = 37, B = 9, per-sequence pair parameters
    lab, sc = hmm_viterbi_perstep((case.init, case.pair[1], case.node[1]), return_score=True)
    assert lab.shape == (37,) and sc.shape == ()
    assert np.array_equal(_np(lab), case.labels[1]) and pd.bits(_np(sc)) == pd.bits(case.score[1])
    only = hmm_viterbi_perstep((case.init, case.pair[1], case.node[1]))
    assert torch.equal(only, lab)


@pytest.mark.parametrize("K", pd.TIE_K)
def test_perstep_viterbi_ties_go_to_the_lowest_index(K):
    _assert_viterbi(pd.tie_case(K), _viterbi(pd.tie_case(K).natparam))


@pytest.mark.parametrize("K", pd.LTR_K)
def test_perstep_viterbi_forbidden_transitions(K):
    case = pd.ltr_case(K)
    got = _viterbi(case.natparam)
    _assert_viterbi(case, got)
    assert (np.diff(got[0], axis=-1) >= 0).all() and np.isfinite(got[1]).all()
    dead = pd.dead_step_case(K)                                          # one all -inf step: score -inf, the oracle's labels
    labels, score = _viterbi(dead.natparam)
    assert (score == -np.inf).all() and np.array_equal(labels, dead.labels)


@pytest.mark.parametrize("K", [3, 16, 17, 64])
def test_perstep_viterbi_reduces_to_the_uniform_viterbi_at_constant_matrices(K):
    from svae_amd.hmm.hmm_inference import hmm_viterbi, hmm_viterbi_perstep
    B, T = 5, 37
    rng = np.random.default_rng(4000 + K)
    init, pair, node, _ = sm.problem(B, T, K, 1, rng, 1.5, batched_pair=True)
    for P, per in ((pair, np.broadcast_to(pair[:, None], (B, T - 1, K, K)).copy()),
                   (pair[0], np.broadcast_to(pair[0], (T - 1, K, K)).copy())):
        a = hmm_viterbi_perstep((init, per, node), return_score=True)
        b = hmm_viterbi((init, P, node), return_score=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("K", [3, 8, 16, 17, 33, 64])
def test_perstep_viterbi_with_lengths(K):
    r = pd.ragged_case(K)
    init, pair, node, u, L = r["init"], r["pair"], r["node"], r["u"], r["L"]
    nan_pair, nan_node, _ = pd.padded(pair, node, u, L)
    labels, score = _viterbi((init, nan_pair, nan_node), lengths=L, check=True)
    assert np.array_equal(labels, r["labels"]) and np.array_equal(pd.bits(score), pd.bits(r["score"]))
    for b, l in enumerate(L):
        assert (labels[b, l:] == -1).all()
    # shared pair parameters (finite everywhere: another sequence may need the step), NaN nodes
    s_lab, s_sc = _viterbi((init, pair[0], nan_node), lengths=torch.tensor(L))
    assert np.array_equal(s_lab, r["shared"][0][0]) and np.array_equal(pd.bits(s_sc), pd.bits(r["shared"][0][1]))
    # no sequence sees another's length: the other sequences permuted, and sequence 0's neighbours' lengths moved
    perm = np.random.default_rng(K).permutation(len(L))
    p_lab, p_sc = _viterbi((init, nan_pair[perm], nan_node[perm]), lengths=L[perm])
    assert np.array_equal(p_lab, labels[perm]) and np.array_equal(pd.bits(p_sc), pd.bits(score[perm]))
    other = L.copy()
    other[1:] = other[1:][::-1]
    o_pair, o_node, _ = pd.padded(pair, node, u, other)
    o_lab, o_sc = _viterbi((init, o_pair, o_node), lengths=other)
    assert np.array_equal(o_lab[0], labels[0]) and pd.bits(o_sc[0]) == pd.bits(score[0])


def test_perstep_decode_clamps_a_length_outside_1_to_T_and_says_so():
    from svae_amd.hmm.hmm_inference import check_lengths_status, hmm_sample_perstep, hmm_viterbi_perstep
    B, T, K = 5, 6, 4
    rng = np.random.default_rng(61)
    init, pair, node, u = pd.problem(B, T, K, 2, rng, False)
    try:
        check_lengths_status()                                           # start from a clean word
    except FloatingPointError:
        pass
    good = np.array([1, T, 3, 1, T])
    for fn in (lambda **kw: hmm_viterbi_perstep((init, pair, node), **kw),
               lambda **kw: hmm_sample_perstep((init, pair, node), num_samples=2, u=u, **kw)):
        for bad in (np.array([0, T + 1, 3, -5, 1000]), np.array([0, T, 3, 1, T]), np.array([1, T + 1, 3, 1, T])):
            got = fn(lengths=bad)                                        # check=False: no synchronisation, no error
            clamped = fn(lengths=np.clip(bad, 1, T))
            with pytest.raises(FloatingPointError):
                check_lengths_status()
            assert torch.equal(got, clamped)
            with pytest.raises(FloatingPointError):
                fn(lengths=bad, check=True)
            fn(lengths=good, check=True)                                 # the word was cleared: a clean call stays clean


def _capture(launch, outs, scratch):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture: the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [x.clone() for x in outs]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for x in list(outs) + list(scratch):
            x.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outs, eager))
    return eager


@pytest.mark.parametrize("K,with_lengths", [(8, False), (24, True), (64, False)])
def test_perstep_viterbi_captured_in_a_graph_replays_the_eager_result(K, with_lengths):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import _status_word
    lib = _lib.load()
    B, T = 5, 37
    rng = np.random.default_rng(80 + K)
    init, pair, node, _ = pd.problem(B, T, K, 1, rng, False, 1.5)
    dev = torch.device("cuda")
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)      # noqa: E731
    d_init, d_pair, d_node = t(init), t(pair), t(node)
    L = np.array([T, 1, 3, T - 1, 20])
    lens = torch.tensor(L, dtype=torch.int32, device=dev) if with_lengths else None
    word = _status_word(dev) if with_lengths else None
    wsb = int(lib.svae_hmm_viterbi_workspace_bytes(B, T, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    p = _lib.ptr

    def launch():
        rc = lib.svae_hmm_perstep_viterbi_f64(B, T, K, 0, p(d_init), p(d_pair), p(d_node), p(lens), p(states), p(score),
                                              p(word), p(ws), wsb, _lib.current_stream(dev))
        assert rc == 0

    eager = _capture(launch, (states, score), (ws,))
    ref = pd.viterbi_ragged(init, pair, node, L) if with_lengths else pd.viterbi_perstep(init, pair, node)
    assert np.array_equal(_np(eager[0]), ref[0]) and np.array_equal(pd.bits(_np(eager[1])), pd.bits(ref[1]))


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def _assert_sample(case, got):
    from svae_amd.hmm.hmm_inference import hmm_logZ_perstep
    states, logZ = got
    assert case.margin >= pd.MARGIN
    assert states.shape == case.states.shape and np.array_equal(states, case.states)
    assert np.array_equal(pd.bits(logZ), pd.bits(_np(hmm_logZ_perstep(case.natparam))))    # the sweep is shared
    for b in range(len(logZ)):
        assert logZ[b] == pytest.approx(case.logZ[b], **TOL_LOG_LZ)


@pytest.mark.parametrize("K", pd.GRID_K)
def test_perstep_sample_grid_label_for_label(K):
    from svae_amd.hmm.hmm_inference import hmm_sample_perstep
    for case in pd.grid_cases(K):
        _assert_sample(case, _sample(case.natparam, case.u))
    case = pd.grid_cases(K)[-1]                                          # T = 37, B = 9, per-sequence pair parameters
    # the samples are independent chains: sample 1 of the S = 3 call is the S = 1 call on its uniforms
    one = hmm_sample_perstep(case.natparam, num_samples=1, u=case.u[:, 1:2])
    assert np.array_equal(_np(one)[:, 0], case.states[:, 1])
    # the unbatched call: (S,T) labels, a 0-d log Z, those of the batch's sequence
    st, lz = hmm_sample_perstep((case.init, case.pair[1], case.node[1]), num_samples=3, u=case.u[1], return_logZ=True)
    assert st.shape == (3, 37) and lz.shape == ()
    assert np.array_equal(_np(st), case.states[1]) and float(lz) == pytest.approx(case.logZ[1], **TOL_LOG_LZ)
    assert hmm_sample_perstep(case.natparam).shape == (9, 1, 37)         # u = None: one sample of device uniforms


@pytest.mark.parametrize("K", pd.LTR_K)
def test_perstep_sample_left_to_right_and_extreme_uniforms(K):
    case = pd.ltr_case(K)
    got = _sample(case.natparam, case.u)
    _assert_sample(case, got)
    assert (np.diff(got[0], axis=-1) >= 0).all()
    # u = 0 draws the lowest allowed state at every step, u = 1 the highest (a state is allowed if its weight is positive:
    # reachable, and its transition into the state drawn after it not forbidden)
    B, T = case.node.shape[:2]
    want_lo, want_hi, rel = pd.extreme_draws(*case.natparam)
    assert rel >= pd.MARGIN
    lo, _ = _sample(case.natparam, np.zeros((B, 1, T)))
    hi, _ = _sample(case.natparam, np.ones((B, 1, T)))
    assert np.array_equal(lo[:, 0], want_lo) and np.array_equal(hi[:, 0], want_hi)


@pytest.mark.parametrize("K", pd.PAIR_K)
def test_perstep_sample_reduces_to_the_uniform_sampler_at_constant_matrices(K):
    from svae_amd.hmm.hmm_inference import hmm_sample
    init, pair, node, u, states, logZ, margin = sm.pair_case(K)
    assert margin >= pd.MARGIN
    B, T = node.shape[:2]
    per = np.broadcast_to(pair[:, None], (B, T - 1, K, K)).copy()
    got, lz = _sample((init, per, node), u)
    assert np.array_equal(got, states)
    assert np.array_equal(got, _np(hmm_sample((init, pair, node), num_samples=u.shape[1], u=u)))
    np.testing.assert_allclose(lz, logZ, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("K", [3, 8, 16, 17, 33, 64])
def test_perstep_sample_with_lengths(K):
    from svae_amd.hmm.hmm_inference import hmm_logZ_perstep
    r = pd.ragged_case(K)
    init, pair, node, u, L = r["init"], r["pair"], r["node"], r["u"], r["L"]
    assert r["margin"] >= pd.MARGIN and r["shared"][1][2] >= pd.MARGIN
    nan_pair, nan_node, nan_u = pd.padded(pair, node, u, L)
    states, logZ = _sample((init, nan_pair, nan_node), nan_u, lengths=L, check=True)
    assert np.array_equal(states, r["states"])
    for b, l in enumerate(L):
        assert (states[b, :, l:] == -1).all()
        assert logZ[b] == pytest.approx(r["logZ"][b], **TOL_LOG_LZ)
    assert np.array_equal(pd.bits(logZ), pd.bits(_np(hmm_logZ_perstep((init, nan_pair, nan_node), lengths=L))))
    s_states, s_lz = _sample((init, pair[0], nan_node), nan_u, lengths=torch.tensor(L))
    assert np.array_equal(s_states, r["shared"][1][0])
    perm = np.random.default_rng(K).permutation(len(L))
    p_states, p_lz = _sample((init, nan_pair[perm], nan_node[perm]), nan_u[perm], lengths=L[perm])
    assert np.array_equal(p_states, states[perm]) and np.array_equal(pd.bits(p_lz), pd.bits(logZ[perm]))
    other = L.copy()
    other[1:] = other[1:][::-1]
    o_pair, o_node, o_u = pd.padded(pair, node, u, other)
    o_states, o_lz = _sample((init, o_pair, o_node), o_u, lengths=other)
    assert np.array_equal(o_states[0], states[0]) and pd.bits(o_lz[0]) == pd.bits(logZ[0])


def test_perstep_sample_statistics_from_device_uniforms():
    """the path from torch.rand to labels: 4096 draws of one sequence against the enumeration of all paths"""
    from svae_amd.hmm.hmm_inference import hmm_sample_perstep
    K, T, N = 3, 4, 4096
    rng = np.random.default_rng(77)
    init, pair, node, _ = pd.problem(1, T, K, 1, rng, False, 1.5)
    pair[1][0, 2] = -np.inf
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    states = _np(hmm_sample_perstep((init, pair, node), num_samples=N, generator=gen))
    assert states.shape == (1, N, T) and states.min() >= 0 and states.max() < K
    worst = pd.statistics_within_5_sigma(states[0], (init, pair, node[0]))
    print("worst cell: %.2f sigma" % worst)
    assert not ((states[0][:, 1] == 0) & (states[0][:, 2] == 2)).any()
    assert len({tuple(s) for s in states[0]}) > 10                       # (the samples differ: each has its own uniforms)


@pytest.mark.parametrize("K", [3, 16, 24, 64])
def test_perstep_sample_nan_potentials_stay_in_their_sequence(K):
    rng = np.random.default_rng(300 + K)
    B, T, S = 5, 17, 3
    init, pair, node, u = pd.problem(B, T, K, S, rng, True, 1.5)
    bad_pair, bad_node = pair.copy(), node.copy()
    bad_pair[2, 5] = np.nan
    bad_node[2, 9:12] = np.nan
    states, logZ = _sample((init, bad_pair, bad_node), u)
    assert states[2].min() >= 0 and states[2].max() < K
    keep = [0, 1, 3, 4]
    ref, ref_lz = _sample((init, pair[keep], node[keep]), u[keep])
    assert np.array_equal(states[keep], ref) and np.array_equal(pd.bits(logZ[keep]), pd.bits(ref_lz))
    v_lab, v_sc = _viterbi((init, bad_pair, bad_node))                   # Viterbi on the same: in range, no fault
    assert v_lab.min() >= 0 and v_lab.max() < K
    c_lab, c_sc = _viterbi((init, pair[keep], node[keep]))
    assert np.array_equal(v_lab[keep], c_lab) and np.array_equal(pd.bits(v_sc[keep]), pd.bits(c_sc))


@pytest.mark.parametrize("K,with_lengths", [(8, False), (24, True), (64, False)])
def test_perstep_sample_captured_in_a_graph_replays_the_eager_result(K, with_lengths):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import _status_word
    lib = _lib.load()
    B, T, S = 5, 37, 3
    rng = np.random.default_rng(90 + K)
    init, pair, node, u = pd.problem(B, T, K, S, rng, False, 1.5)
    dev = torch.device("cuda")
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)      # noqa: E731
    d_init, d_pair, d_node, d_u = t(init), t(pair), t(node), t(u)
    L = np.array([T, 1, 3, T - 1, 20])
    lens = torch.tensor(L, dtype=torch.int32, device=dev) if with_lengths else None
    word = _status_word(dev) if with_lengths else None
    wsb = int(lib.svae_hmm_perstep_workspace_bytes(B, T, K))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    states = torch.empty(B, S, T, dtype=torch.int32, device=dev)
    logZ = torch.empty(B, dtype=torch.float64, device=dev)
    p = _lib.ptr

    def launch():
        rc = lib.svae_hmm_perstep_sample_f64(B, T, K, S, 0, p(d_init), p(d_pair), p(d_node), p(lens), p(d_u), p(states),
                                             p(logZ), p(word), p(ws), wsb, _lib.current_stream(dev))
        assert rc == 0

    eager = _capture(launch, (states, logZ), (ws,))
    ref = pd.sample_ragged(init, pair, node, u, L) if with_lengths else pd.sample_perstep(init, pair, node, u)
    assert ref[2] >= pd.MARGIN
    assert np.array_equal(_np(eager[0]), ref[0])
    np.testing.assert_allclose(_np(eager[1]), ref[1], rtol=1e-9, atol=1e-9)
