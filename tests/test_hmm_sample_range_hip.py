"""GPU tests of HMM posterior sampling where a SCALED filter loses mass while its normalisers look ordinary
(tests/_hmm_range_numpy.py: a transition more than 745 nats below the matrix' maximum, E[log pi] of a sparse Dirichlet
row, a state forbidden at the start and entered through a deep transition).  hmm_sample keeps the E-step's range
contract: such a sequence is filtered again, all of it, in log space (csrc/hmm_sample_log.hip), and
hmm_inference.sample_redone_sequences says which were.

Paths are compared label for label with the log-space oracle tests/_hmm_sample_numpy.py; every compared case has a margin
of at least 1e-8 between each draw and its nearest decision boundary (asserted in tests/test_hmm_sample_range_cpu.py,
which also shows that the sampler's arithmetic before the contract draws other paths on the gap, sparse and ramp batches).
S = 4, per-sequence transition matrices; K at the DPP-row and wide boundaries, T around the row kernels' 16-step and the
wide kernels' 8- / 64-step blocks, the first hop at every ring position."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_range_numpy as R  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402
import _hmm_sample_range_numpy as Q  # noqa: E402

LZ_REL = 1e-9           # log Z of a sequence the kernels may have redone in log space (tests/test_hmm_range_hip.py)


def _np(x):
    return x.detach().cpu().numpy()


def _sample(init, pair, node, u, lengths=None):
    """hmm_sample on a workspace of its own -> states, logZ, the (B) bool array of sequences redone in log space"""
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_sample, sample_redone_sequences
    B, T, K = node.shape
    ws = torch.empty(int(_lib.load().svae_hmm_sample_workspace_bytes(B, T, K)) // 8, dtype=torch.float64, device="cuda")
    init, pair, node, u = (np.array(x) for x in (init, pair, node, u))            # (the shared cases are read-only)
    kw = {} if lengths is None else dict(lengths=np.array(lengths), check=True)   # check: the status word is clear
    states, logZ = hmm_sample((init, pair, node), num_samples=u.shape[1], u=u, return_logZ=True, workspace=ws, **kw)
    return _np(states), _np(logZ), _np(sample_redone_sequences(ws, B, T, K))


def _check(b):
    """the batch through the kernels: every label the oracle's, log Z within 1e-9, every extreme sequence reported redone"""
    assert b["margin"] >= smp.MARGIN
    got, lz, redone = _sample(b["init"], b["pair"], b["node"], b["u"], b["lengths"])
    want = b["states"]
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    assert np.isfinite(lz).all()
    # the form of tests/test_hmm_range_hip.py (TOL_LOG): pytest.approx's absolute floor of 1e-12 stands in where log Z is
    # 0 by construction -- a K = 2 gap sequence cut before its event has log Z = log(1 + e^-g), a sum the kernels (and the
    # E-step's) form as m + log(s) of terms of magnitude 1
    assert lz == pytest.approx(b["logZ"], rel=LZ_REL), np.abs(lz - b["logZ"]).max()
    assert b["extreme"].any() and redone[b["extreme"]].all(), (redone, b["extreme"])
    return got, lz, redone


@pytest.mark.parametrize("T", R.GAP_T)
@pytest.mark.parametrize("K", Q.ALL_K)
def test_gap_cases(K, T):
    """the only way into state 1 costs g in {100 .. 3000}, at every position of the event in the kernels' rounds"""
    _check(Q.gap_batch(K, T))


@pytest.mark.parametrize("name", Q.FAMILIES)
@pytest.mark.parametrize("K", Q.FAMILY_K)
def test_surprise_sparse_and_ramp_cases(K, name):
    _check(Q.family_batch(name, K))


@pytest.mark.parametrize("K", Q.ALL_K)
def test_gap_cases_with_lengths(K):
    """the T = 37 batch cut to lengths that include 1 and 2, NaN from each length on: the paths of every cut sequence
    run alone, -1 behind them, the status word clear (check=True in _sample)"""
    b = Q.ragged_gap_batch(K)
    got, _, _ = _check(b)
    for i, L in enumerate(b["lengths"]):
        assert (got[i, :, L:] == -1).all() and got[i, :, :L].min() >= 0 and got[i, :, :L].max() < K


@pytest.mark.parametrize("variant", Q.VARIANTS)
@pytest.mark.parametrize("K", Q.ALL_K)
def test_mixed_batches(K, variant):
    """extreme rows among ordinary ones (0, 1, 2 and 4 of them in a wavefront of four rows): every row exact, the extreme
    ones redone, and the ordinary ones bit for bit what they are in a batch without the extreme rows"""
    b = Q.mixed(K, variant)
    got, lz, _ = _check(b)
    o = b["ordinary"]
    pair = b["pair"][o] if b["pair"].ndim == 3 else b["pair"]
    got_o, lz_o, redone_o = _sample(b["init"], pair, b["node"][o], b["u"][o],
                                    None if b["lengths"] is None else b["lengths"][o])
    assert np.array_equal(got_o, got[o])
    assert np.array_equal(lz_o.view(np.int64), lz[o].view(np.int64))
    assert not redone_o.any(), redone_o


@pytest.mark.parametrize("K", smp.GRID_K)
def test_ordinary_sequences_are_not_redone(K):
    """the cap on false positives: the scale-1 grid of tests/test_hmm_sample_hip.py (and its batched-pair case) stays on
    the scaled route, every sequence"""
    for T in (7, 200):
        for B in (5, 64):
            init, pair, node, u = smp.grid_case(K, T, B, 1.0)[:4]
            _, _, redone = _sample(init, pair, node, u)
            assert not redone.any(), (T, B, redone)
    if K in smp.PAIR_K:
        init, pair, node, u = smp.pair_case(K)[:4]
        _, _, redone = _sample(init, pair, node, u)
        assert not redone.any(), redone


def _header_example():
    """include/svae_hip.h, svae_hmm_sample_f64: K = 2, T = 4; the chain starts in state 0, must be in state 1 at t = 2,
    and its only way there is a transition of -800.  Posterior: z_1 (1/2, 1/2), z_3 (1/3, 2/3)."""
    inf = np.inf
    init = np.zeros(2)
    pair = np.array([[0.0, -800.0], [0.0, 0.0]])
    node = np.array([[[0.0, -inf], [0.0, 0.0], [-inf, 0.0], [0.0, np.log(2.0)]]])
    return init, pair, node


def test_the_headers_example_has_the_posterior_marginals():
    """S = 4096, u drawn on the device: every cell within 5 binomial standard deviations of hmm_estep's E_states"""
    from svae_amd.hmm.hmm_inference import hmm_estep, hmm_sample
    init, pair, node = _header_example()
    S = 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    states, logZ = hmm_sample((init, pair, node), num_samples=S, generator=g, return_logZ=True)
    _, (_, _, Es) = hmm_estep((init, pair, node))
    Es, got = _np(Es)[0], _np(states)[0]
    np.testing.assert_allclose(Es, [[1, 0], [0.5, 0.5], [0, 1], [1 / 3, 2 / 3]], atol=1e-12)
    assert float(logZ[0]) == pytest.approx(-800.0 + np.log(2.0) + np.log(3.0), rel=1e-12)
    freq = np.stack([(got == k).mean(0) for k in range(2)], -1)              # (T,K)
    sd = np.sqrt(Es * (1 - Es) / S)
    print("worst cell: %.2f sd" % np.nanmax(np.abs(freq - Es) / np.where(sd > 0, sd, np.nan)))
    assert (np.abs(freq - Es) <= 5 * sd).all(), (freq, Es)
    assert abs(freq[3, 1] - 2 / 3) <= 5 * np.sqrt(2 / 9 / S) and abs(freq[1, 0] - 0.5) <= 5 * np.sqrt(0.25 / S)


@pytest.mark.parametrize("K", [8, 33])
def test_capture_and_replay_of_a_batch_with_a_redone_sequence(K):
    """the three launches (filter, log-space filter, draw) under graph capture: the eager result"""
    from svae_amd import _lib
    b = Q.mixed(K, "batched")
    B, T, _ = b["node"].shape
    dev = torch.device("cuda")
    t = lambda x: torch.as_tensor(np.array(x), device=dev)
    d_init, d_pair, d_node, d_u = t(b["init"]), t(b["pair"]), t(b["node"]), t(b["u"])
    lib, p = _lib.load(), _lib.ptr
    wsb = int(lib.svae_hmm_sample_workspace_bytes(B, T, K))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
    states = torch.zeros(B, Q.S, T, dtype=torch.int32, device=dev)
    logZ = torch.zeros(B, dtype=torch.float64, device=dev)

    def launch():
        rc = lib.svae_hmm_sample_f64(B, T, K, Q.S, 1, p(d_init), p(d_pair), p(d_node), p(d_u), p(states), p(logZ), p(ws),
                                     wsb, _lib.current_stream(dev))
        assert rc == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture: the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager_s, eager_z = states.clone(), logZ.clone()
    assert np.array_equal(_np(eager_s), b["states"])
    states.zero_(); logZ.zero_(); ws.fill_(1.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(states, eager_s) and torch.equal(logZ, eager_z)
    from svae_amd.hmm.hmm_inference import sample_redone_sequences
    assert _np(sample_redone_sequences(ws, B, T, K))[b["extreme"]].all()
