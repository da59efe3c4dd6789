"""GPU tests of time-chunked HMM posterior sampling (svae_amd.hmm.hmm_sample_chunked, svae_hmm_chunked_sample_f64): labels
equal to the log-space oracle's label for label on the smallest shapes at which the stages can go wrong (no draw left out:
tests/test_hmm_sample_chunked_cpu.py asserts every margin), equal to hmm_sample's with the same uniforms, no sequence
redone, log Z bit for bit hmm_logZ_chunked's; chunk >= T is hmm_sample; the forms of the call; the range contract on the
batches of tests/_hmm_sample_range_numpy.py; the workspace bounds; graph capture; NaN input."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_sample_chunked_numpy as SC  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402
import _hmm_sample_range_numpy as Q  # noqa: E402

CANARY = 0xA5


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _chunked(init, pair, node, u, chunk):
    """hmm_sample_chunked on a workspace of exactly the closed form, 64 canary bytes behind it
    -> labels, logZ, the (B) bool array of sequences redone in log space"""
    from svae_amd import _lib
    from svae_amd.hmm import hmm_sample_chunked, sample_redone_sequences
    B, T, K = node.shape
    S = u.shape[1]
    need = int(_lib.load().svae_hmm_chunked_sample_workspace_bytes(B, T, K, S, chunk))
    assert need == SC.workspace_bytes(B, T, K, S, chunk) and need % 16 == 0
    ws = torch.full((need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    init, pair, node, u = (np.array(x) for x in (init, pair, node, u))            # (the shared cases are read-only)
    labels, logZ = hmm_sample_chunked((init, pair, node), num_samples=S, u=u, chunk=chunk, workspace=ws[:need],
                                      return_logZ=True)
    assert labels.dtype == torch.int32 and logZ.dtype == torch.float64 and labels.shape == (B, S, T)
    assert (_np(ws[need:]) == CANARY).all()                            # nothing written behind the closed form
    redone = sample_redone_sequences(ws[:128 * B * T].view(torch.float64), B, T, K)
    return _np(labels), _np(logZ), _np(redone)


def _serial(init, pair, node, u):
    from svae_amd.hmm.hmm_inference import hmm_sample
    init, pair, node, u = (np.array(x) for x in (init, pair, node, u))
    labels, logZ = hmm_sample((init, pair, node), num_samples=u.shape[1], u=u, return_logZ=True)
    return _np(labels), _np(logZ)


@pytest.mark.parametrize("B,T,K,S,chunk,pb", SC.CASES)
def test_labels_are_the_oracles_and_the_serial_samplers(B, T, K, S, chunk, pb):
    from svae_amd.hmm import hmm_logZ_chunked
    init, pair, node, u, want, want_logZ, margin = SC.case(B, T, K, S, chunk, pb)
    assert margin >= smp.MARGIN
    labels, logZ, redone = _chunked(init, pair, node, u, chunk)
    assert np.array_equal(labels, want), np.argwhere(labels != want)[:5]
    assert not redone.any()                                            # the fallback cannot hide a wrong chunked route
    s_labels, _ = _serial(init, pair, node, u)
    assert np.array_equal(labels, s_labels)
    lz = _np(hmm_logZ_chunked((np.array(init), np.array(pair), np.array(node)), chunk=chunk))
    assert np.array_equal(_bits(logZ), _bits(lz))
    assert logZ == pytest.approx(want_logZ, rel=1e-10)
    if not pb:
        for other in (3, 2 * chunk + 1):
            if other < T:
                assert np.array_equal(_chunked(init, pair, node, u, other)[0], want), other


@pytest.mark.parametrize("B,T,K,S,chunk,pb", [SC.CASES[2], SC.CASES[5]])
def test_one_chunk_is_the_serial_sampler_bit_for_bit(B, T, K, S, chunk, pb):
    init, pair, node, u = SC.case(B, T, K, S, chunk, pb)[:4]
    s_labels, s_logZ = _serial(init, pair, node, u)
    for ch in (T, T + 5, 2 ** 31 - 1):
        labels, logZ, _ = _chunked(init, pair, node, u, ch)
        assert np.array_equal(labels, s_labels) and np.array_equal(_bits(logZ), _bits(s_logZ))


def test_determinism_and_call_forms():
    from svae_amd.hmm import hmm_sample_chunked
    B, T, K, S, chunk, pb = SC.CASES[3]
    init, pair, node, u, want = (np.array(x) for x in SC.case(B, T, K, S, chunk, pb)[:5])
    a = _chunked(init, pair, node, u, chunk)
    b = _chunked(init, pair, node, u, chunk)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    # the unbatched form
    one = hmm_sample_chunked((init, pair, node[1]), num_samples=S, u=u[1], chunk=chunk)
    assert one.shape == (S, T) and np.array_equal(_np(one), want[1])
    one, lz = hmm_sample_chunked((init, pair, node[1]), num_samples=S, u=u[1], chunk=chunk, return_logZ=True)
    assert lz.shape == () and _bits(_np(lz)) == _bits(a[1][1])
    # chunk=None: the library's pick (T < 500: the serial route), and without return_logZ / workspace / u
    got = hmm_sample_chunked((init, pair, node), num_samples=S, u=u)
    assert np.array_equal(_np(got), want)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    d1 = hmm_sample_chunked((init, pair, node), num_samples=3, generator=g, chunk=chunk)
    g.manual_seed(5)
    d2 = hmm_sample_chunked((init, pair, node), num_samples=3, generator=g, chunk=chunk)
    assert d1.shape == (B, 3, T) and torch.equal(d1, d2) and 0 <= int(d1.min()) and int(d1.max()) < K
    # a long sequence at chunk=None takes a chunk below T
    from svae_amd import _lib
    assert 2 <= _lib.load().svae_hmm_chunked_sample_default_chunk(1, 1100, 8, 17) < 1100
    i2, p2, n2, u2, w2 = SC.case(*SC.CASES[7])[:5]
    got = hmm_sample_chunked((np.array(i2), np.array(p2), np.array(n2)), num_samples=17, u=np.array(u2))
    assert np.array_equal(_np(got), w2)


@pytest.mark.parametrize("K,T,chunk", [(2, 37, 8), (8, 37, 5), (16, 13, 4), (3, 12, 2)])
def test_range_gap_batches(K, T, chunk):
    b = Q.gap_batch(K, T)
    assert b["margin"] >= smp.MARGIN
    labels, logZ, redone = _chunked(b["init"], b["pair"], b["node"], b["u"], chunk)
    assert np.array_equal(labels, b["states"]), np.argwhere(labels != b["states"])[:5]
    assert np.isfinite(logZ).all() and logZ == pytest.approx(b["logZ"], rel=1e-9)
    assert b["extreme"].any() and redone[b["extreme"]].all()


@pytest.mark.parametrize("K", [3, 8, 16])
@pytest.mark.parametrize("variant", ["shared", "batched"])
def test_range_mixed_batches(K, variant):
    """extreme rows among ordinary ones: every row the oracle's, exactly the sequences redone that the restatement flags
    -- with per-sequence matrices exactly the extreme ones; a SHARED matrix with an entry below the range puts it into
    every sequence's chunk operators, so the chunked stages flag them all --, the ordinary ones bit for bit what they are
    in a batch without the extreme rows"""
    b = Q.mixed(K, variant)
    assert b["margin"] >= smp.MARGIN
    chunk = 5
    labels, logZ, redone = _chunked(b["init"], b["pair"], b["node"], b["u"], chunk)
    assert np.array_equal(labels, b["states"])
    assert logZ == pytest.approx(b["logZ"], rel=1e-9)
    flagged = SC.chunked_sample_batch(b["init"], b["pair"], b["node"], b["u"], chunk)[2]
    assert np.array_equal(redone, flagged), (redone, flagged)
    assert redone[b["extreme"]].all()
    if variant == "batched":
        assert np.array_equal(redone, b["extreme"]), (redone, b["extreme"])
    o = b["ordinary"]
    pair = b["pair"][o] if b["pair"].ndim == 3 else b["pair"]
    l_o, z_o, r_o = _chunked(b["init"], pair, b["node"][o], b["u"][o], chunk)
    assert np.array_equal(l_o, labels[o]) and np.array_equal(_bits(z_o), _bits(logZ[o]))
    assert np.array_equal(r_o, redone[o])


def test_the_headers_example_is_redone_and_has_the_posterior_marginals():
    """include/svae_hip.h's K = 2, T = 4 example at chunk 2, S = 4096, u from a seeded generator"""
    from svae_amd import _lib
    from svae_amd.hmm import hmm_sample_chunked, sample_redone_sequences
    inf = np.inf
    init = np.zeros(2)
    pair = np.array([[0.0, -800.0], [0.0, 0.0]])
    node = np.array([[[0.0, -inf], [0.0, 0.0], [-inf, 0.0], [0.0, np.log(2.0)]]])
    S = 4096
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    ws = torch.empty(int(_lib.load().svae_hmm_chunked_sample_workspace_bytes(1, 4, 2, S, 2)), dtype=torch.uint8, device="cuda")
    states, logZ = hmm_sample_chunked((init, pair, node), num_samples=S, generator=g, chunk=2, workspace=ws, return_logZ=True)
    assert bool(sample_redone_sequences(ws[:128 * 4].view(torch.float64), 1, 4, 2)[0])
    assert float(logZ[0]) == pytest.approx(-800.0 + np.log(6.0), rel=1e-12)
    got = _np(states)[0]
    Es = np.array([[1, 0], [0.5, 0.5], [0, 1], [1 / 3, 2 / 3]])
    freq = np.stack([(got == k).mean(0) for k in range(2)], -1)
    sd = np.sqrt(Es * (1 - Es) / S)
    print("worst cell: %.2f sd" % np.nanmax(np.abs(freq - Es) / np.where(sd > 0, sd, np.nan)))
    assert (np.abs(freq - Es) <= 5 * sd).all(), (freq, Es)


def test_workspace_bounds():
    from svae_amd import _lib
    from svae_amd.hmm import hmm_sample_chunked
    B, T, K, S, chunk, pb = SC.CASES[4]
    init, pair, node, u, want = (np.array(x) for x in SC.case(B, T, K, S, chunk, pb)[:5])
    need = int(_lib.load().svae_hmm_chunked_sample_workspace_bytes(B, T, K, S, chunk))
    assert np.array_equal(_chunked(init, pair, node, u, chunk)[0], want)          # the exact size, canary intact
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="-14"):
        hmm_sample_chunked((init, pair, node), num_samples=S, u=u, chunk=chunk, workspace=ws[:need - 1])
    with pytest.raises(RuntimeError, match="-15"):
        hmm_sample_chunked((init, pair, node), num_samples=S, u=u, chunk=chunk, workspace=ws[8:need + 8])


def test_capture_and_replay_give_the_eager_bits():
    from svae_amd import _lib
    b = Q.mixed(8, "batched")                                          # a batch with redone sequences
    B, T, K = b["node"].shape
    chunk = 5
    dev = torch.device("cuda")
    t = lambda x: torch.as_tensor(np.array(x), device=dev)
    d_init, d_pair, d_node, d_u = t(b["init"]), t(b["pair"]), t(b["node"]), t(b["u"])
    lib, p = _lib.load(), _lib.ptr
    wsb = int(lib.svae_hmm_chunked_sample_workspace_bytes(B, T, K, Q.S, chunk))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = torch.zeros(B, Q.S, T, dtype=torch.int32, device=dev)
    logZ = torch.zeros(B, dtype=torch.float64, device=dev)

    def launch():
        rc = lib.svae_hmm_chunked_sample_f64(B, T, K, Q.S, 1, chunk, p(d_init), p(d_pair), p(d_node), p(d_u), p(states),
                                             p(logZ), p(ws), wsb, _lib.current_stream(dev))
        assert rc == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                      # warm-up outside the capture: the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager, eager_lz = states.clone(), logZ.clone()
    assert np.array_equal(_np(eager), b["states"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    states.zero_()
    logZ.zero_()
    ws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(states, eager) and np.array_equal(_bits(_np(logZ)), _bits(_np(eager_lz)))


def test_nan_potentials_stay_in_their_sequence():
    B, T, K, S, chunk, pb = SC.CASES[5]
    init, pair, node, u = (np.array(x) for x in SC.case(B, T, K, S, chunk, pb)[:4])
    clean, clean_lz, _ = _chunked(init, pair, node, u, chunk)
    bad = node.copy()
    bad[2, 40:45] = np.nan
    labels, logZ, _ = _chunked(init, pair, bad, u, chunk)
    assert labels[2].min() >= 0 and labels[2].max() < K
    keep = [0, 1, 3, 4]
    assert np.array_equal(labels[keep], clean[keep]) and np.array_equal(_bits(logZ[keep]), _bits(clean_lz[keep]))
