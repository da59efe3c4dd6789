"""GPU tests of the time-chunked Viterbi decoder (svae_amd.hmm.hmm_viterbi_chunked, svae_hmm_chunked_viterbi_f64): labels
and score bit for bit the NumPy restatement of its five stages (tests/_hmm_viterbi_chunked_numpy.py) on the smallest
shapes at which the stages can go wrong; against hmm_viterbi on the same inputs (bound (c) of include/svae_hip.h); bit for
bit hmm_viterbi under exact arithmetic, -inf entries and ties included; chunk >= T is hmm_viterbi; the forms of the call;
the workspace bounds; graph capture; NaN inputs.  There is no fallback route: every result below comes from the chunked
kernels unless the test says chunk >= T."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_chunked_numpy as C  # noqa: E402
import _hmm_viterbi_chunked_numpy as VC  # noqa: E402
import _hmm_viterbi_numpy as V  # noqa: E402

CANARY = -12345.678
# PARITY_SHAPES: chunk = 2 (operators without a recursion step), a one-step last chunk ((1,7,3,2), (2,65,2,64)), K = 1 and
# K = 16, batches that leave rows of a wavefront idle (5, 9, 13), 16 chunks of 32; and more chunks than a wavefront has lanes
SHAPES = C.PARITY_SHAPES + [(1, 4097, 4, 64)]


def _np(x):
    return x.detach().cpu().numpy()


def _chunked(init, pair, node, chunk):
    """hmm_viterbi_chunked on a workspace of exactly the closed form, eight canary doubles behind it -> labels, score"""
    from svae_amd import _lib
    from svae_amd.hmm import hmm_viterbi_chunked
    B, T, K = node.shape
    need = int(_lib.load().svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, chunk))
    assert need == VC.workspace_bytes(B, T, K, chunk) and need % 8 == 0
    ws = torch.full((need // 8 + 8,), CANARY, dtype=torch.float64, device="cuda")
    labels, score = hmm_viterbi_chunked((init, pair, node), chunk=chunk, workspace=ws[:need // 8], return_score=True)
    assert labels.dtype == torch.int32 and score.dtype == torch.float64
    assert (_np(ws[need // 8:]) == CANARY).all()                       # nothing written behind the closed form
    return _np(labels), _np(score)


def _serial(init, pair, node):
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    labels, score = hmm_viterbi((init, pair, node), return_score=True)
    return _np(labels), _np(score)


@pytest.mark.parametrize("pair_batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("B,T,K,chunk", SHAPES)
def test_bit_for_bit_the_restatement_and_within_the_bound_of_the_serial_decoder(B, T, K, chunk, pair_batched):
    init, pair, node = C.parity_problem(B, T, K, chunk, pair_batched)
    labels, score = _chunked(init, pair, node, chunk)
    want, want_score = VC.chunked_viterbi_batch(init, pair, node, chunk)
    assert np.array_equal(labels, want)
    assert np.array_equal(VC.bits(score), VC.bits(want_score))
    # against hmm_viterbi on the GPU, same inputs: labels identical, score and the path's own score within bound (c)
    s_labels, s_score = _serial(init, pair, node)
    assert np.array_equal(labels, s_labels)
    for b in range(B):
        pb = pair[b] if pair_batched else pair
        bound = VC.score_bound(init, pb, node[b])
        print("b=%d |score - serial| = %.3e, |path_score - serial| = %.3e, bound %.3e"
              % (b, abs(score[b] - s_score[b]), abs(V.path_score(init, pb, node[b], labels[b]) - s_score[b]), bound))
        assert abs(score[b] - s_score[b]) <= bound
        assert abs(V.path_score(init, pb, node[b], labels[b]) - s_score[b]) <= bound


def test_exact_arithmetic_with_minus_infinity_and_ties_is_the_serial_decoder_bit_for_bit():
    ties, neg_inf, dead = 0, 0, 0
    for seed in VC.DYADIC_SEEDS:
        init, pair, node, chunk = VC.dyadic_problem(seed)
        B = node.shape[0]
        labels, score = _chunked(init, pair, node, chunk)
        s_labels, s_score = _serial(init, pair, node)
        r_labels, r_score = V.viterbi_batch(init, pair, node)
        assert np.array_equal(labels, s_labels) and np.array_equal(labels, r_labels), seed
        assert np.array_equal(VC.bits(score), VC.bits(s_score)) and np.array_equal(VC.bits(score), VC.bits(r_score)), seed
        ties += sum(VC.count_ties(init, pair[b] if pair.ndim == 3 else pair, node[b]) for b in range(B))
        neg_inf += int(np.isinf(pair).any() or np.isinf(node).any())
        dead += int((r_score == -np.inf).any())
    # the inputs do exercise ties (on average at least one tied maximum per problem), -inf entries and a dead chain
    assert ties >= len(VC.DYADIC_SEEDS) and neg_inf >= len(VC.DYADIC_SEEDS) // 3 and dead >= 1, (ties, neg_inf, dead)


@pytest.mark.parametrize("chunk", [9, 10, 1000])
def test_one_chunk_is_the_serial_decoder(chunk):
    from svae_amd.hmm import hmm_viterbi_chunked
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    init, pair, node = C.parity_problem(5, 9, 3, 3, True)
    want, want_score = hmm_viterbi((init, pair, node), return_score=True)
    got, got_score = hmm_viterbi_chunked((init, pair, node), chunk=chunk, return_score=True)
    assert torch.equal(got, want) and torch.equal(got_score.view(torch.int64), want_score.view(torch.int64))


def test_forms_of_the_call():
    from svae_amd.hmm import hmm_viterbi_chunked
    init, pair, node = C.parity_problem(1, 33, 4, 8, False)
    want, want_score = VC.chunked_viterbi(init, pair, node[0], 8)
    labels = hmm_viterbi_chunked((init, pair, node[0]), chunk=8)                      # unbatched, labels alone
    assert isinstance(labels, torch.Tensor) and labels.shape == (33,) and labels.dtype == torch.int32
    assert np.array_equal(_np(labels), want)
    labels, score = hmm_viterbi_chunked((init, pair, node[0]), chunk=8, return_score=True)
    assert labels.shape == (33,) and score.dim() == 0
    assert np.array_equal(_np(labels), want) and VC.bits(_np(score)) == VC.bits(want_score)
    labels, score = hmm_viterbi_chunked((init, pair, node), chunk=8, return_score=True)
    assert labels.shape == (1, 33) and score.shape == (1,)
    # chunk=None takes the library's pick: at T = 33 the serial route, at T = 600 whatever default_chunk says
    assert np.array_equal(_np(hmm_viterbi_chunked((init, pair, node[0]))), V.viterbi(init, pair, node[0])[0])
    init, pair, node = C.parity_problem(2, 600, 5, 32, False)
    pick = VC.default_chunk(2, 600, 5)
    labels, score = hmm_viterbi_chunked((init, pair, node), return_score=True)
    want, want_score = VC.chunked_viterbi_batch(init, pair, node, pick) if pick < 600 else V.viterbi_batch(init, pair, node)
    assert np.array_equal(_np(labels), want) and np.array_equal(VC.bits(_np(score)), VC.bits(want_score))


def test_workspace_of_exactly_the_closed_form_one_byte_fewer_and_misaligned():
    from svae_amd import _lib
    from svae_amd.hmm import hmm_viterbi_chunked
    B, T, K, chunk = 5, 9, 2, 3
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    labels, score = _chunked(init, pair, node, chunk)                  # exactly the closed form, canaries behind it
    want, want_score = VC.chunked_viterbi_batch(init, pair, node, chunk)
    assert np.array_equal(labels, want) and np.array_equal(VC.bits(score), VC.bits(want_score))
    need = int(_lib.load().svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, chunk))
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="rc=-11"):
        hmm_viterbi_chunked((init, pair, node), chunk=chunk, workspace=small)
    off = torch.empty(need + 16, dtype=torch.uint8, device="cuda")[8:]
    with pytest.raises(RuntimeError, match="rc=-12"):
        hmm_viterbi_chunked((init, pair, node), chunk=chunk, workspace=off)


def test_graph_capture_replays_the_eager_bits():
    from svae_amd import _lib
    from svae_amd.hmm import hmm_viterbi_chunked
    B, T, K, chunk = 3, 40, 8, 8
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = tuple(torch.as_tensor(np.array(x), **f64) for x in (init, pair, node))
    need = int(_lib.load().svae_hmm_chunked_viterbi_workspace_bytes(B, T, K, chunk))
    ws = torch.full((need // 8,), CANARY, **f64)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [x.clone() for x in hmm_viterbi_chunked(d, chunk=chunk, workspace=ws, return_score=True)]   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hmm_viterbi_chunked(d, chunk=chunk, workspace=ws, return_score=True)
    out[0].fill_(-7)
    out[1].fill_(CANARY)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1].view(torch.int64), eager[1].view(torch.int64))
    want, want_score = VC.chunked_viterbi_batch(init, pair, node, chunk)
    assert np.array_equal(_np(out[0]), want) and np.array_equal(VC.bits(_np(out[1])), VC.bits(want_score))


def test_nan_node_potentials_give_labels_in_range():
    from svae_amd.hmm import hmm_viterbi_chunked
    B, T, K, chunk = 2, 11, 3, 4
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    node = node.copy()
    node[0, 5, 1] = np.nan
    node[1, :, :] = np.nan
    labels = _np(hmm_viterbi_chunked((init, pair, node), chunk=chunk))
    assert labels.shape == (B, T) and ((labels >= 0) & (labels < K)).all(), labels
