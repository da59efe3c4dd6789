"""GPU tests of time-chunked HMM posterior sampling on ONE LONG sequence (T = 22 785, K = 8 and 16, S = 2): labels equal,
label for label, to a truth computed by a per-step-normalised log filter in np.longdouble
(tests/_hmm_sample_chunked_numpy.long_truth; its draw margins, 6.5e-7 and 5.2e-7, are asserted in
tests/test_hmm_sample_chunked_cpu.py), at the library's own chunk and at 256 (90 chunks, a one-step last chunk)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_sample_chunked_numpy as SC  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402


@pytest.mark.parametrize("chunk", SC.LONG_CHUNKS, ids=["default", "256"])
@pytest.mark.parametrize("B,T,K,S", SC.LONG_CASES)
def test_long_sequence_labels_are_the_long_double_truths(B, T, K, S, chunk):
    from svae_amd import _lib
    from svae_amd.hmm import hmm_sample_chunked, sample_redone_sequences
    init, pair, node, u, want, want_logZ, margin = SC.long_case(B, T, K, S)
    assert margin >= smp.MARGIN
    lib = _lib.load()
    L = chunk if chunk is not None else int(lib.svae_hmm_chunked_sample_default_chunk(B, T, K, S))
    assert 2 <= L < T                                                   # the chunked route, not the serial one
    if chunk == 256:
        assert -(-T // 256) == 90 and T - 89 * 256 == 1
    ws = torch.empty(int(lib.svae_hmm_chunked_sample_workspace_bytes(B, T, K, S, L)), dtype=torch.uint8, device="cuda")
    labels, logZ = hmm_sample_chunked((np.array(init), np.array(pair), np.array(node)), num_samples=S, u=np.array(u),
                                      chunk=chunk, workspace=ws, return_logZ=True)
    labels, logZ = labels.cpu().numpy(), logZ.cpu().numpy()
    assert not sample_redone_sequences(ws[:128 * B * T].view(torch.float64), B, T, K).cpu().numpy().any()
    assert np.array_equal(labels, want), np.argwhere(labels != want)[:5]
    assert logZ == pytest.approx(want_logZ, rel=1e-10)
