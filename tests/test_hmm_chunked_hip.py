"""GPU tests of the time-chunked HMM E-step (svae_amd.hmm.hmm_estep_chunked / hmm_logZ_chunked,
svae_hmm_chunked_estep_f64): parity with the log-space oracle (and the reference's compiled hmm_logZ / hmm_logZ_grad) on
the smallest shapes at which the three stages can go wrong, with NO sequence on the serial fallback; chunk >= T is
hmm_estep bit for bit; determinism; the logZ-only mode; the range contract and its route words; the workspace size; graph
capture.  Inputs: tests/test_hmm_hip.py::_problem (tests/_hmm_chunked_numpy.py)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_chunked_numpy as C  # noqa: E402
from oracle import hmm_numpy, ref  # noqa: E402  (checkers only)

# sequences the serial route may have redone in log space / ordinary ones (tests/test_hmm_range_hip.py, test_hmm_hip.py)
TOL_LOG = dict(lz=dict(rel=1e-9), st=dict(rtol=1e-7, atol=1e-10), tr=dict(rtol=1e-7, atol=1e-9))
TOL_ORD = dict(lz=dict(rel=1e-10, abs=1e-10), st=dict(rtol=1e-8, atol=1e-12), tr=dict(rtol=1e-8, atol=1e-11))
CANARY = -12345.678


def _np(x):
    return x.detach().cpu().numpy()


def _ws(B, T, K, chunk, extra=0):
    from svae_amd import _lib
    need = int(_lib.load().svae_hmm_chunked_workspace_bytes(B, T, K, chunk))
    assert need > 0 and need % 8 == 0
    return torch.full((need // 8 + extra,), CANARY, dtype=torch.float64, device="cuda"), need


def _chunked(init, pair, node, chunk):
    """hmm_estep_chunked on a workspace of its own (eight canary doubles behind it) -> numpy outputs, the route words"""
    from svae_amd.hmm import hmm_estep_chunked, chunked_redone_sequences
    B, T, K = node.shape
    ws, need = _ws(B, T, K, chunk, extra=8)
    logZ, (Ei, Et, Es) = hmm_estep_chunked((init, pair, node), chunk=chunk, workspace=ws[:need // 8])
    redone = _np(chunked_redone_sequences(ws[:need // 8], B, T, K, chunk))
    assert (_np(ws[need // 8:]) == CANARY).all()                       # nothing written behind the closed form
    return (_np(logZ), _np(Ei), _np(Et), _np(Es)), redone


def _check(got, init, pair, node, tol_of, with_ref=True):
    logZ, Ei, Et, Es = got
    B, T, K = node.shape
    assert all(np.isfinite(x).all() for x in got)
    for b in range(B):
        tol = tol_of(b)
        pb = pair[b] if pair.ndim == 3 else pair
        lz, (oi, ot, os_) = hmm_numpy.hmm_estep((init, pb, node[b]))
        assert logZ[b] == pytest.approx(lz, **tol["lz"]), b
        np.testing.assert_allclose(Ei[b], oi, err_msg="E_init %d" % b, **tol["st"])
        np.testing.assert_allclose(Et[b], ot, err_msg="E_trans %d" % b, **tol["tr"])
        np.testing.assert_allclose(Es[b], os_, err_msg="E_states %d" % b, **tol["st"])
        if with_ref and ref.available():
            rz, aux = ref.hmm_logZ((init, np.array(pb), np.array(node[b])))
            gi, gp, gn = ref.hmm_logZ_grad(1.0, aux)
            assert logZ[b] == pytest.approx(rz, **tol["lz"])
            np.testing.assert_allclose(Ei[b], gi, **tol["st"])
            np.testing.assert_allclose(Et[b], gp, **tol["tr"])
            np.testing.assert_allclose(Es[b], gn, **tol["st"])
    assert np.abs(Es.sum(-1) - 1).max() < 1e-12
    assert np.abs(Et.sum((-1, -2)) - (T - 1)).max() < 1e-10 * T


@pytest.mark.parametrize("pair_batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("B,T,K,chunk", C.PARITY_SHAPES)
def test_parity_with_oracle_and_reference_without_fallback(B, T, K, chunk, pair_batched):
    init, pair, node = C.parity_problem(B, T, K, chunk, pair_batched)
    got, redone = _chunked(init, pair, node, chunk)
    # the cap on the share of redone sequences is zero: the fallback must not hide a wrong chunked route
    assert not redone.any(), redone
    _check(got, init, pair, node, lambda b: TOL_ORD)


def test_unbatched_call_and_default_chunk():
    from svae_amd.hmm import hmm_estep_chunked, hmm_logZ_chunked
    init, pair, node = C.parity_problem(1, 33, 4, 8, False)
    logZ, (Ei, Et, Es) = hmm_estep_chunked((init, pair, node[0]), chunk=8)
    assert logZ.dim() == 0 and Ei.shape == (4,) and Et.shape == (4, 4) and Es.shape == (33, 4)
    _check(tuple(_np(x)[None] for x in (logZ, Ei, Et, Es)), init, pair, node, lambda b: TOL_ORD)
    lz = hmm_logZ_chunked((init, pair, node[0]))                      # default chunk (T = 33: the serial route)
    assert lz.dim() == 0 and float(lz) == pytest.approx(float(logZ), rel=1e-12)


@pytest.mark.parametrize("chunk", [9, 10, 1000])
def test_one_chunk_is_the_serial_path(chunk):
    from svae_amd.hmm import hmm_estep_chunked, hmm_logZ_chunked
    from svae_amd.hmm.hmm_inference import hmm_estep
    init, pair, node = C.parity_problem(5, 9, 3, 3, True)
    want = hmm_estep((init, pair, node))
    got = hmm_estep_chunked((init, pair, node), chunk=chunk)
    assert torch.equal(got[0], want[0])
    for g, w in zip(got[1], want[1]):
        assert torch.equal(g, w)
    assert torch.equal(hmm_logZ_chunked((init, pair, node), chunk=chunk), want[0])


def test_two_calls_give_the_same_bits():
    init, pair, node = C.parity_problem(9, 50, 8, 7, False)
    a, _ = _chunked(init, pair, node, 7)
    b, _ = _chunked(init, pair, node, 7)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("B,T,K,chunk", [(9, 50, 8, 7), (4, 33, 16, 8), (1, 12, 1, 4)])
def test_logZ_only_mode(B, T, K, chunk):
    from svae_amd import _lib
    from svae_amd.hmm import hmm_logZ_chunked
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    (logZ, _, _, _), _ = _chunked(init, pair, node, chunk)
    assert np.array_equal(_np(hmm_logZ_chunked((init, pair, node), chunk=chunk)), logZ)
    # NULL statistics through the C entry: canary-filled buffers (the ones a full call would fill) stay untouched
    lib, p = _lib.load(), _lib.ptr
    f64 = dict(dtype=torch.float64, device="cuda")
    t = lambda x: torch.as_tensor(np.array(x), **f64)                  # noqa: E731
    d_init, d_pair, d_node = t(init), t(pair), t(node)
    out = torch.full((B + B * K + B * K * K + B * T * K + 8,), CANARY, **f64)
    ws, need = _ws(B, T, K, chunk, extra=8)
    rc = lib.svae_hmm_chunked_estep_f64(B, T, K, 0, chunk, p(d_init), p(d_pair), p(d_node), p(out), None, None, None,
                                        p(ws), need, _lib.current_stream(torch.device("cuda")))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(out[:B]), logZ)
    assert (_np(out[B:]) == CANARY).all() and (_np(ws[need // 8:]) == CANARY).all()


def test_range_contract_and_route_words():
    init, pair, node, hostile = C.range_batch()
    B = node.shape[0]
    got, redone = _chunked(init, pair, node, 8)
    assert (redone == hostile).all(), (redone, hostile)
    _check(got, init, pair, node, lambda b: TOL_LOG if hostile[b] else TOL_ORD, with_ref=False)
    # no sequence is affected by its neighbour's route: the benign ones alone give the same bits
    keep = np.flatnonzero(~hostile)
    alone, redone_alone = _chunked(init, pair[keep], node[keep], 8)
    assert not redone_alone.any()
    for x, y in zip(got, alone):
        assert np.array_equal(x[keep], y)
    # ... and so does the logZ-only mode, whose recompute writes its statistics into the workspace
    from svae_amd.hmm import hmm_logZ_chunked
    assert np.array_equal(_np(hmm_logZ_chunked((init, pair, node), chunk=8)), got[0])


def test_workspace_of_exactly_the_closed_form_and_one_byte_fewer():
    from svae_amd import _lib
    from svae_amd.hmm import hmm_estep_chunked
    B, T, K, chunk = 5, 9, 2, 3
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    got, redone = _chunked(init, pair, node, chunk)                    # exactly svae_hmm_chunked_workspace_bytes
    assert not redone.any()
    _check(got, init, pair, node, lambda b: TOL_ORD)
    need = int(_lib.load().svae_hmm_chunked_workspace_bytes(B, T, K, chunk))
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="rc=-12"):
        hmm_estep_chunked((init, pair, node), chunk=chunk, workspace=small)
    # the C entry: nothing launched, the outputs untouched
    lib, p = _lib.load(), _lib.ptr
    f64 = dict(dtype=torch.float64, device="cuda")
    t = lambda x: torch.as_tensor(np.array(x), **f64)                  # noqa: E731
    d_init, d_pair, d_node = t(init), t(pair), t(node)
    outs = [torch.full(s, CANARY, **f64) for s in ((B,), (B, K), (B, K, K), (B, T, K))]
    ws = torch.full((need // 8,), CANARY, **f64)
    rc = lib.svae_hmm_chunked_estep_f64(B, T, K, 0, chunk, p(d_init), p(d_pair), p(d_node), *map(p, outs), p(ws), need - 1,
                                        _lib.current_stream(torch.device("cuda")))
    assert rc == -12
    torch.cuda.synchronize()
    assert all((_np(x) == CANARY).all() for x in outs + [ws])


def test_graph_capture_replays_the_eager_bits():
    from svae_amd.hmm import hmm_estep_chunked
    B, T, K, chunk = 3, 40, 8, 8
    init, pair, node = C.parity_problem(B, T, K, chunk, False)
    f64 = dict(dtype=torch.float64, device="cuda")
    d = tuple(torch.as_tensor(np.array(x), **f64) for x in (init, pair, node))
    ws, need = _ws(B, T, K, chunk)

    def flat(out):
        return [out[0], *out[1]]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [x.clone() for x in flat(hmm_estep_chunked(d, chunk=chunk, workspace=ws))]     # warm-up = the eager result
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = flat(hmm_estep_chunked(d, chunk=chunk, workspace=ws))
    for x in out:
        x.fill_(CANARY)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(out, eager):
        assert torch.equal(x, y)
    _check(tuple(_np(x) for x in out), init, pair, node, lambda b: TOL_ORD)
