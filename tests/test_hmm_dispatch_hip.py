"""GPU test of EVERY slot of the HMM entry points' K dispatch (csrc/hmm_units.hpp): the row kernels K = 1 .. 16, both
edges of the two wide kernels (17, 32, 33, 64), and for the per-step entries both edges of their lane groups (8, 9, 16, 17,
32, 33, 64).  A table with a missing or shifted entry fails at exactly one K, and the other GPU files sample K.  Every
entry is called once uniform (shared pair parameters) and once with per-sequence lengths, one of them 1 (per-sequence pair
parameters, node potentials NaN from the length on), on B = 5 sequences -- not a multiple of the four rows of a wavefront
-- of T = 4 steps.

References and tolerances are those of the entry's own GPU file: oracle/hmm_numpy.py at TOL of tests/test_hmm_hip.py,
tests/_hmm_viterbi_numpy.py bit for bit, tests/_hmm_sample_numpy.py label for label (margins >= 1e-8 asserted) with logZ
at rtol 1e-10, tests/_hmm_vjp_numpy.py at ORD of tests/test_hmm_estep_vjp_hip.py; per step tests/_hmm_perstep_numpy.py
at TOL_LOG of tests/test_hmm_perstep_hip.py, tests/_hmm_perstep_decode_numpy.py bit for bit / label for label with logZ at
TOL_LOG, tests/_hmm_perstep_vjp_numpy.py at RTOL, ATOL of tests/test_hmm_perstep_vjp_hip.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_perstep_decode_numpy as pd  # noqa: E402
import _hmm_perstep_numpy as ps  # noqa: E402
import _hmm_perstep_vjp_numpy as pvjp  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402
import _hmm_viterbi_numpy as vit  # noqa: E402
import _hmm_vjp_numpy as vjp  # noqa: E402
from oracle import hmm_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

KS = tuple(range(1, 17)) + (17, 32, 33, 64)
GROUP_KS = (8, 9, 16, 17, 32, 33, 64)
B, T, S = 5, 4, 2
LENGTHS = (4, 1, 3, 2, 4)
TOL = dict(lz=dict(rel=1e-10, abs=1e-10), st=dict(rtol=1e-8, atol=1e-12), tr=dict(rtol=1e-8, atol=1e-11))
TOL_LOG = dict(lz=dict(rel=1e-9, abs=1e-9), st=dict(rtol=1e-7, atol=1e-10), tr=dict(rtol=1e-7, atol=1e-9))
VJP_ORD = (1e-8, 1e-11)
PERSTEP_VJP = (1e-7, 1e-9)


def _np(x):
    return x.detach().cpu().numpy()


def _dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.float64, device="cuda")


def _padded(x, lengths, first=0):
    """a copy with sequence b's steps from lengths[b] - first on replaced by NaN"""
    out = np.array(x, dtype=np.float64)
    for b, L in enumerate(lengths):
        out[b, L - first:] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def _problem(K):
    """the potentials of tests/test_hmm_hip.py::_problem with shared and with per-sequence pair parameters, uniforms and
    all four cotangents; read-only"""
    rng = np.random.default_rng(4100 + K)
    init = np.log(rng.dirichlet(np.ones(K)))
    pairs = np.log(rng.dirichlet(np.ones(K), size=(B + 1, K))) + 0.3 * rng.standard_normal((B + 1, K, K))
    p = dict(init=init, pair=pairs[0], pairs=pairs[1:], node=rng.standard_normal((B, T, K)), u=rng.random((B, S, T)),
             g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, K, K)),
             W=rng.standard_normal((B, T, K)))
    for x in p.values():
        x.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _perstep_problem(K):
    """the potentials of tests/test_hmm_perstep_hip.py::_problem (every step's matrix at its own offset), likewise"""
    rng = np.random.default_rng(4200 + K)
    init = np.log(rng.dirichlet(np.ones(K)))
    pairs = np.log(rng.dirichlet(np.ones(K), size=(B + 1, T - 1, K))) + 0.5 * rng.standard_normal((B + 1, T - 1, K, K))
    pairs = pairs + 3.0 * rng.standard_normal((B + 1, T - 1, 1, 1))
    p = dict(init=init, pair=pairs[0], pairs=pairs[1:], node=1.5 * rng.standard_normal((B, T, K)), u=rng.random((B, S, T)),
             g=rng.standard_normal(B), u0=rng.standard_normal((B, K)), V=rng.standard_normal((B, T - 1, K, K)),
             W=rng.standard_normal((B, T, K)))
    for x in p.values():
        x.setflags(write=False)
    return p


def _calls(p, perstep=False):
    """the two calls of every test: (natparam, lengths, the potentials its reference is computed from)"""
    ragged_pair = _padded(p["pairs"], LENGTHS, first=1) if perstep else p["pairs"]
    return (((p["init"], p["pair"], p["node"]), None, (p["pair"], (T,) * B)),
            ((p["init"], ragged_pair, _padded(p["node"], LENGTHS)), np.array(LENGTHS), (p["pairs"], LENGTHS)))


# ---- one transition matrix per sequence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_estep_at_every_K(K):
    from svae_amd.hmm.hmm_inference import hmm_estep
    p = _problem(K)
    for nat, lengths, (pair, Ls) in _calls(p):
        logZ, (Ei, Et, Es) = (hmm_estep(nat) if lengths is None else hmm_estep(nat, lengths=lengths, check=True))
        logZ, Ei, Et, Es = _np(logZ), _np(Ei), _np(Et), _np(Es)
        assert logZ.shape == (B,) and Ei.shape == (B, K) and Et.shape == (B, K, K) and Es.shape == (B, T, K)
        for b, L in enumerate(Ls):
            lz, (oi, ot, os_) = hmm_numpy.hmm_estep((p["init"], pair[b] if pair.ndim == 3 else pair, p["node"][b, :L]))
            assert logZ[b] == pytest.approx(lz, **TOL["lz"]), (K, b)
            np.testing.assert_allclose(Ei[b], oi, **TOL["st"])
            np.testing.assert_allclose(Et[b], ot, **TOL["tr"])
            np.testing.assert_allclose(Es[b, :L], os_, **TOL["st"])
            assert (Es[b, L:] == 0.0).all()


@pytest.mark.parametrize("K", KS)
def test_viterbi_at_every_K(K):
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    p = _problem(K)
    for nat, lengths, (pair, Ls) in _calls(p):
        states, score = hmm_viterbi(nat, return_score=True, lengths=lengths, check=lengths is not None)
        states, score = _np(states), _np(score)
        assert states.shape == (B, T) and states.dtype == np.int32 and score.shape == (B,)
        for b, L in enumerate(Ls):
            lab, sc = vit.viterbi(p["init"], pair[b] if pair.ndim == 3 else pair, p["node"][b, :L])
            assert np.array_equal(states[b, :L], lab) and (states[b, L:] == -1).all(), (K, b)
            assert vit.bits(score[b]) == vit.bits(sc), (K, b)


@pytest.mark.parametrize("K", KS)
def test_sample_at_every_K(K):
    from svae_amd.hmm.hmm_inference import hmm_sample
    p = _problem(K)
    for nat, lengths, (pair, Ls) in _calls(p):
        want, want_lz, margin = smp.sample_ragged(p["init"], np.broadcast_to(pair, (B, K, K)), p["node"], p["u"], Ls)
        assert margin >= smp.MARGIN, (K, margin)
        states, logZ = hmm_sample(nat, num_samples=S, u=p["u"], return_logZ=True, lengths=lengths,
                                  check=lengths is not None)
        assert states.dtype == torch.int32 and np.array_equal(_np(states), want), K
        np.testing.assert_allclose(_np(logZ), want_lz, rtol=1e-10, atol=0)


def _within(got, want, scales, tol, what):
    rt, at = tol
    for name, a, b in zip(("d_init", "d_pair", "d_node"), got, want):
        assert a.shape == b.shape and np.isfinite(a).all(), (what, name)
        for s in range(B):
            err = np.abs(a[s] - b[s])
            assert (err <= rt * np.abs(b[s]) + at * scales[s]).all(), (what, name, s, float(err.max()), float(scales[s]))


@pytest.mark.parametrize("K", KS)
def test_estep_vjp_at_every_K(K):
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_estep_vjp, vjp_redone_sequences
    p = _problem(K)
    cot = {k: p[k] for k in ("g", "u0", "V", "W")}
    ws = torch.empty(int(_lib.load().svae_hmm_estep_vjp_workspace_bytes(B, T, K)) // 8, dtype=torch.float64, device="cuda")
    for nat, lengths, (pair, Ls) in _calls(p):
        got = hmm_estep_vjp(tuple(_dev(x) for x in nat), (_dev(cot["g"]), (_dev(cot["u0"]), _dev(cot["V"]), _dev(cot["W"]))),
                            workspace=ws, lengths=lengths, check=lengths is not None)
        assert not _np(vjp_redone_sequences(ws, B, T, K)).any(), K          # ordinary potentials: the scaled kernels
        want = vjp.estep_vjp_batch(p["init"], pair, p["node"], lengths=Ls, **cot)
        scales = [vjp.scale(cot["g"][b], cot["u0"][b], cot["V"][b], cot["W"][b, :L], L) for b, L in enumerate(Ls)]
        _within([_np(x) for x in got], want, scales, VJP_ORD, (K, lengths is not None))
        assert all((_np(got[2])[b, L:] == 0.0).all() for b, L in enumerate(Ls))


# ---- per-step transition matrices: the edges of the lane groups ---------------------------------------------------------------
@pytest.mark.parametrize("K", GROUP_KS)
def test_perstep_estep_at_the_group_edges(K):
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep
    p = _perstep_problem(K)
    for nat, lengths, (pair, Ls) in _calls(p, perstep=True):
        logZ, (Ei, Et, Es) = hmm_estep_perstep(nat, lengths=lengths, check=lengths is not None)
        logZ, Ei, Et, Es = _np(logZ), _np(Ei), _np(Et), _np(Es)
        assert logZ.shape == (B,) and Ei.shape == (B, K) and Et.shape == (B, T - 1, K, K) and Es.shape == (B, T, K)
        for b, L in enumerate(Ls):
            pb = pair[b] if pair.ndim == 4 else pair
            lz, (oi, ot, os_) = ps.hmm_estep_perstep((p["init"], pb[:L - 1], p["node"][b, :L]))
            assert logZ[b] == pytest.approx(lz, **TOL_LOG["lz"]), (K, b)
            np.testing.assert_allclose(Ei[b], oi, **TOL_LOG["st"])
            np.testing.assert_allclose(Es[b, :L], os_, **TOL_LOG["st"])
            np.testing.assert_allclose(Et[b, :L - 1], ot, **TOL_LOG["tr"])
            assert (Es[b, L:] == 0.0).all() and (Et[b, L - 1:] == 0.0).all()


@pytest.mark.parametrize("K", GROUP_KS)
def test_perstep_viterbi_at_the_group_edges(K):
    from svae_amd.hmm.hmm_inference import hmm_viterbi_perstep
    p = _perstep_problem(K)
    for nat, lengths, (pair, Ls) in _calls(p, perstep=True):
        want, want_score = pd.viterbi_ragged(p["init"], pair, p["node"], Ls)
        states, score = hmm_viterbi_perstep(nat, return_score=True, lengths=lengths, check=lengths is not None)
        assert states.dtype == torch.int32 and np.array_equal(_np(states), want), K
        assert np.array_equal(pd.bits(_np(score)), pd.bits(want_score)), K


@pytest.mark.parametrize("K", GROUP_KS)
def test_perstep_sample_at_the_group_edges(K):
    from svae_amd.hmm.hmm_inference import hmm_sample_perstep
    p = _perstep_problem(K)
    for nat, lengths, (pair, Ls) in _calls(p, perstep=True):
        want, want_lz, margin = pd.sample_ragged(p["init"], pair, p["node"], p["u"], Ls)
        assert margin >= pd.MARGIN, (K, margin)
        states, logZ = hmm_sample_perstep(nat, num_samples=S, u=p["u"], return_logZ=True, lengths=lengths,
                                          check=lengths is not None)
        assert states.dtype == torch.int32 and np.array_equal(_np(states), want), K
        for b in range(B):
            assert _np(logZ)[b] == pytest.approx(want_lz[b], **TOL_LOG["lz"]), (K, b)


@pytest.mark.parametrize("K", GROUP_KS)
def test_perstep_estep_vjp_at_the_group_edges(K):
    from svae_amd.hmm.hmm_inference import hmm_estep_perstep_vjp
    p = _perstep_problem(K)
    cot = {k: p[k] for k in ("g", "u0", "V", "W")}
    for nat, lengths, (pair, Ls) in _calls(p, perstep=True):
        got = hmm_estep_perstep_vjp(tuple(_dev(x) for x in nat),
                                    (_dev(cot["g"]), (_dev(cot["u0"]), _dev(cot["V"]), _dev(cot["W"]))),
                                    lengths=lengths, check=lengths is not None)
        want = pvjp.estep_perstep_vjp_batch(p["init"], pair, p["node"], lengths=Ls, **cot)
        scales = [pvjp.scale(cot["g"][b], cot["u0"][b], cot["V"][b, :L - 1], cot["W"][b, :L], L) for b, L in enumerate(Ls)]
        _within([_np(x) for x in got], want, scales, PERSTEP_VJP, (K, lengths is not None))
        assert all((_np(got[2])[b, L:] == 0.0).all() and (_np(got[1])[b, L - 1:] == 0.0).all() for b, L in enumerate(Ls))
