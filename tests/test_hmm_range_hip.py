"""GPU tests of the HMM kernels where a SCALED recursion loses mass while its normalisers look ordinary
(tests/_hmm_range_numpy.py: a transition more than 745 nats below the matrix' maximum, a message component below 1e-308
of a step's total, the two-ended kernel's unnormalised steps).  Every family, every K of the DPP-row kernels and of the
wide kernel, uniform and with lengths=, against the log-space oracle (oracle/hmm_numpy.hmm_estep, itself checked against a
60-digit restatement in tests/test_hmm_range_cpu.py) at the tolerances the project applies to sequences it redoes in log
space (test_hmm_hip.py::test_hmm_forced_transition_through_a_tiny_entry); which route a sequence took is asserted from
the REDO words of the workspace (hmm_inference.redone_sequences).

Not here: hmm_sample.  Its filter has the same hole (SMP_TINY) and is left as it is, with its range tests, for a change of
its own."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hmm_range_numpy as R  # noqa: E402
import _hmm_viterbi_numpy as vit  # noqa: E402
from oracle import ref  # noqa: E402  (checker only)

ALL_K = R.K_ROW + R.K_WIDE
# sequences the kernels may have redone in log space / ordinary ones (tests/test_hmm_hip.py)
TOL_LOG = dict(lz=dict(rel=1e-9), st=dict(rtol=1e-7, atol=1e-10), tr=dict(rtol=1e-7, atol=1e-9))
TOL_ORD = dict(lz=dict(rel=1e-10, abs=1e-10), st=dict(rtol=1e-8, atol=1e-12), tr=dict(rtol=1e-8, atol=1e-11))


def _np(x):
    return x.detach().cpu().numpy()


def _estep(init, pair, node, lengths=None):
    """hmm_estep on a workspace of its own -> numpy outputs and the (B) bool array of sequences redone in log space"""
    from svae_amd import _lib
    from svae_amd.hmm.hmm_inference import hmm_estep, redone_sequences
    B, T, K = node.shape
    ws = torch.empty(int(_lib.load().svae_hmm_workspace_bytes(B, T, K)) // 8, dtype=torch.float64, device="cuda")
    init, pair, node = (np.array(x) for x in (init, pair, node))          # (the shared cases are read-only)
    logZ, (Ei, Et, Es) = hmm_estep((init, pair, node), workspace=ws, lengths=None if lengths is None else np.array(lengths))
    return (_np(logZ), _np(Ei), _np(Et), _np(Es)), _np(redone_sequences(ws, B, T, K))


def _check(got, refs, lengths=None, ordinary=(), with_ref=None):
    """every sequence against its reference (cut to its length); finite; marginals sum to 1, transition counts to L-1"""
    logZ, Ei, Et, Es = got
    for b, (lz, (oi, ot, os_)) in enumerate(refs):
        tol = TOL_ORD if b in ordinary else TOL_LOG
        L = os_.shape[0]
        assert lengths is None or L == lengths[b]
        assert np.isfinite(lz) and logZ[b] == pytest.approx(lz, **tol["lz"]), b
        np.testing.assert_allclose(Ei[b], oi, err_msg="E_init %d" % b, **tol["st"])
        np.testing.assert_allclose(Et[b], ot, err_msg="E_trans %d" % b, **tol["tr"])
        np.testing.assert_allclose(Es[b, :L], os_, err_msg="E_states %d" % b, **tol["st"])
        assert (Es[b, L:] == 0.0).all()
        assert np.abs(Es[b, :L].sum(-1) - 1).max() < 1e-12, b
        assert abs(Et[b].sum() - (L - 1)) < 1e-10 * max(1, L), b
        if with_ref is not None and ref.available():
            init, pair, node = with_ref
            natparam = tuple(np.array(x) for x in (init, pair[b] if pair.ndim == 3 else pair, node[b, :L]))
            rz, aux = ref.hmm_logZ(natparam)
            gi, gp, gn = ref.hmm_logZ_grad(1.0, aux)
            assert logZ[b] == pytest.approx(rz, **tol["lz"])
            np.testing.assert_allclose(Ei[b], gi, **tol["st"])
            np.testing.assert_allclose(Et[b], gp, **tol["tr"])
            np.testing.assert_allclose(Es[b, :L], gn, **tol["st"])
    assert all(np.isfinite(x).all() for x in got)


def _cut_refs(init, pair, node, lengths):
    refs = [R._oracle(init, pair[b] if pair.ndim == 3 else pair, node[b, :L]) for b, L in enumerate(lengths)]
    extreme = np.array([R.beyond_range(init, pair[b] if pair.ndim == 3 else pair, node[b, :L], refs[b])
                        for b, L in enumerate(lengths)])
    return refs, extreme


def _padded(node, lengths):
    out = np.array(node)
    for b, L in enumerate(lengths):
        out[b, L:] = np.nan
    return out


def _uniform_and_ragged(keys, seed, expect_extreme=True):
    """the batch of `keys`: the uniform call, then the same batch with lengths= (NaN from each length on).  Redone must
    be: every case that is extreme by construction; for K <= 16 also every case on which the uniform call's two-ended
    schedule (renormalisation every fourth step) is off; with lengths=, every cut sequence that is R.beyond_range"""
    init, pair, node, refs, extreme = R.stack(keys)
    B, T, K = node.shape
    if K <= 16:
        extreme = extreme | np.array([R.four_step_off(init, pair[b], node[b], refs[b]) for b in range(B)])
    assert extreme.any() or not expect_extreme
    got, redone = _estep(init, pair, node)
    _check(got, refs, with_ref=(init, pair, node))
    assert redone[extreme].all(), (redone, extreme)
    lengths = R.ragged_lengths(B, T, seed)
    refs_c, extreme_c = _cut_refs(init, pair, node, lengths)
    assert extreme_c.any() or not expect_extreme
    got, redone = _estep(init, pair, _padded(node, lengths), lengths=lengths)
    _check(got, refs_c, lengths=lengths)
    assert redone[extreme_c].all(), (redone, extreme_c)


# ---- E-step: every family, every K, uniform and ragged -------------------------------------------------------------------
@pytest.mark.parametrize("half", ["g <= 600", "g >= 700"])
@pytest.mark.parametrize("T", R.GAP_T)
@pytest.mark.parametrize("K", ALL_K)
def test_gap_cases(K, T, half):
    """the only way into state 1 costs g in {100 .. 3000}, at every position of the event in the kernels' rounds of eight
    steps: g >= 745 is exactly 0 (or a denormal) in a scaled transition matrix, g <= 700 is within its range"""
    g_set = R.GAP_G[:6] if half == "g <= 600" else R.GAP_G[6:]
    _uniform_and_ragged(R.gap_keys(K, T, g_set), seed=K + T, expect_extreme=half == "g >= 700")


@pytest.mark.parametrize("K", [k for k in ALL_K if k >= 3])
def test_surprise_cases(K):
    """r steps that shrink an unnormalised message by e^-s each, on top of a component at e^-g: no transition is deep, but
    g + s = 740 is beyond any scaled step, and g + r s beyond one that renormalises every fourth step only"""
    _uniform_and_ragged(R.surprise_keys(K), seed=K)


@pytest.mark.parametrize("K", ALL_K)
def test_sparse_dirichlet_cases(K):
    """transitions E[log pi] of a sparse Dirichlet row, down to psi(5e-4) - psi(50) = -2004, crossed where the evidence hops"""
    _uniform_and_ragged(R.sparse_keys(K), seed=K)


@pytest.mark.parametrize("K", ALL_K)
def test_ramp_cases(K):
    """the evidence for the state behind the -g transition arrives at 50 (200) nats per step: no single step is surprising"""
    _uniform_and_ragged(R.ramp_keys(K), seed=K)


@pytest.mark.parametrize("variant", ["shared", "shared4", "batched", "ragged"])
@pytest.mark.parametrize("K", ALL_K)
def test_mixed_batches(K, variant):
    """extreme rows among ordinary ones (0, 1, 2 and 4 of them in a wavefront of four rows): the extreme ones are redone
    and right, the ordinary ones keep the scaled pass (not redone) and its tolerances"""
    m = R.mixed_batch(K, variant)
    B = m["node"].shape[0]
    got, redone = _estep(m["init"], m["pair"], m["node"], lengths=m["lengths"])
    ordinary = [b for b in range(B) if b not in m["ext"]]
    _check(got, m["refs"], lengths=m["lengths"], ordinary=ordinary,
           with_ref=None if m["lengths"] is not None else (m["init"], m["pair"], m["node"]))
    assert m["extreme"].any() and redone[m["extreme"]].all(), (redone, m["extreme"])
    assert not redone[ordinary].any(), (redone, ordinary)


# ---- the SLDS sweep's fused route: node potentials built inside the kernel ------------------------------------------------
def _fused(K, init, pair, node):
    """svae_slds_hmm_meanfield_f64 with node_params = NULL on potentials that reproduce `node` (node[:, 0] = 0):
    pair_contr[b,t,1,k] = node[b,t,k], everything else 0; the rows listed backwards, one unused row, a trailing -1 slot"""
    from svae_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    B, T, _ = node.shape
    rows, n = B + 1, 1
    f64 = dict(dtype=torch.float64, device="cuda")
    t = lambda x: torch.as_tensor(np.array(x), **f64)                     # (a copy: the shared cases are read-only)
    pc = np.zeros((rows, T, 2, K))
    pc[:B, 1:, 1, :] = node[:, 1:]
    idx = torch.tensor(list(range(B - 1, -1, -1)) + [-1], dtype=torch.int32, device="cuda")
    zeros = lambda *s: torch.zeros(*s, **f64)
    nan = lambda *s: torch.full(s, float("nan"), **f64)
    logZ, Ei, Et, Es, nout = nan(rows), nan(rows, K), nan(rows, K, K), nan(rows, T, K), nan(rows, T, K)
    wsb = int(lib.svae_hmm_workspace_bytes(rows, T, K))
    ws = torch.empty(wsb // 8, **f64)
    pc_d, init_d, pair_d = t(pc), t(init), t(pair)
    ei, iJ, ih, ci, lz = zeros(rows, n * n + n), zeros(K, n, n), zeros(K, n), zeros(K), zeros(K)
    rc = lib.svae_slds_hmm_meanfield_f64(B + 1, rows, T, K, n, p(init_d), p(pair_d), None, p(pc_d), p(ei), p(iJ), p(ih),
                                         p(ci), p(lz), p(idx), p(logZ), p(Ei), p(Et), p(Es), p(nout), p(ws), wsb,
                                         _lib.current_stream(torch.device("cuda")))
    _lib.check(rc, "svae_slds_hmm_meanfield_f64")
    from svae_amd.hmm.hmm_inference import redone_sequences
    return tuple(_np(x) for x in (logZ, Ei, Et, Es, nout)), _np(redone_sequences(ws, rows, T, K))


@pytest.mark.parametrize("family", ["gap", "sparse"])
@pytest.mark.parametrize("K", [3, 8, 16])
def test_fused_route_sees_the_same_cases(K, family):
    """the FUSED instantiation (potentials from the LDS contractions, indexed rows) on gap_case (g = 800, T = 12, nine event
    starts) and sparse_case (conc = 1e-3, five seeds) -- the unused slot shares a wavefront with a live row --: the outputs of hmm_estep on the same potentials, and the
    oracle's; the row no slot lists stays untouched"""
    if family == "gap":
        keys = [("gap", K, 800.0, t0, 12) for t0 in range(1, 10)]
    else:
        keys = [("sparse", K, 1e-3, 200.0, 8, 24, seed) for seed in range(5)]
    init, pairs, node, refs, extreme = R.stack(keys)
    assert extreme.all() and (node[:, 0] == 0).all()
    B = node.shape[0]
    (logZ, Ei, Et, Es, nout), redone = _fused(K, init, pairs[0], node)
    assert redone[:B].all()
    _check((logZ[:B], Ei[:B], Et[:B], Es[:B]), refs)
    np.testing.assert_array_equal(nout[:B], node)
    want, _ = _estep(init, pairs[0], node)
    for g, w, tol in zip((logZ, Ei, Et, Es), want, ("lz", "st", "tr", "st")):
        if tol == "lz":
            np.testing.assert_allclose(g[:B], w, rtol=1e-9, atol=0)
        else:
            np.testing.assert_allclose(g[:B], w, **TOL_LOG[tol])
    assert all(np.isnan(x[B]).all() for x in (logZ, Ei, Et, Es, nout))


# ---- gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("gap", 8, 800.0, 5, 12), ("sparse", 9, 5e-4, 400.0, 8, 24, 1)])
def test_gradient_of_logZ_on_extreme_cases(key):
    from svae_amd.hmm.hmm_inference import hmm_logZ_differentiable
    init, pair, node = (np.array(x) for x in R.case(*key))
    lz, (_, _, os_) = R.reference(*key)
    x = torch.tensor(node, dtype=torch.float64, device="cuda", requires_grad=True)
    out = hmm_logZ_differentiable((init, pair, x))
    out.backward()
    assert float(out.detach()) == pytest.approx(lz, **TOL_LOG["lz"])
    g = _np(x.grad)
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g, os_, **TOL_LOG["st"])


# ---- Viterbi: log space already, a regression guard -------------------------------------------------------------------------
def _viterbi_and_marginals(init, pair, node, lengths=None):
    """hmm_viterbi against the restatement, bit for bit (with lengths=: on every sequence cut to its length, labels -1
    behind it); where the KERNELS' marginals are deterministic (every row has an entry > 1 - 1e-9) their argmax is the
    kernels' path.  -> the number of such sequences"""
    from svae_amd.hmm.hmm_inference import hmm_viterbi
    init, pair, node = (np.array(x) for x in (init, pair, node))
    B, T, K = node.shape
    labels, score = hmm_viterbi((init, pair, node), return_score=True, lengths=None if lengths is None else np.array(lengths))
    labels, score = _np(labels), _np(score)
    (_, _, _, Es), _ = _estep(init, pair, node, lengths=lengths)
    n_det = 0
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        want_l, want_s = vit.viterbi_batch(init, pair[b] if pair.ndim == 3 else pair, node[b:b + 1, :L])
        assert np.array_equal(labels[b, :L], want_l[0]) and (labels[b, L:] == -1).all(), b
        assert vit.bits(score[b]) == vit.bits(want_s[0]), b
        if R.deterministic(Es[b, :L]):
            n_det += 1
            assert np.array_equal(Es[b, :L].argmax(-1), labels[b, :L]), b
    return n_det


@pytest.mark.parametrize("K,family", [(K, f) for K in ALL_K for f in ("gap", "surprise", "sparse", "ramp")
                                      if K >= 3 or f != "surprise"])
def test_viterbi_on_the_same_cases(K, family):
    """every case of the family (gap: every T, g and event start), uniform and with lengths=.  (Only the sparse family has
    deterministic posteriors -- the others spread their switch over several steps --, so only there must the argmax
    comparison have fired.)"""
    if family == "gap":
        batches = [R.gap_keys(K, T, g_set) for T in R.GAP_T for g_set in (R.GAP_G[:6], R.GAP_G[6:])]
    else:
        batches = [{"surprise": R.surprise_keys, "sparse": R.sparse_keys, "ramp": R.ramp_keys}[family](K)]
    n_det = 0
    for keys in batches:
        init, pair, node, _, _ = R.stack(keys)
        B, T, _ = node.shape
        n_det += _viterbi_and_marginals(init, pair, node)
        lengths = R.ragged_lengths(B, T, K)
        n_det += _viterbi_and_marginals(init, pair, _padded(node, lengths), lengths=lengths)
    assert n_det > 0 or family != "sparse"


@pytest.mark.parametrize("variant", ["shared", "shared4", "batched", "ragged"])
@pytest.mark.parametrize("K", ALL_K)
def test_viterbi_on_the_mixed_batches(K, variant):
    m = R.mixed_batch(K, variant)
    assert _viterbi_and_marginals(m["init"], m["pair"], m["node"], lengths=m["lengths"]) > 0


# ---- which route ran -------------------------------------------------------------------------------------------------------
ORDINARY_SHAPES = [(5, 7, 3, 1.0), (9, 50, 8, 3.0), (3, 1, 4, 1.0), (4, 33, 16, 1.0), (1, 12, 1, 2.0), (6, 2, 5, 1.0),
                   (7, 3, 9, 2.0), (13, 17, 8, 1.0), (3, 25, 12, 1.0), (5, 7, 17, 1.0), (3, 50, 20, 3.0), (2, 120, 32, 2.0),
                   (4, 9, 33, 1.0), (3, 1, 40, 1.0), (2, 2, 64, 1.0)]


@pytest.mark.parametrize("B,T,K,scale", ORDINARY_SHAPES)
def test_ordinary_sequences_are_not_redone(B, T, K, scale):
    """the problems of test_hmm_hip.py::test_hmm_estep_against_oracle_and_reference (and of its wide twin) with scale <= 3
    stay on the scaled route, every sequence: the cap on false positives of the range criterion"""
    rng = np.random.default_rng(B * 100 + T + K)
    init, pair, node = R.ordinary(B, T, K, rng, scale)
    _, redone = _estep(init, pair, node)
    assert not redone.any(), redone


def test_redone_share_on_wide_potentials_is_reported():
    """no cap, a figure: the share of sequences redone at scale = 50 (T = 500, K = 8) and on the
    HMM node potentials of the SLDS golden run (tests/golden/slds_K8_n10_T40.npz); both still match the oracle"""
    rng = np.random.default_rng(2 * 100 + 500 + 8)
    init, pair, node = R.ordinary(2, 500, 8, rng, 50.0)
    got, redone = _estep(init, pair, node)
    print("redone share, scale 50, T 500, K 8: %d of %d" % (redone.sum(), redone.size))
    _check(got, [R._oracle(init, pair, node[b]) for b in range(2)])
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slds_K8_n10_T40.npz"))
    init, pair, node = d["hmm_init"], d["hmm_pair"], d["opt_node_hmm"]
    got, redone = _estep(init, pair, node)
    print("redone share, SLDS golden node potentials (K 8, T 40): %d of %d" % (redone.sum(), redone.size))
    _check(got, [R._oracle(init, pair, node[b]) for b in range(node.shape[0])])
