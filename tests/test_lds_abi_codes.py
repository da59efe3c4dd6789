"""CPU test of the host-side argument checks of the uniform LDS entry points (include/svae_hip.h): every code an entry
point can return before a launch, which error wins when two checks are violated at once, and what an empty batch
returns.  No call here may reach a HIP call: each one has B == 0 or carries at least one error, and every assertion is
on an exact code (a call that slipped through to a launch comes back -1000 without a GPU and fails)."""
import ctypes

import pytest

from svae_amd import _lib as L


@pytest.fixture(scope="module")
def lib():
    return L.load()


_BUF = (ctypes.c_double * 64)()
P = ctypes.cast(_BUF, ctypes.c_void_p)        # any non-NULL address: every call returns before it is used
BIG = 1 << 62                                 # a byte count that passes every size check

MODEL = ["init_J", "init_h", "init_logZ", "J11", "J12", "J22", "logZ_pair", "node_J", "node_h", "node_logZ"]
STATS = ["lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x"]
# the pointer checks the E-step-like entry points share, in source order: (code, the argument that is NULL)
MODEL_CHECKS = [(-6, "init_J"), (-7, "init_h"), (-8, "init_logZ"), (-9, "J11"), (-13, "node_J"), (-14, "node_h")]
STATS_CHECKS = [(-16, "lognorm"), (-17, "E_init"), (-18, "E_pair"), (-19, "E_node_diagxx"), (-20, "E_node_x")]


def null(checks):
    return [(code, {name: None}) for code, name in checks]


def entry(lib, fn, names, **base):
    """call(**overrides) -> the return code of lib.fn on the valid argument set `base` with `overrides` applied"""
    assert set(base) == set(names), set(base) ^ set(names)

    def call(**kw):
        assert set(kw) <= set(names), set(kw) - set(names)
        a = dict(base, **kw)
        return getattr(lib, fn)(*[a[k] for k in names])
    return call


def walk(call, ladder, cannot_coincide=()):
    """ladder: the checks in source order as (code, overrides that violate that check alone).  Each violation alone returns
    its code; each consecutive pair violated together returns the FIRST one's code.  cannot_coincide: consecutive pairs
    (code, code) that no argument set violates together."""
    for code, kw in ladder:
        assert call(**kw) == code, (code, kw)
    done = 0
    for (c1, k1), (c2, k2) in zip(ladder, ladder[1:]):
        if (c1, c2) in cannot_coincide:
            continue
        assert all(k1[k] == k2[k] for k in set(k1) & set(k2)), (c1, c2)
        assert call(**dict(k2, **k1)) == c1, (c1, c2)
        done += 1
    assert done == len(ladder) - 1 - len(cannot_coincide)


def test_estep_codes(lib):
    need = lib.svae_lds_workspace_bytes(2, 3, 4)
    names = ["B", "T", "n", "inhomog", "pair_batched", "keep", "options"] + MODEL + STATS + ["info", "ws", "ws_bytes", "stream"]
    base = dict(B=2, T=3, n=4, inhomog=0, pair_batched=0, keep=0, options=0, info=P, ws=P, ws_bytes=need, stream=None)
    base.update({k: P for k in MODEL + STATS})
    call = entry(lib, "svae_lds_estep_f64", names, **base)
    walk(call, [(-1, dict(B=-1)), (-2, dict(T=0)), (-3, dict(n=0)), (-23, dict(keep=4)), (-5, dict(pair_batched=1))]
         + null(MODEL_CHECKS + STATS_CHECKS) + [(-21, dict(info=None)), (-22, dict(ws=None)), (-24, dict(options=3))])
    assert call(n=65) == -3 and call(n=128) == -3
    assert call(keep=-1) == -23 and call(n=16, keep=1) == -23 and call(n=16, keep=5) == -23
    for k in ("J12", "J22", "logZ_pair"):
        assert call(**{k: None}) == -9
    assert call(T=1, J11=None, J12=None, J22=None, logZ_pair=None, ws=None) == -22        # T = 1: no pair parameters
    assert call(node_logZ=None, ws=None) == -22                                           # node_logZ may be NULL
    assert call(ws_bytes=need - 8) == -22
    for bad in (L.OPT_LAYOUT_SPLIT | L.OPT_LAYOUT_PACKED, L.OPT_PRODUCERS_ON | L.OPT_PRODUCERS_OFF, 0x1000,
                L.OPT_LEAN_ON | L.OPT_LEAN_OFF, L.OPT_TILE_FORWARD, L.OPT_TILE_BACKWARD):
        assert call(options=bad) == -24, bad
    assert call(n=16, ws_bytes=BIG, options=L.OPT_TILE_FORWARD | L.OPT_TILE_BACKWARD) == -24
    assert call(n=16, ws_bytes=BIG, options=L.OPT_TILE_FORWARD | 3) == -24
    # tiled path, SVAE_KEEP_SIGMA: the section behind the workspace is checked after the B == 0 return
    off = lib.svae_lds_tile_sigma_offset_bytes(2, 3, 40, 0, 0)
    assert call(n=40, keep=L.KEEP_SIGMA, ws_bytes=off + 2 * 3 * 40 * 40 * 8 - 8) == -22
    # an empty batch: 0, after every check above
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0 and call(B=0, n=40, keep=L.KEEP_SIGMA, ws_bytes=0) == 0
    assert call(B=0, ws=None) == -22 and call(B=0, options=3) == -24 and call(B=0, options=L.OPT_TILE_FORWARD) == -24
    assert call(B=0, info=None) == -21 and call(B=0, init_J=None) == -6 and call(B=0, keep=4) == -23


def test_filter_codes(lib):
    need = lib.svae_lds_workspace_bytes(2, 3, 4)
    msgs = ["J_pred", "h_pred", "J_filt", "h_filt"]
    names = ["B", "T", "n", "inhomog", "pair_batched", "options"] + MODEL + ["lognorm"] + msgs + ["info", "ws", "ws_bytes", "stream"]
    base = dict(B=2, T=3, n=4, inhomog=0, pair_batched=0, options=0, lognorm=P, info=P, ws=P, ws_bytes=need, stream=None)
    base.update({k: P for k in MODEL + msgs})
    call = entry(lib, "svae_lds_filter_f64", names, **base)
    walk(call, [(-1, dict(B=-1)), (-2, dict(T=0)), (-3, dict(n=16)), (-5, dict(pair_batched=1))] + null(MODEL_CHECKS)
         + [(-16, dict(lognorm=None)), (-21, dict(info=None)), (-22, dict(ws=None)), (-24, dict(options=3))])
    assert call(n=0) == -3 and call(n=64) == -3
    for k in ("J12", "J22", "logZ_pair"):
        assert call(**{k: None}) == -9
    assert call(T=1, J11=None, J12=None, J22=None, logZ_pair=None, ws=None) == -22
    assert call(ws_bytes=need - 8) == -22
    assert call(J_pred=None, h_pred=None, J_filt=None, h_filt=None, node_logZ=None, ws=None) == -22      # all optional
    assert call(options=0x40) == -24 and call(options=0x0c) == -24 and call(options=0x30) == -24
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0
    assert call(B=0, ws=None) == -22 and call(B=0, options=3) == -24 and call(B=0, info=None) == -21


def test_sample_codes(lib):
    need = lib.svae_lds_workspace_bytes(2, 3, 4)
    names = ["B", "T", "n", "S", "options", "eps", "samples", "ws", "ws_bytes", "stream"]
    call = entry(lib, "svae_lds_sample_f64", names, B=2, T=3, n=4, S=1, options=0, eps=P, samples=P, ws=P, ws_bytes=need,
                 stream=None)
    walk(call, [(-1, dict(B=-1)), (-2, dict(T=0)), (-3, dict(n=16)), (-4, dict(S=0)), (-5, dict(eps=None)),
                (-6, dict(samples=None)), (-7, dict(ws=None)), (-24, dict(options=3))])
    assert call(n=0) == -3 and call(S=-1) == -4 and call(ws_bytes=need - 8) == -7
    assert call(options=0x40) == -24 and call(options=0x30) == -24
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0
    assert call(B=0, ws=None) == -7 and call(B=0, options=3) == -24 and call(B=0, S=0) == -4


def _inference(lib, options):
    need = lib.svae_lds_workspace_bytes(2, 3, 4)
    names = (["B", "T", "n", "S", "inhomog", "pair_batched", "keep_vjp", "options"] + MODEL + ["eps", "samples"] + STATS
             + ["info", "ws", "ws_bytes", "stream"])
    base = dict(B=2, T=3, n=4, S=1, inhomog=0, pair_batched=0, keep_vjp=1, options=options, eps=P, samples=P, info=P, ws=P,
                ws_bytes=need, stream=None)
    base.update({k: P for k in MODEL + STATS})
    return entry(lib, "svae_lds_inference_f64", names, **base), need


def test_inference_general_branch_codes(lib):
    """B below LEAN_MIN_B without SVAE_OPT_LEAN_ON: the checks of svae_lds_estep_f64 behind -3 and -4 (the keep word it
    passes is 0, 1 or 3: no -23)"""
    call, need = _inference(lib, 0)
    assert lib.svae_lds_inference_is_lean(2, 3, 4, 1, 0, 1, 0) == 0
    walk(call, [(-3, dict(n=16)), (-4, dict(S=-1)), (-1, dict(B=-1)), (-2, dict(T=0)), (-5, dict(pair_batched=1))]
         + null(MODEL_CHECKS + STATS_CHECKS) + [(-21, dict(info=None)), (-22, dict(ws=None)), (-24, dict(options=3))])
    assert call(n=0) == -3 and call(eps=None) == -4 and call(samples=None) == -4
    assert call(S=0, eps=None, samples=None, ws=None) == -22
    assert call(T=1, J11=None, ws=None) == -22 and call(ws_bytes=need - 8) == -22
    assert call(options=L.OPT_LEAN_OFF | 0x0c) == -24
    # this branch masks the word with SVAE_OPT_ALL before it hands it on: a bit outside it is dropped, not refused (the
    # lean branch below and svae_lds_estep_f64 itself return -24 for it)
    assert call(B=0, options=0x1000) == 0 and call(options=0x1000, ws=None) == -22
    for keep_vjp, S in ((0, 0), (0, 1), (1, 0), (1, 2)):
        assert call(B=0, keep_vjp=keep_vjp, S=S) == 0
    assert call(B=0, ws=None) == -22 and call(B=0, options=3) == -24 and call(B=0, S=-1) == -4


def test_inference_lean_branch_codes(lib):
    """SVAE_OPT_LEAN_ON: its own ladder, with -5 behind -9"""
    call, need = _inference(lib, L.OPT_LEAN_ON)
    assert lib.svae_lds_inference_is_lean(2, 3, 4, 1, 0, 1, L.OPT_LEAN_ON) == 1
    assert lib.svae_lds_inference_is_lean(-1, 3, 4, 1, 0, 1, L.OPT_LEAN_ON) == 1
    walk(call, [(-3, dict(n=16)), (-4, dict(S=-1)), (-1, dict(B=-1))] + null(MODEL_CHECKS[:4])
         + [(-5, dict(pair_batched=1))] + null(MODEL_CHECKS[4:] + STATS_CHECKS)
         + [(-21, dict(info=None)), (-22, dict(ws=None)), (-24, dict(options=L.OPT_LEAN_ON | 3))])
    for k in ("J12", "J22", "logZ_pair"):
        assert call(**{k: None}) == -9
    assert call(T=0) == -2 and call(T=1, ws=None) == -22            # T < 2: the general branch
    assert call(ws_bytes=need - 8) == -22 and call(eps=None) == -4
    assert call(options=L.OPT_LEAN_ON | 0x1000) == -24
    assert call(B=0) == 0 and call(B=0, S=0, eps=None, samples=None, keep_vjp=0) == 0
    assert call(B=0, ws=None) == -22 and call(B=0, options=L.OPT_LEAN_ON | 3) == -24 and call(B=0, J11=None) == -9


VJP_PTRS = ["J12", "g_lognorm", "g_E_node_diagxx", "g_E_node_x", "g_E_init", "g_E_pair", "g_samples", "eps", "samples",
            "E_pair", "E_node_x", "g_node_J", "g_node_h"]
VJP_TAIL = ["ws", "ws_bytes", "vws", "vws_bytes", "stream"]
VJP_LADDER = [(-1, dict(B=-1)), (-2, dict(T=0)), (-3, dict(n=16)), (-4, dict(S=0)), (-5, dict(J12=None)),
              (-6, dict(g_lognorm=None)), (-7, dict(pair_batched=1)), (-8, dict(g_E_pair=P)), (-10, dict(eps=None)),
              (-12, dict(g_node_J=None)), (-13, dict(g_node_h=None)), (-14, dict(ws=None)), (-16, dict(vws=None)),
              (-24, dict(options=3))]


def _vjp_base(lib):
    base = dict(B=2, T=3, n=4, S=1, inhomog=0, pair_batched=0, options=0, ws=P, ws_bytes=lib.svae_lds_workspace_bytes(2, 3, 4),
                vws=P, vws_bytes=lib.svae_lds_vjp_workspace_bytes(2, 3, 4), stream=None)
    base.update({k: P for k in VJP_PTRS})
    base["g_E_pair"] = None                     # (a cotangent of the per-step statistics needs inhomog: -8)
    return base


def _vjp_common(call, base):
    """what vjp_impl checks, whichever entry point it is reached through"""
    assert call(n=0) == -3 and call(S=17) == -4
    assert call(S=0, g_samples=None, eps=None, samples=None, ws=None) == -14        # no sample cotangents: S is not read
    assert call(T=1, J12=None, ws=None) == -14
    assert call(inhomog=1, g_E_pair=P, E_pair=None) == -8 and call(inhomog=1, g_E_pair=P, E_node_x=None) == -8
    assert call(inhomog=1, g_E_pair=P, ws=None) == -14
    assert call(samples=None) == -10
    assert call(ws_bytes=base["ws_bytes"] - 8) == -14 and call(vws_bytes=base["vws_bytes"] - 8) == -16
    assert call(options=0x40) == -24 and call(options=L.OPT_INFER_RECORDS | 0x0c) == -24
    assert call(B=0) == 0 and call(B=0, ws_bytes=0, vws_bytes=0) == 0
    assert call(B=0, ws=None) == -14 and call(B=0, vws=None) == -16 and call(B=0, options=3) == -24
    # lean records (SVAE_OPT_INFER_RECORDS where svae_lds_inference_f64 wrote them): no statistics cotangents
    lean = L.OPT_INFER_RECORDS | L.OPT_LEAN_ON
    assert call(options=lean, g_E_init=P) == -8


def test_vjp_ex_codes(lib):
    base = _vjp_base(lib)
    names = ["B", "T", "n", "S", "inhomog", "pair_batched", "options"] + VJP_PTRS + VJP_TAIL
    call = entry(lib, "svae_lds_estep_vjp_ex_f64", names, **base)
    walk(call, VJP_LADDER)
    _vjp_common(call, base)
    assert call(B=0, options=L.OPT_INFER_RECORDS | L.OPT_LEAN_ON) == 0


def test_vjp_dense_codes(lib):
    base = dict(_vjp_base(lib), g_node_J_dense=P)
    names = ["B", "T", "n", "S", "inhomog", "pair_batched", "options"] + VJP_PTRS + ["g_node_J_dense"] + VJP_TAIL
    call = entry(lib, "svae_lds_estep_vjp_dense_f64", names, **base)
    walk(call, [(-27, dict(g_node_J_dense=None))] + VJP_LADDER)
    _vjp_common(call, base)
    assert call(options=L.OPT_INFER_RECORDS | L.OPT_LEAN_ON, g_E_init=None) == -8        # the dense cotangent itself
    assert call(B=0, g_node_J_dense=None) == -27


def test_vjp_params_codes(lib):
    grads = ["g_init_J", "g_init_h", "g_init_logZ", "g_J11", "g_J12", "g_J22", "g_logZ_pair"]
    pneed = lib.svae_lds_param_vjp_workspace_bytes(2, 3, 4, 0, 0)
    assert pneed > 0
    base = dict(_vjp_base(lib), pws=P, pws_bytes=pneed)
    base.update({k: P for k in grads})
    names = (["B", "T", "n", "S", "inhomog", "pair_batched", "options"] + VJP_PTRS + grads + VJP_TAIL[:4]
             + ["pws", "pws_bytes", "stream"])
    call = entry(lib, "svae_lds_estep_vjp_params_f64", names, **base)
    # -30 needs B > 0 and T > 65536: it cannot coincide with -1 (the pair with -3 is below)
    walk(call, [(-29, dict(pws=None)), (-30, dict(T=65537, pws_bytes=BIG))] + VJP_LADDER, cannot_coincide=[(-30, -1)])
    assert call(T=65537, pws_bytes=BIG, n=16) == -30 and call(T=65537, pws_bytes=BIG, S=0) == -30
    assert call(pws_bytes=pneed - 8) == -29
    assert call(pws=None, S=0) == -29 and call(pws=None, options=3) == -29
    # sizes that vjp_impl refuses need no parameter workspace: their own codes
    assert call(pws=None, B=-1) == -1 and call(pws=None, T=0) == -2 and call(pws=None, n=16) == -3
    _vjp_common(call, base)
    assert call(B=0, pws=None, pws_bytes=0) == 0 and call(B=0, T=65537) == 0
    assert call(options=L.OPT_INFER_RECORDS | L.OPT_LEAN_ON, g_E_init=None) == -8        # (it always carries g_P)


def test_slds_meanfield_codes(lib):
    ptrs = ["init_J", "init_h", "J11", "J12", "J22", "weights", "node_J", "node_h", "node_logZ", "seq_index"]
    outs = ["lognorm", "E_init", "E_node_diagxx", "E_node_x", "pair_contr"]
    names = ["B", "rows", "T", "n", "K"] + ptrs + outs + ["info", "ws", "ws_bytes", "options", "stream"]
    need = lib.svae_slds_lds_meanfield_workspace_bytes(2, 4, 4)
    assert need > 0
    base = dict(B=2, rows=2, T=4, n=4, K=2, info=P, ws=P, ws_bytes=need, options=0, stream=None)
    base.update({k: P for k in ptrs + outs})
    call = entry(lib, "svae_slds_lds_meanfield_f64", names, **base)
    walk(call, [(-1, dict(B=-1)), (-2, dict(T=3)), (-3, dict(n=11)), (-4, dict(K=0))]
         + null([(-5, "init_J"), (-6, "init_h"), (-7, "J11"), (-10, "weights"), (-11, "node_J"), (-12, "node_h"),
                 (-15, "lognorm"), (-16, "E_init"), (-17, "E_node_diagxx"), (-18, "E_node_x"), (-19, "pair_contr"),
                 (-20, "info"), (-21, "ws")]) + [(-24, dict(options=L.OPT_TWOEND_OFF))])
    assert call(B=3) == -1 and call(n=0) == -3 and call(K=17) == -4
    assert call(J12=None) == -7 and call(J22=None) == -7
    assert call(node_logZ=None, seq_index=None, ws=None) == -21                           # both optional
    assert call(ws_bytes=need - 8) == -21
    assert call(options=L.OPT_LAYOUT_SPLIT | L.OPT_LAYOUT_PACKED) == -24 and call(options=L.OPT_PRODUCERS_ON) == -24
    assert call(K=9, options=L.OPT_LAYOUT_PACKED) == -24                                  # row-per-chain layout: K <= 8
    assert call(B=0) == 0 and call(B=0, options=L.OPT_LAYOUT_SPLIT) == 0 and call(B=0, options=L.OPT_LAYOUT_PACKED) == 0
    assert call(B=0, K=9) == 0
    assert call(B=0, ws=None) == -21 and call(B=0, ws_bytes=need - 8) == -21              # (sized by rows, not by B)
    assert call(B=0, options=1) == -24 and call(B=0, K=9, options=L.OPT_LAYOUT_PACKED) == -24


@pytest.mark.parametrize("fn,n_ok,n_bad", [("svae_lds_reduce_stats_f64", 4, (0, 65, 128)),
                                           ("svae_lds_xl_reduce_stats_f64", 80, (0, 4, 64, 129))])
def test_reduce_stats_codes(lib, fn, n_ok, n_bad):
    """(both launch even at B == 0: only their error cases are probed)"""
    names = ["B", "n", "E_init", "E_pair", "lognorm", "out", "stream"]
    call = entry(lib, fn, names, B=2, n=n_ok, E_init=P, E_pair=P, lognorm=P, out=P, stream=None)
    walk(call, [(-1, dict(B=-1)), (-2, dict(n=n_bad[0]))]
         + null([(-3, "E_init"), (-4, "E_pair"), (-5, "lognorm"), (-6, "out")]))
    for n in n_bad:
        assert call(n=n) == -2
    assert call(B=0, out=None) == -6 and call(B=0, n=n_bad[-1]) == -2


def test_xl_estep_codes(lib):
    need = lib.svae_lds_xl_workspace_bytes(2, 3, 80, 0, 0)
    assert need > 0
    names = ["B", "T", "n", "inhomog", "pair_batched", "keep", "options"] + MODEL + STATS + ["info", "ws", "ws_bytes", "stream"]
    base = dict(B=2, T=3, n=80, inhomog=0, pair_batched=0, keep=0, options=0, info=P, ws=P, ws_bytes=need, stream=None)
    base.update({k: P for k in MODEL + STATS})
    call = entry(lib, "svae_lds_xl_estep_f64", names, **base)
    walk(call, [(-1, dict(B=-1)), (-2, dict(T=0)), (-3, dict(n=64)), (-23, dict(keep=1)), (-5, dict(pair_batched=1))]
         + null(MODEL_CHECKS[:4]) + [(-24, dict(options=1))] + null(MODEL_CHECKS[4:] + STATS_CHECKS)
         + [(-21, dict(info=None)), (-22, dict(ws=None))])
    assert call(n=129) == -3 and call(n=4) == -3 and call(keep=L.KEEP_SIGMA) == -23
    for k in ("J12", "J22", "logZ_pair"):
        assert call(**{k: None}) == -9
    assert call(T=1, J11=None, ws=None) == -22 and call(ws_bytes=need - 8) == -22
    assert call(options=L.OPT_LEAN_ON) == -24 and call(options=L.OPT_TILE_FORWARD) == -24
    # the empty batch returns ahead of the per-sequence arrays' checks, behind the model's and the options word's
    assert call(B=0) == 0
    assert call(B=0, node_J=None, node_h=None, lognorm=None, E_init=None, E_pair=None, E_node_diagxx=None, E_node_x=None,
                info=None, ws=None, ws_bytes=0) == 0
    assert call(B=0, options=1) == -24 and call(B=0, J11=None) == -9 and call(B=0, init_J=None) == -6
    assert call(B=0, keep=1) == -23
