"""C ABI of the parameter-gradient entry point (svae_lds_estep_vjp_params_f64, svae_lds_param_vjp_workspace_bytes): the
workspace formula and the argument checks, every one of which returns its documented code (include/svae_hip.h) before any
HIP call -- the pointers below are never dereferenced.  No GPU needed."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from svae_amd import _lib
    return _lib.load()


D = 0x1000          # a non-NULL pointer value that is never dereferenced (every case fails its checks first)
BIG = 1 << 50

# positions in the pointer block of svae_lds_estep_vjp_params_f64
J12, G_LOGNORM, G_DXX, G_X, G_EINIT, G_EPAIR, G_SAMPLES, EPS, SAMPLES, E_PAIR, E_NODE_X, G_NODE_J, G_NODE_H = range(13)
N_PTRS = 20          # + the seven parameter cotangents


def _call(lib, B=2, T=3, n=3, S=1, inhomog=0, pb=0, options=0, null=(), ws=D, ws_bytes=BIG, vws=D, vws_bytes=BIG,
          pws=D, pws_bytes=BIG):
    p = [D] * N_PTRS
    p[G_EINIT] = p[G_EPAIR] = None           # (optional cotangents: absent unless a case asks for them)
    for k in null:
        p[k] = None
    return lib.svae_lds_estep_vjp_params_f64(B, T, n, S, inhomog, pb, options, *p, ws, ws_bytes, vws, vws_bytes,
                                             pws, pws_bytes, None)


def test_workspace_formula(lib):
    f = lib.svae_lds_param_vjp_workspace_bytes
    # g_P (B,T,n,n) + g_R (B,T-1,2,n,n) [+ homogeneous: per-step batch sums (T-1,3,n,n)]
    assert f(3, 7, 5, 1, 0) == (3 * 7 * 25 + 3 * 6 * 2 * 25) * 8
    assert f(3, 7, 5, 1, 1) == (3 * 7 * 25 + 3 * 6 * 2 * 25) * 8
    assert f(3, 7, 5, 0, 0) == (3 * 7 * 25 + 3 * 6 * 2 * 25 + 6 * 3 * 25) * 8
    assert f(512, 200, 10, 0, 0) == (512 * 200 * 100 + 512 * 199 * 200 + 199 * 300) * 8
    assert f(2, 1, 4, 0, 0) == 2 * 16 * 8                       # T = 1: no pair steps
    assert f(1, 1, 15, 1, 0) == 225 * 8
    for n in (0, -1, 16, 64):
        assert f(2, 3, n, 0, 0) == 0
    assert f(0, 3, 4, 0, 0) == 0 and f(-1, 3, 4, 0, 0) == 0
    assert f(2, 0, 4, 0, 0) == 0 and f(2, -3, 4, 0, 0) == 0


def test_size_checks(lib):
    assert _call(lib, B=-1) == -1
    assert _call(lib, T=0) == -2
    assert _call(lib, n=0) == -3
    assert _call(lib, n=16) == -3             # the register path only: launches nothing
    assert _call(lib, n=64) == -3
    assert _call(lib, S=0) == -4              # with g_samples given
    assert _call(lib, S=17) == -4
    assert _call(lib, inhomog=0, pb=1) == -7
    assert _call(lib, T=65537) == -30


def test_pointer_checks(lib):
    assert _call(lib, null=(J12,)) == -5
    assert _call(lib, T=1, null=(J12,), ws_bytes=0) == -14       # (T = 1 needs no J12: the next check fails)
    assert _call(lib, null=(G_LOGNORM,)) == -6
    p = [D] * N_PTRS
    p[G_EINIT] = None
    assert lib.svae_lds_estep_vjp_params_f64(2, 3, 3, 1, 0, 0, 0, *p, D, BIG, D, BIG, D, BIG, None) == -8   # g_E_pair: per-step only
    p[E_PAIR] = None
    assert lib.svae_lds_estep_vjp_params_f64(2, 3, 3, 1, 1, 0, 0, *p, D, BIG, D, BIG, D, BIG, None) == -8   # .. needs E_pair
    assert _call(lib, null=(EPS,)) == -10
    assert _call(lib, null=(SAMPLES,)) == -10
    assert _call(lib, null=(G_NODE_J,)) == -12
    assert _call(lib, null=(G_NODE_H,)) == -13
    assert _call(lib, ws=None) == -14
    assert _call(lib, ws_bytes=lib.svae_lds_workspace_bytes(2, 3, 3) - 1) == -14
    assert _call(lib, vws=None) == -16
    assert _call(lib, vws_bytes=lib.svae_lds_vjp_workspace_bytes(2, 3, 3) - 1) == -16
    assert _call(lib, pws=None) == -29
    assert _call(lib, pws_bytes=lib.svae_lds_param_vjp_workspace_bytes(2, 3, 3, 0, 0) - 1) == -29
    # homogeneous parameters need the per-step batch sums on top of what per-step ones need
    assert _call(lib, pws_bytes=lib.svae_lds_param_vjp_workspace_bytes(2, 3, 3, 1, 0)) == -29


def test_option_checks(lib):
    from svae_amd import _lib
    assert _call(lib, options=_lib.OPT_LEAN_ON | _lib.OPT_LEAN_OFF) == -24
    assert _call(lib, options=0x8000) == -24
    assert _call(lib, options=_lib.OPT_PRODUCERS_ON | _lib.OPT_PRODUCERS_OFF) == -24
    # lean records (the workspace of svae_lds_inference_f64 on a shape it keeps lean records for): refused, nothing launched
    assert lib.svae_lds_inference_is_lean(2, 3, 3, 1, 0, 1, _lib.OPT_LEAN_ON) == 1
    assert _call(lib, options=_lib.OPT_LEAN_ON | _lib.OPT_INFER_RECORDS) == -8
    assert _call(lib, B=2000, options=_lib.OPT_INFER_RECORDS) == -8          # (the default from 1025 sequences)


def test_empty_batch_is_a_no_op(lib):
    assert _call(lib, B=0) == 0
    assert _call(lib, B=0, pws=None, pws_bytes=0) == 0
    assert _call(lib, B=0, null=tuple(range(13, N_PTRS))) == 0
