"""C ABI of the three reverse-mode primitives (svae_lds_{filter,smoother,sample}_vjp_f64): argument checks that return
before any HIP call, the workspace formula, and the DPP hazard audit of the per-n unit's ISA.  No GPU needed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from svae_amd import _lib
    return _lib.load()


D = 0x1000          # a non-NULL pointer value that is never dereferenced (every case fails its checks first)


def _filter(lib, B=1, T=3, n=3, inhomog=0, pb=0, null=None):
    p = [D] * 12
    if null is not None:
        p[null] = None
    return lib.svae_lds_filter_vjp_f64(B, T, n, inhomog, pb, *p, None, None)


def _smoother(lib, B=1, T=3, n=3, inhomog=0, pb=0, null=None, ws=D, ws_bytes=1 << 40):
    p = [D] * 15
    if null is not None:
        p[null] = None
    return lib.svae_lds_smoother_vjp_f64(B, T, n, inhomog, pb, *p, None, ws, ws_bytes, None)


def _sample(lib, B=1, T=3, n=3, S=2, inhomog=0, pb=0, null=None):
    p = [D] * 11
    if null is not None:
        p[null] = None
    return lib.svae_lds_sample_vjp_f64(B, T, n, S, inhomog, pb, *p, None, None)


def test_abi_version(lib):
    assert lib.svae_hip_abi_version() == 15


@pytest.mark.parametrize("call", [_filter, _smoother, _sample])
def test_size_checks(lib, call):
    assert call(lib, n=0) == -3
    assert call(lib, n=16) == -3
    assert call(lib, T=0) == -2
    assert call(lib, B=-1) == -1
    assert call(lib, inhomog=0, pb=1) == -7


def test_null_pointers(lib):
    assert _filter(lib, null=0) == -5 and _filter(lib, null=1) == -5
    assert _filter(lib, null=2) == -6 and _filter(lib, null=3) == -6
    for k in range(4, 9):
        assert _filter(lib, null=k) == -8
    for k in range(9, 12):
        assert _filter(lib, null=k) == -9
    for k in range(3):
        assert _smoother(lib, null=k) == -5
    for k in range(3, 7):
        assert _smoother(lib, null=k) == -6
    for k in range(11, 15):
        assert _smoother(lib, null=k) == -9
    assert _smoother(lib, ws=None) == -14
    assert _smoother(lib, ws_bytes=lib.svae_lds_smoother_vjp_workspace_bytes(1, 3, 3) - 1) == -14
    for k in range(2):
        assert _sample(lib, null=k) == -5
    for k in range(2, 4):
        assert _sample(lib, null=k) == -6
    for k in range(4, 7):
        assert _sample(lib, null=k) == -8
    for k in range(7, 11):
        assert _sample(lib, null=k) == -9
    assert _sample(lib, S=0) == -4 and _sample(lib, S=17) == -4


@pytest.mark.parametrize("B,T,n", [(1, 1, 1), (3, 7, 5), (512, 200, 10), (4096, 200, 15)])
def test_smoother_workspace_formula(lib, B, T, n):
    assert lib.svae_lds_smoother_vjp_workspace_bytes(B, T, n) == B * T * (3 * n * n + 2 * n) * 8
    assert lib.svae_lds_smoother_vjp_workspace_bytes(B, T, 16) == 0


@pytest.mark.parametrize("n", [1, 7, 15])
def test_prim_unit_dpp_hazard_audit(tmp_path, n):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "svae_amd", "csrc")
    s = str(tmp_path / ("p%d.s" % n))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DSVAE_N=%d" % n, "--cuda-device-only", "-S",
                    os.path.join(csrc, "lds_prim_vjp_n.hip"), "-o", s], check=True, cwd=csrc)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), s],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
