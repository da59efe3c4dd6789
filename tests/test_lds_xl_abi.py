"""CPU tests of the LDS E-step entries for latent dimension 65 <= n <= 128 (svae_lds_xl_*, include/svae_hip.h): the
workspace formula, host-side argument checks, the ISA of the kernel unit, and the sampler / VJP entry points that must
refuse these sizes before touching the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")


def _lib():
    from svae_amd import _lib as L
    return L, L.load()


def test_xl_symbols_and_limits():
    L, lib = _lib()
    for s in ("svae_lds_xl_workspace_bytes", "svae_lds_xl_estep_f64", "svae_lds_xl_reduce_stats_f64"):
        assert s in L.SIGNATURES and hasattr(lib, s)
    assert L.LDS_XL_MAX_N == 128
    hdr = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert "#define SVAE_LDS_XL_MAX_N 128" in hdr


@pytest.mark.parametrize("n", [65, 96, 128])
@pytest.mark.parametrize("inhomog,batched", [(0, 0), (1, 0), (1, 1)])
def test_xl_workspace_bytes_closed_form(n, inhomog, batched):
    _, lib = _lib()
    NP = 16 * ((n + 15) // 16)
    for B, T in ((1, 1), (3, 2), (5, 7), (512, 200)):
        packed = 0 if T < 2 else (B if batched else 1) * (T - 1 if inhomog else 2) * 3 * NP * NP
        assert lib.svae_lds_xl_workspace_bytes(B, T, n, inhomog, batched) == 8 * (B * T * (2 * NP * NP + NP) + packed)
    assert lib.svae_lds_xl_workspace_bytes(512, 200, 128, 0, 0) > 26.9e9


def test_xl_workspace_bytes_range():
    _, lib = _lib()
    for n in (1, 16, 64, 129, 200):
        assert lib.svae_lds_xl_workspace_bytes(2, 5, n, 0, 0) == 0
    assert lib.svae_lds_xl_workspace_bytes(0, 5, 80, 0, 0) == 0
    assert lib.svae_lds_xl_workspace_bytes(2, 0, 80, 0, 0) == 0
    # the existing entries keep their ranges
    assert lib.svae_lds_workspace_bytes(1, 1, 65) == 0
    assert lib.svae_lds_workspace_bytes_ex(1, 1, 65, 0, 0) == 0


def test_xl_estep_rejects_bad_arguments_on_the_host():
    """every argument error comes back before any HIP call (safe without a GPU)"""
    _, lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    info = (ctypes.c_int32 * 1)()
    pi = ctypes.cast(info, ctypes.c_void_p)
    ws_need = lib.svae_lds_xl_workspace_bytes(2, 3, 80, 0, 0)

    def call(B=2, T=3, n=80, inhomog=0, batched=0, keep=0, options=0, ptrs=None, info_p=pi, ws=p, ws_bytes=ws_need):
        ptrs = [p] * 15 if ptrs is None else ptrs
        return lib.svae_lds_xl_estep_f64(B, T, n, inhomog, batched, keep, options, *ptrs, info_p, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(T=0) == -2
    for n in (64, 129, 16, 1):
        assert call(n=n) == -3
    assert call(keep=1) == -23 and call(keep=4) == -23
    assert call(batched=1) == -5
    for k, code in ((0, -6), (1, -7), (2, -8), (3, -9), (7, -13), (8, -14), (10, -16), (11, -17), (12, -18),
                    (13, -19), (14, -20)):
        ptrs = [p] * 15
        ptrs[k] = None
        assert call(ptrs=ptrs) == code, k
    assert call(info_p=None) == -21
    assert call(ws=None) == -22
    assert call(ws_bytes=ws_need - 8) == -22
    assert call(options=1) == -24 and call(options=0x40) == -24
    assert call(B=0, ws_bytes=0) == 0    # empty batch: nothing to launch
    assert call(B=0, ptrs=[p] * 7 + [None] * 8, info_p=None, ws=None, ws_bytes=0) == 0
    assert call(B=0, options=1) == -24 and call(B=0, n=64) == -3
    # the existing entries keep their ranges
    null = None
    args = [null] * 15 + [null, null, 0, null]
    assert lib.svae_lds_estep_f64(4, 5, 65, 0, 0, 0, 0, *args) == -3
    assert lib.svae_lds_reduce_stats_f64(2, 65, p, p, p, p, None) == -2
    assert lib.svae_lds_xl_reduce_stats_f64(2, 64, p, p, p, p, None) == -2
    assert lib.svae_lds_xl_reduce_stats_f64(2, 129, p, p, p, p, None) == -2
    assert lib.svae_lds_xl_reduce_stats_f64(-1, 80, p, p, p, p, None) == -1
    assert lib.svae_lds_xl_reduce_stats_f64(2, 80, None, p, p, p, None) == -3


def test_xl_unit_compiles_without_scratch_and_without_dpp_hazards(tmp_path):
    """every NB = 5..8 instance: no private segment, no scratch instruction, and the DPP hazard audit passes"""
    s = tmp_path / "xl.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "lds_estep_xl.hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "lds_estep_xl_kernel" in l]
    assert len(names) == 8, names                       # NB = 5..8, homogeneous and per-step pair parameters
    for l in isa.splitlines():
        if ".private_segment_fixed_size:" in l:
            assert l.split()[-1] == "0", l
    audit = subprocess.run(["python3", os.path.join(ROOT, "tools", "audit_dpp_hazards.py"), str(s)],
                           capture_output=True, text=True)
    assert audit.returncode == 0, audit.stdout + audit.stderr


def test_xl_sampler_and_vjp_entry_points_refuse_before_the_device():
    """the entry points that need the sampler or the VJP name the 64 limit before they look for a device"""
    torch = pytest.importorskip("torch")
    from svae_amd.lds.lds_inference import lds_inference_differentiable, natural_lds_inference_general, natural_lds_sample
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    rng = np.random.default_rng(0)
    n, T = 80, 3
    natparam = rand_lds_natparam(n, rng)
    node = rand_node_potentials((2, T, n), rng)
    with pytest.raises(ValueError, match="64"):
        natural_lds_sample(natparam, node, 1)
    with pytest.raises(ValueError, match="64"):
        natural_lds_inference_general(natparam, node, num_samples=2)
    with pytest.raises(ValueError, match="64"):
        lds_inference_differentiable(natparam, tuple(torch.as_tensor(x) for x in node))
    with pytest.raises(ValueError, match="128"):
        from svae_amd.lds.lds_inference import LDSEStepPlan
        LDSEStepPlan(1, 2, 129, "cpu")
