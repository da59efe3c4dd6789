"""CPU checks behind tests/test_hmm_sample_range_hip.py (HMM posterior sampling under the E-step's range contract,
csrc/hmm_sample_kernel.hpp and csrc/hmm_sample_log.hip): the margin of every case the GPU file compares label for label,
the teeth of those cases (the sampler's arithmetic before the contract, tests/_hmm_sample_range_numpy.old_sample, draws
other paths than the log-space oracle on them), the export of sample_redone_sequences, and the ISA of the new unit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _hmm_range_numpy as R  # noqa: E402
import _hmm_sample_numpy as smp  # noqa: E402
import _hmm_sample_range_numpy as Q  # noqa: E402


# ---- margins: a condition on the inputs of the exact comparisons, not a tolerance of the kernel ----------------------
@pytest.mark.parametrize("K", Q.ALL_K)
def test_margins_and_teeth_of_the_gap_batches(K):
    """every T: the oracle's margin, and the old arithmetic off on an extreme sequence (g >= 745)"""
    for T in R.GAP_T:
        b = Q.gap_batch(K, T)
        print("gap K=%d T=%d margin %.3g, %d extreme of %d" % (K, T, b["margin"], b["extreme"].sum(), b["extreme"].size))
        assert b["margin"] >= smp.MARGIN, (T, b["margin"])
        assert b["node"].shape[0] == (22 if T == 4 else 88) and b["extreme"].sum() == (8 if T == 4 else 32)
        assert Q.old_differs(b), T


@pytest.mark.parametrize("name", Q.FAMILIES)
@pytest.mark.parametrize("K", Q.FAMILY_K)
def test_margins_and_teeth_of_the_family_batches(K, name):
    """sparse and ramp have teeth; surprise only covers the route (the old per-step filter gets it right)"""
    b = Q.family_batch(name, K)
    print("%s K=%d margin %.3g" % (name, K, b["margin"]))
    assert b["margin"] >= smp.MARGIN, b["margin"]
    assert b["extreme"].any()
    if name != "surprise":
        assert Q.old_differs(b)


@pytest.mark.parametrize("K", Q.ALL_K)
def test_margins_of_the_ragged_gap_batches(K):
    b = Q.ragged_gap_batch(K)
    print("ragged gap K=%d margin %.3g" % (K, b["margin"]))
    assert b["margin"] >= smp.MARGIN, b["margin"]
    L = b["lengths"]
    assert L[1] == 1 and L[2] == 2 and b["extreme"].any()
    for i in (1, 2, 5):
        assert np.isnan(b["node"][i, L[i]:]).all() and np.isnan(b["u"][i, :, L[i]:]).all()
        assert (b["states"][i, :, L[i]:] == -1).all() and b["states"][i, :, :L[i]].min() >= 0


@pytest.mark.parametrize("variant", Q.VARIANTS)
@pytest.mark.parametrize("K", Q.ALL_K)
def test_margins_of_the_mixed_batches(K, variant):
    b = Q.mixed(K, variant)
    print("mixed K=%d %s margin %.3g" % (K, variant, b["margin"]))
    assert b["margin"] >= smp.MARGIN, b["margin"]
    assert b["extreme"].any() and not b["extreme"][b["ordinary"]].any()


def test_old_arithmetic_is_the_oracle_on_ordinary_work():
    """old_sample is a faithful sampler where nothing is extreme: the oracle's paths on a grid case"""
    init, pair, node, u, want, want_lz, margin = smp.grid_case(5, 7, 5, 1.0)
    assert margin >= smp.MARGIN
    for b in range(5):
        got, lz = Q.old_sample(init, pair, node[b], u[b])
        assert np.array_equal(got, want[b]) and lz == pytest.approx(want_lz[b], rel=1e-12)


# ---- Python surface ---------------------------------------------------------------------------------------------------
def test_sample_redone_sequences_is_exported_and_checks_its_arguments():
    torch = pytest.importorskip("torch")
    import svae_amd.hmm as H
    from svae_amd.hmm import hmm_inference
    assert H.sample_redone_sequences is hmm_inference.sample_redone_sequences
    f = hmm_inference.sample_redone_sequences
    # the records describe themselves: a scaled record has a positive entry, a log record none
    B, T, K, KP = 3, 2, 17, 32
    ws = torch.zeros(B, T, KP, dtype=torch.float64)
    ws[0, 0, 5] = 1.0
    ws[1] = -float("inf")
    ws[1, :, 3] = 0.0
    ws[2, 0, :K] = -1.0                                                  # (flagged and not yet redone)
    ws[2, 0, K] = 1.0                                                    # a padding lane is not looked at
    assert f(ws, B, T, K).tolist() == [False, True, True]
    with pytest.raises(ValueError):
        f(ws, B, T, 65)
    with pytest.raises(ValueError):
        f(ws, B + 1, T, K)
    with pytest.raises(ValueError):
        f(ws.float(), B, T, K)


# ---- the new unit ---------------------------------------------------------------------------------------------------------
def test_log_unit_compiles_without_scratch_and_without_dpp_hazards(tmp_path):
    """csrc/hmm_sample_log.hip: three uniform and three ragged kernels (KP = 16, 32, 64), no private segment, no spills,
    one 64-double LDS line; in OBJS and in the audit target"""
    import audit_dpp_hazards
    s = tmp_path / "hmm_sample_log.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, "hmm_sample_log.hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "svae" in l]
    assert len(names) == 6 and all("hmm_filter_log_kernel" in n for n in names), names
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 6 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == 6 and set(spills) == {"0"}, spills
    lds = {int(l.split()[-1]) for l in isa.splitlines() if ".group_segment_fixed_size:" in l}
    assert lds == {64 * 8}, lds
    _, findings = audit_dpp_hazards.audit(str(s))
    assert findings == [], findings[:5]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hmm_sample_log.o" in mk and "sample_log.s" in mk
