"""CPU test of the ISA of the units of the HMM E-step's derivative (csrc/hmm_estep_vjp.hip, hmm_estep_vjp_ragged.hip):
every kernel compiles for gfx950 without a private segment and without spills, and the DPP hazard audit
(tools/audit_dpp_hazards.py) has no findings."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("unit", ["hmm_estep_vjp", "hmm_estep_vjp_ragged"])
def test_vjp_unit_compiles_without_scratch_and_without_dpp_hazards(unit, tmp_path):
    import audit_dpp_hazards
    s = tmp_path / (unit + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "svae" in l]
    # 16 row kernels; the wide kernel scaled at KP = 32 and 64, in log space at KP = 16, 32 and 64
    for kernel, count in (("hmm_vjp_row_kernel", 16), ("hmm_vjp_wide_kernel", 5)):
        assert sum(kernel in n for n in names) == count, (kernel, names)
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 21 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == 21 and set(spills) == {"0"}, spills
    # the wide kernels at KP = 64: the matrix, V and the g_pair accumulators, KP x 64 doubles each, and two lines
    lds = sorted(int(l.split()[-1]) for l in isa.splitlines() if ".group_segment_fixed_size:" in l)
    assert lds[-1] == (3 * 64 * 64 + 128) * 8 and lds[-1] <= 160 * 1024
    n_dpp, findings = audit_dpp_hazards.audit(str(s))
    assert findings == [], findings[:5]
    assert n_dpp >= 2000, n_dpp            # (2272 as built) the row kernels' broadcast multiply-accumulates are there
    flags = open(os.path.join(CSRC, "Makefile")).read()
    assert unit + ".o" in flags and unit.replace("hmm_", "") + ".s" in flags       # in OBJS and in the audit target
