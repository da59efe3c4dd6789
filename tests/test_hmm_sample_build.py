"""CPU test of the ISA of the HMM sampling units (csrc/hmm_sample.hip, hmm_sample_ragged.hip): every instance compiles
for gfx950 without a private segment, and the DPP hazard audit (tools/audit_dpp_hazards.py) has no findings."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# DPP instructions of one unit as built (12908 uniform, more in the ragged one): the row kernels' broadcast
# multiply-accumulates; a unit far below has lost them to a compiler-only path
DPP_FLOOR = 10000


@pytest.mark.parametrize("unit", ["hmm_sample", "hmm_sample_ragged"])
def test_sample_unit_compiles_without_scratch_and_without_dpp_hazards(unit, tmp_path):
    import audit_dpp_hazards
    s = tmp_path / (unit + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    assert "scratch_" not in isa
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "svae" in l]
    for kernel, count in (("hmm_filter_row_kernel", 16), ("hmm_filter_wide_kernel", 2),
                          ("hmm_draw_row_kernel", 16), ("hmm_draw_wide_kernel", 2)):
        assert sum(kernel in n for n in names) == count, (kernel, names)
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 36 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert spills and set(spills) == {"0"}, spills
    # the wide draw kernel's transposed matrix and its cumulative-sum line: KP KP + 128 doubles
    lds = sorted(int(l.split()[-1]) for l in isa.splitlines() if ".group_segment_fixed_size:" in l)
    assert lds[-1] == (64 * 64 + 128) * 8 and lds[-1] <= 64 * 1024
    n_dpp, findings = audit_dpp_hazards.audit(str(s))
    assert findings == [], findings[:5]
    assert n_dpp >= DPP_FLOOR, n_dpp
    flags = open(os.path.join(CSRC, "Makefile")).read()
    assert unit + ".o" in flags and unit.replace("hmm_", "") + ".s" in flags       # in OBJS and in the audit target
