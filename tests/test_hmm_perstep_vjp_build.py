"""CPU test of the ISA of the unit of the per-step HMM E-step's derivative (csrc/hmm_estep_perstep_vjp.hip): it compiles
for gfx950 into four kernels (groups of 8, 16, 32 and 64 lanes) without a private segment and without spills, the
largest LDS allocation is the formula of DESIGN 4.5i at K = 64 and leaves room for two workgroups per CU, and the DPP
hazard audit (tools/audit_dpp_hazards.py) has no findings."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svae_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "hmm_estep_perstep_vjp"


def _lds_bytes(K, W, groups):
    """per group the e tile and the V tile (K x KS, KS = K | 1), two broadcast vectors, and per wavefront the row factors
    and the partial (maximum, sum, weighted sum) triples: 2 K KS + 2 K + 4 W K doubles"""
    return groups * (2 * K * (K | 1) + 2 * K + 4 * W * K) * 8


def test_perstep_vjp_unit_compiles_without_scratch_and_without_dpp_hazards(tmp_path):
    import audit_dpp_hazards
    s = tmp_path / (UNIT + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "--cuda-device-only", "-S", os.path.join(CSRC, UNIT + ".hip"), "-o", str(s)],
                   check=True, cwd=CSRC)
    isa = s.read_text()
    names = [l.split()[-1] for l in isa.splitlines() if l.strip().startswith(".name:") and "svae" in l]
    assert sum("hmm_perstep_vjp_kernel" in n for n in names) == 4 and len(names) == 4, names
    sizes = [l.split()[-1] for l in isa.splitlines() if ".private_segment_fixed_size:" in l]
    assert len(sizes) == 4 and set(sizes) == {"0"}, sizes
    spills = [l.split()[-1] for l in isa.splitlines() if ".vgpr_spill_count:" in l]
    assert len(spills) == 4 and set(spills) == {"0"}, spills
    # LDS is sized at compile time for the widest K of each group width: 64 / G groups of K = G
    lds = sorted(int(l.split()[-1]) for l in isa.splitlines() if ".group_segment_fixed_size:" in l)
    assert lds == sorted(_lds_bytes(G, 1 if G <= 16 else 4, 64 // G) for G in (8, 16, 32, 64)), lds
    assert lds[-1] == _lds_bytes(64, 4, 1) == 75776 and lds[-1] <= 80 * 1024          # two workgroups per CU (160 KiB)
    n_dpp, findings = audit_dpp_hazards.audit(str(s))
    assert findings == [], findings[:5]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT + ".o" in mk and "estep_perstep_vjp.s" in mk             # in OBJS and in the audit target
    objs = next(l for l in mk.splitlines() if l.startswith("OBJS"))
    assert "$(BUILD)/" + UNIT + ".o" in objs
    audit = mk[mk.index("\naudit:"):mk.index("\nclean:")]
    assert audit.count("estep_perstep_vjp.s") == 2                       # compiled there and handed to the audit tool
