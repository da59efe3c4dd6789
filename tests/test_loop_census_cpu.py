"""Instruction census of the headline kernel's loops (tools/loop_census.py) on the assembly hipcc generates for
svae_amd/csrc/lds_estep_n.hip at n = 10, compiled as tests/test_build_audit.py compiles it.  The two-ended E-step is a
latency chain, one wavefront per SIMD: every instruction inside its elimination and smoother loops is an issue slot.  The
assertions pin the schedule of the elimination step (lds_estep_twoend.hpp: elim_step, tools/gen_gj_asm.py) and ratchet
the loops' instruction counts: a change that makes a loop longer has to say so here."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import audit_dpp_hazards  # noqa: E402
import loop_census  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lds_estep_twoend_kernelILi10ELb0ELb1ELb0ELb0ELb1EE"     # <10, homogeneous, lean, S4>: bench.py's 512 x T=200, n=10
N = 10
# hot-path instructions per trip (tools/loop_census.py) of the finished build; the parent of this schedule had
# 356 / 364 per elimination step (HBM / LDS records; 358 by the count of the issue that asked for it, which took the
# loop's two skipped blocks slightly differently) and 665 / 663 per four smoother steps (166.25 per step)
ELIM_HBM_MAX, ELIM_LDS_MAX = 326, 335
SMOOTH4_MAX = 665


def test_census_tool_on_a_planted_loop(tmp_path):
    s = tmp_path / "k.s"
    s.write_text("other:\n\ts_nop 0\n\ts_endpgm\nmy_kernel:\n\tv_mov_b32_e32 v0, 0\n.LBB0_1:\n\ts_waitcnt lgkmcnt(0)\n"
                 "\t;;#ASMSTART\n\tv_fmac_f64_dpp v[2:3], v[4:5], v[6:7] row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t;;#ASMEND\n"
                 "\ts_cbranch_scc1 .LBB0_3\n; %bb.2:\n\tv_rcp_f64_e32 v[8:9], v[2:3]\n\ts_nop 0\n.LBB0_3:\n"
                 "\tds_read2_b64 v[10:13], v1 offset1:16\n\tglobal_store_dwordx2 v1, v[2:3], s[0:1]\n\ts_add_i32 s2, s2, 1\n"
                 "\tv_mov_b64_e32 v[4:5], v[10:11]\n\ts_cbranch_scc0 .LBB0_1\n\ts_endpgm\n")
    loops = loop_census.census(str(s), "my_kernel")
    assert len(loops) == 1
    lp = loops[0]
    assert (lp["label"], lp["total"], lp["hot"]) == (".LBB0_1", 10, 8)
    want = dict.fromkeys(loop_census.CLASSES, 0)
    want.update(s_waitcnt=1, dpp_fma=1, salu=3, lds=1, vmem=1, copy=1)
    assert lp["counts"] == want
    with pytest.raises(ValueError):
        loop_census.census(str(s), "no_such_kernel")


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("census") / "lds_estep_n.10.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DSVAE_N=%d" % N, "--cuda-device-only", "-S",
           os.path.join(ROOT, "svae_amd/csrc", "lds_estep_n.hip"), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lps = loop_census.census(str(out), HEADLINE)
    for lp in lps:
        print("%-12s total %4d hot %4d %s" % (lp["label"], lp["total"], lp["hot"], lp["counts"]))
    return lps


def _elim(loops):
    """the two elimination loops: the only ones with reciprocals; HBM records first (ten global stores per step)"""
    el = [lp for lp in loops if lp["counts"]["trans"] > 0]
    assert len(el) == 2, [lp["label"] for lp in loops]
    assert el[0]["counts"]["vmem"] >= N and el[1]["counts"]["vmem"] < N
    return el


def _dpp_lane(t):
    return int(t.split("row_newbcast:")[1].split()[0])


def test_elimination_loops_schur_stage_is_not_padded(loops):
    for lp in _elim(loops):
        ops = [t.split(None, 1)[0] for _, t in lp["body"]]
        schur = [i for i, (_, t) in enumerate(lp["body"]) if ops[i].startswith("v_fmac_f64_dpp") and _dpp_lane(t) >= N]
        assert len(schur) == 5 * N, len(schur)                          # J = 5 slots x N pivots rows
        inside = ops[schur[0]:schur[-1] + 1]
        assert "s_nop" not in inside, inside


def test_elimination_loops_wait_once_for_the_split_tile(loops):
    for lp in _elim(loops):
        first_pivot = next(i for i, (_, t) in enumerate(lp["body"]) if t.startswith("v_mov_b64_dpp") and _dpp_lane(t) == 0)
        waits = [t for _, t in lp["body"][:first_pivot] if t.startswith("s_waitcnt") and "lgkmcnt" in t]
        assert len(waits) <= 1, waits


def test_elimination_loops_cover_the_split_tile_reads(loops):
    """from the last ds_read2_b64 of a step to the first instruction that reads one of the registers the reads fill
    (around the back edge, on the hot path): at least 20 instructions"""
    for lp in _elim(loops):
        body = [t for _, t in lp["body"]]
        reads = [i for i, t in enumerate(body) if t.startswith("ds_read2_b64")]
        assert len(reads) == N // 2, reads
        filled = set()
        for i in reads:
            filled |= audit_dpp_hazards.regs(body[i].split(None, 1)[1].split(",")[0])
        order = body[reads[-1] + 1:] + body[:reads[0]]
        dist = None
        for d, t in enumerate(order):
            parts = t.split(None, 1)
            if len(parts) < 2 or parts[0].startswith("s_"):
                continue
            args = parts[1].split(",")
            srcs = args if parts[0].startswith(("v_fmac", "global_store", "ds_write")) else args[1:]
            if any(audit_dpp_hazards.regs(a) & filled for a in srcs):
                dist = d
                break
        assert dist is not None and dist >= 20, dist


def test_loop_totals_do_not_grow(loops):
    el = _elim(loops)
    assert el[0]["hot"] <= ELIM_HBM_MAX and el[1]["hot"] <= ELIM_LDS_MAX, (el[0]["hot"], el[1]["hot"])
    assert el[0]["counts"]["dpp_fma"] == el[1]["counts"]["dpp_fma"] == 150
    smooth = [lp for lp in loops if lp["counts"]["dpp_fma"] == 4 * 96]
    assert len(smooth) == 2, [(lp["label"], lp["counts"]["dpp_fma"]) for lp in loops]
    for lp in smooth:
        assert lp["hot"] <= SMOOTH4_MAX, lp["hot"]
