"""Instruction census of the headline kernel's SMOOTHER loops (tools/loop_census.py) on the assembly hipcc generates for
svae_amd/csrc/lds_estep_n.hip at n = 10, compiled as tests/test_loop_census_cpu.py compiles it.  The smoother phase
(lds_estep_twoend_s4.hpp) runs one chain per wavefront, four steps per trip of its loop; every instruction in it is an
issue slot of a latency chain.  Its three product stages are one generated statement each (tools/gen_gj_asm.py:
smoother_stage), the record is read in place, and a step waits once for its three ring loads.  The assertions pin that
schedule and ratchet the count: a change that makes the loop longer has to say so here.

Before: 665 hot instructions per trip, 22 of them s_nop padding inside the product stages of one of the four unrolled
steps, 12 a second copy of the record in front of the preparation stage, 3 vmcnt waits per step."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_census  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADLINE = "lds_estep_twoend_kernelILi10ELb0ELb1ELb0ELb0ELb1EE"     # <10, homogeneous, lean, S4>: bench.py's 512 x T=200, n=10
N = 10
J, J1 = (N + 3) // 4, (N + 4) // 4
SMOOTH4_GOAL = 631          # 665 - 22 padding s_nop - 12 second-hop copies
SMOOTH4_MAX = 613           # the count reached (both chains' loops)
COPY_MAX = 26               # 12 ring copies, 12 W~ = 0, 2 at the back edge
MIN_LOADS_IN_FLIGHT = 9     # smallest vmcnt a wait inside the loop may ask for (the ring runs four records ahead)


@pytest.fixture(scope="module")
def smooth(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("census") / "lds_estep_n.10.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DSVAE_N=%d" % N, "--cuda-device-only", "-S",
           os.path.join(ROOT, "svae_amd/csrc", "lds_estep_n.hip"), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lps = [lp for lp in loop_census.census(str(out), HEADLINE) if lp["counts"]["dpp_fma"] == 4 * 96]
    for lp in lps:
        print("%-12s total %4d hot %4d %s" % (lp["label"], lp["total"], lp["hot"], lp["counts"]))
    assert len(lps) == 2, [lp["label"] for lp in lps]          # chain A's wavefront, chain B's
    return lps


def _stages(body):
    """[(first, last)] indices into `body` of the product stages: a stage's multiply-adds broadcast lanes 0, 0, .., 1, ..
    in ascending order, the next stage starts over at lane 0"""
    out, prev = [], None
    for i, (_, t) in enumerate(body):
        if not t.startswith("v_fmac_f64_dpp"):
            continue
        lane = int(t.split("row_newbcast:")[1].split()[0])
        if prev is None or lane < prev:
            out.append([i, i])
        out[-1][1] = i
        prev = lane
    return out


def test_stage_finder_on_a_planted_body():
    mac = lambda k: (0, "v_fmac_f64_dpp v[0:1], v[2:3], v[4:5] row_newbcast:%d row_mask:0xf bank_mask:0xf" % k)
    body = [mac(0), mac(0), mac(1), (0, "s_nop 0"), mac(1), (0, "ds_write_b64 v1, v[0:1]"), mac(0), mac(1)]
    assert _stages(body) == [[0, 4], [6, 7]]


def test_smoother_loops_reach_the_goal_and_do_not_grow(smooth):
    for lp in smooth:
        assert lp["hot"] <= SMOOTH4_GOAL, lp["hot"]
        assert lp["hot"] <= SMOOTH4_MAX, lp["hot"]
        assert lp["hot"] == lp["total"], (lp["hot"], lp["total"])          # no branch inside a trip
        assert lp["counts"]["copy"] <= COPY_MAX, lp["counts"]


def test_smoother_product_stages_are_not_padded(smooth):
    """twelve stages per trip -- W~ = S~ G~' (J1 x (N + 1) multiply-adds), the preparation (J x N), S~ = PiZ + G~ W~
    (J1 x (N + 1)), four times -- and nothing but multiply-adds between the first and the last of each"""
    for lp in smooth:
        st = _stages(lp["body"])
        ops = [t.split(None, 1)[0] for _, t in lp["body"]]
        sizes = [sum(1 for o in ops[a:b + 1] if o.startswith("v_fmac_f64_dpp")) for a, b in st]
        assert sizes == [J1 * (N + 1), J * N, J1 * (N + 1)] * 4, sizes
        for a, b in st:
            inside = ops[a:b + 1]
            assert "s_nop" not in inside, inside
            assert b - a + 1 == len([o for o in inside if o.startswith("v_fmac_f64_dpp")]), inside
        assert lp["counts"]["s_nop"] == 0, lp["counts"]


def test_smoother_loops_keep_the_ring_loads_in_flight(smooth):
    """a step waits ONCE for its three ring loads, and no wait inside the loop drains the ring: every vmcnt it asks for
    leaves at least nine loads (three records) in flight"""
    for lp in smooth:
        waits = [t for _, t in lp["body"] if t.startswith("s_waitcnt") and "vmcnt" in t]
        assert 1 <= len(waits) <= 4, waits
        for t in waits:
            k = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
            assert k >= MIN_LOADS_IN_FLIGHT, waits
        assert not any(t.startswith("flat_") for _, t in lp["body"])
