"""Instruction census (tools/loop_census.py) of what SVAE_TE_EARLY_NODE changes in the headline kernel, on the assembly
hipcc generates for svae_amd/csrc/lds_estep_n.hip at n = 10, compiled as tests/test_smoother_census_cpu.py compiles it.

Prologue (lds_estep_twoend.hpp): the first node potentials are loaded with the batch of parameter loads -- no load is
left between that batch and the elimination loop -- and the head of the HBM-record elimination loop still waits for the
prefetched potentials with vmcnt(N), the N hand-off stores behind them in flight, not for the stores.

(The conditioning inside the split tile, which the same request asked for, was not built, and its unclamped record ring
was measured slower and taken out, DESIGN section 4.1: the loops are pinned at the counts they had.)"""
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
SMOOTH4_MAX = 613           # both chains' loops: unchanged
ELIM_MAX = (326, 335)       # HBM-record loop, LDS-record loop: unchanged


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("census") / "lds_estep_n.10.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DSVAE_N=%d" % N, "--cuda-device-only", "-S",
           os.path.join(ROOT, "svae_amd/csrc", "lds_estep_n.hip"), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    loops = loop_census.census(str(out), HEADLINE)
    for lp in loops:
        print("%-12s total %4d hot %4d %s" % (lp["label"], lp["total"], lp["hot"], lp["counts"]))
    return str(out), loops


def test_smoother_loops_did_not_grow(listing):
    lps = [lp for lp in listing[1] if lp["counts"]["dpp_fma"] == 4 * 96]
    assert len(lps) == 2, [lp["label"] for lp in lps]          # chain A's wavefront, chain B's
    for lp in lps:
        assert lp["hot"] <= SMOOTH4_MAX and lp["hot"] == lp["total"], (lp["hot"], lp["total"])


def test_elimination_loops_did_not_grow_and_wait_for_the_potentials_only(listing):
    lps = [lp for lp in listing[1] if lp["counts"]["dpp_fma"] == 150]
    assert len(lps) == 2, [lp["label"] for lp in lps]
    # (the LDS-record loop hands over through LDS: nothing but the potentials is in flight at its head)
    for lp, most, stores in zip(lps, ELIM_MAX, (N, 0)):
        assert lp["hot"] <= most, (lp["label"], lp["hot"])
        first_wait = next(t for _, t in lp["body"] if t.startswith("s_waitcnt") and "vmcnt" in t)
        assert first_wait.split() == ["s_waitcnt", "vmcnt(%d)" % stores], first_wait


def test_first_node_potentials_are_loaded_with_the_prologue_batch(listing):
    path, loops = listing
    lines, _ = loop_census.kernel_lines(path, HEADLINE)
    first_loop = min(lp["first_line"] for lp in loops if lp["counts"]["dpp_fma"] == 150)
    front = [t for ln, t in lines if ln < first_loop]
    loads = [i for i, t in enumerate(front) if t.startswith("global_load")]
    waits = [i for i, t in enumerate(front) if t.startswith("s_waitcnt") and "vmcnt" in t]
    assert loads and waits
    # one batch: every load in front of the elimination loops is issued before the first wait for any of them
    assert loads[-1] < waits[0], (loads[-1], waits[0])
    # ... and the last two of them are still in flight behind the batch's last wait: the potentials are not waited for there
    assert min(int(re.search(r"vmcnt\((\d+)\)", front[i]).group(1)) for i in waits) >= 2, [front[i] for i in waits]
