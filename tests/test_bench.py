"""bench.py's plain run and its --dump-outputs: the line a plain run prints, the arrays it writes, and what those arrays
hold (the last timed step's E-step outputs of the headline workload, against the checker oracle/bench_parity uses)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_plan(B, T, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return types.SimpleNamespace(B=B, device=torch.device("cpu"), lognorm=r(B), E_init=r(B, n * n + n),
                                 E_pair=r(B, 3, n, n), E_node_diagxx=r(B, T, n), E_node_x=r(B, T, n),
                                 reduced=r(4 * n * n + n + 2))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_whole_batch_under_the_budget(tmp_path):
    plan = _fake_plan(6, 5, 3)
    bench.dump_outputs(plan, str(tmp_path))
    got = _load(str(tmp_path))
    assert sorted(got) == ["E_init", "E_node_diagxx", "E_node_x", "E_pair", "lognorm", "reduced_stats", "sequence_index"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["sequence_index"], np.arange(6))
    for name in ("lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x"):
        np.testing.assert_array_equal(got[name], getattr(plan, name).numpy())
    np.testing.assert_array_equal(got["reduced_stats"], plan.reduced.numpy())


def test_dump_outputs_seeded_sample_above_the_budget(tmp_path):
    """Over the budget: the same fixed rows of every per-sequence array, the same rows on every run, within the budget."""
    plan = _fake_plan(50, 40, 4)
    budget = 40000
    bench.dump_outputs(plan, str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(_fake_plan(50, 40, 4), str(tmp_path / "b"), budget=budget)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["sequence_index"].astype(int)
    assert 1 <= len(idx) < 50 and np.all(np.diff(idx) > 0) and idx[-1] < 50
    assert sum(x.nbytes for x in a.values()) <= budget
    for name in ("lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x"):
        np.testing.assert_array_equal(a[name], getattr(plan, name).numpy()[idx])
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])


@pytest.mark.gpu
def test_plain_bench_run_and_its_dumped_outputs(tmp_path):
    """A plain run times the headline only (no parity gate, CPU baseline or extra configurations), honours --steps, and
    --dump-outputs writes the last timed step's outputs: checked against the reference's E-step (oracle/bench_parity) on
    the inputs bench.py generates, and against the batch statistics the step reduced."""
    from svae_amd.lds.synthetic_data import rand_node_potentials
    from oracle import bench_parity
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "sequences/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - line["config"]["sequences_per_gpu"] / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not {"parity", "extra", "cpu_baseline"} & set(line)

    got = _load(d)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    T, n, B = bench.WORKLOADS["lds10"]
    np.testing.assert_array_equal(got["sequence_index"], np.arange(B))
    assert got["E_node_x"].shape == (B, T, n) and got["E_pair"].shape == (B, 3, n, n)
    # the batch statistics of the step: [sum E_init | sum E_pair | sum lognorm | B]
    want = np.concatenate([got["E_init"].sum(0), got["E_pair"].sum(0).ravel(), [got["lognorm"].sum(), B]])
    np.testing.assert_allclose(got["reduced_stats"], want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
    # the outputs of a few sequences against the checker, on the inputs bench.measure generates (rank 0)
    init, pair = bench.bench_natparam(n)
    node_J, node_h = rand_node_potentials((B, T, n), np.random.default_rng(1000))
    idx = np.array([0, 137, B - 1])
    snap = dict(index=idx, init_J=init[0], init_h=init[1], init_logZ=init[2], J11=pair[0], J12=pair[1], J22=pair[2],
                logZ_pair=pair[3], node_J=node_J[idx], node_h=node_h[idx],
                **{k: got[k][idx] for k in ("lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x")})
    path = str(tmp_path / "snap.npz")
    np.savez(path, **snap)
    out = bench_parity.check(path)
    assert out["max_rel"] < bench.PARITY_TOL, out
