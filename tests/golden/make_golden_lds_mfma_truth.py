"""Generates tests/golden/lds_mfma_truth_<n>_<form>_<draw>.npz: the 50-digit truth (oracle/lds_mp.py alone) of the LDS
E-step -- and, for the tile sizes, of the sampler on real noise and of the training VJP -- on the draws of
tests/_lds_mfma_truth.py, where the oracle takes seconds to minutes per evaluation (n = 64: ~20 s an E-step, ~1 min a
directional derivative): too long for a test, fine once.  CPU only, mpmath only, at most 16 processes.

Draws (rand_lds_natparam + rand_node_potentials, exactly symmetric blocks; seeds 0 .. 99), two per size and form:
  ill     the seed of largest cond(J22) whose fp64 restatement (oracle.lds_numpy.natural_lds_estep_general) stays within
          1e-9 of the truth on every statistics array -- candidates are tried by decreasing cond(J22), each against its own
          mp truth, and the first that meets the condition is taken;
  median  the seed nearest the median cond(J22) (the 51st of the 100, then the 52nd, the 50th, ...) on which the 1e-11 floor
          binds: the fp64 restatement within 1e-11 / 3 of the truth on every statistics array.  Only n = 128 per-step moves
          off the 51st (seed 90, ill-conditioned init block: kept as the fixture n128_perstep_s90, EXTRA_DRAWS).
  illinit the seed of largest cond(J0) under the ill draws' condition (n64_perstep_illinit, EXTRA_DRAWS; its stored `cond`
          is cond(J0)).
A fixture stores the seed, not the model: the tests regenerate the inputs and check them against the stored SHA-256.

Reproducibility: the mp arithmetic is deterministic, so on the same NumPy / LAPACK (which draw the inputs and choose
the seeds) and torch (whose fp64 autograd picks the coordinate directions) the files come out bit for bit; elsewhere the
stored hash says whether the inputs are the same, and then the truths agree to 1e-15.

    python tests/golden/make_golden_lds_mfma_truth.py [name ...]        (all 30 fixtures: ~7 min on 8 cores)
"""
import concurrent.futures as cf
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # the pool is the parallelism: idle BLAS / OpenMP threads of 16 processes starve the mp arithmetic

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _lds_mfma_truth as M  # noqa: E402
from oracle import lds_mp, lds_numpy  # noqa: E402

SEEDS = range(100)


def _truth(n, T, seed, form):
    """mp truth and the fp64 restatement's distance to it, per statistics array"""
    natparam, node = M.model(n, T, seed, form)
    truth = M._stats_arrays(*lds_mp.estep_mp(natparam, node))
    fp64 = M._distances(M._stats_arrays(*lds_numpy.natural_lds_estep_general(natparam, node)), truth)
    return truth, fp64


def task_select(n, T, form, kind):
    """-> seed, cond(J22), truth, fp64 distances, seeds rejected on the way"""
    conds = sorted((M.cond_J22(M.model(n, T, s, form)[0][1]), s) for s in SEEDS)
    rejected = []
    if kind.startswith("seed"):
        cond, seed = next(c for c in conds if c[1] == int(kind[4:]))
        truth, fp64 = _truth(n, T, seed, form)
        assert max(fp64.values()) <= M.RESTATEMENT_BOUND, (n, form, seed, fp64)
        return seed, cond, truth, fp64, rejected
    if kind == "illinit":       # by decreasing cond(J0), under the ill draws' condition
        conds = sorted((float(np.linalg.cond(M.model(n, T, s, form)[0][0][0])), s) for s in SEEDS)
    if kind == "median":
        mid = len(conds) // 2
        for k in sorted(range(len(conds)), key=lambda i: (abs(i - mid), -i)):
            cond, seed = conds[k]
            truth, fp64 = _truth(n, T, seed, form)
            if max(fp64.values()) <= M.MEDIAN_BOUND:
                return seed, cond, truth, fp64, rejected
            rejected.append((seed, cond, max(fp64.values())))
        raise AssertionError("no seed on which the floor binds", n, form)
    for cond, seed in reversed(conds):
        truth, fp64 = _truth(n, T, seed, form)
        if max(fp64.values()) <= M.RESTATEMENT_BOUND:
            return seed, cond, truth, fp64, rejected
        rejected.append((seed, cond, max(fp64.values())))
    raise AssertionError("no seed meets the condition", n, form)


def task_samples(n, T, seed, form):
    natparam, node = M.model(n, T, seed, form)
    messages, _ = lds_mp.filter_mp(natparam[0], natparam[1], node)
    return lds_mp.sample_on_messages_mp(messages, natparam[1], M.noise(seed, T, n))


def task_solve(n, T, seed, form, rhs):
    """Sigma rhs, Sigma the joint covariance: E[x] of the model with init h = 0 and node h = rhs"""
    (init, pair), node = M.model(n, T, seed, form)
    _, (_, _, E_node) = lds_mp.estep_mp(((init[0], np.zeros(n), 0.0), pair), (node[0], rhs))
    return E_node[1]


def task_jvp(n, T, seed, form, v):
    """d/ds of (lognorm, diag E[xx'], E[x], samples) along node J += s v"""
    natparam, node = M.model(n, T, seed, form)
    d = lds_mp.jvp_mp(lds_mp.inference_mp, (natparam, node, M.noise(seed, T, n)), (None, (v, None, None), None))
    return d[0], d[1][0], d[1][1], d[2]


def main(only):
    t0 = time.time()
    todo = [f for f in M.fixture_names() if not only or f[0] in only]
    todo.sort(key=lambda f: -f[2])                              # the long chains first
    fix, pending = {}, {}
    with cf.ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for name, kind, n, T, form, draw in todo:
            pending[pool.submit(task_select, n, T, form, draw)] = (name, "select", None)
        while pending:
            done, _ = cf.wait(list(pending), return_when=cf.FIRST_COMPLETED)
            for fut in done:
                name, what, k = pending.pop(fut)
                kind, n, T, form, draw = next(f[1:] for f in todo if f[0] == name)
                if what == "select":
                    seed, cond, truth, fp64, rejected = fut.result()
                    natparam, node = M.model(n, T, seed, form)
                    fx = dict(truth, n=n, T=T, seed=seed, form=form, cond=cond, sha256=M.input_hash(natparam, node))
                    fx.update(("fp64_" + key, v) for key, v in fp64.items())
                    fix[name] = {"fx": fx, "left": 0}
                    print("%-20s seed %3d cond %.1e fp64 %.1e rejected %s  [%.0f s]" % (
                        name, seed, cond, max(fp64.values()),
                        ["s%d %.1e %.1e" % r for r in rejected], time.time() - t0), flush=True)
                    if kind == "tile":
                        eps, cot = M.noise(seed, T, n), M.cotangents(seed, T, n)
                        g_l, g_d, g_x, g_s, dense = cot
                        gJ, _ = M.autograd_node_grads(natparam, node, eps, cot)
                        gJ0, _ = M.autograd_node_grads(natparam, node, eps, cot, sampler=False)
                        dirs = M.directions(gJ, dense)
                        fx.update(eps=eps, g_l=g_l, g_d=g_d, g_x=g_x, g_s=g_s, dirs=dirs, scale_J=float(np.abs(gJ).max()),
                                  scale_J_nosampler=float(np.abs(gJ0).max()))
                        jobs = [(pool.submit(task_jvp, n, T, seed, form, v), "jvp", i) for i, v in enumerate(dirs)]
                        jobs.append((pool.submit(task_solve, n, T, seed, form, g_x + 2 * g_d * truth["Enode_x"]), "solve", 0))
                        jobs.append((pool.submit(task_solve, n, T, seed, form, g_s.sum(1)), "solve", 1))
                        jobs.append((pool.submit(task_samples, n, T, seed, form), "samples", None))
                        fix[name].update(jvp=[None] * len(dirs), solve=[None, None], left=len(jobs))
                        for f, w, i in jobs:
                            pending[f] = (name, w, i)
                else:
                    slot = fix[name]
                    if what == "samples":
                        slot["fx"]["samples"] = fut.result()
                    else:
                        slot[what][k] = fut.result()
                    slot["left"] -= 1
                slot = fix[name]
                if slot["left"] == 0:
                    fx = slot["fx"]
                    if kind == "tile":
                        # d L / d node h = g_l E[x] + Sigma (g_x + 2 g_d * E[x]) [+ Sigma sum_s g_s: a sample is affine in
                        # (h, eps) and equals E[x] at eps = 0]
                        fx["grad_h_nosampler"] = fx["g_l"] * fx["Enode_x"] + slot["solve"][0]
                        fx["grad_h"] = fx["grad_h_nosampler"] + slot["solve"][1]
                        # <g, J v> per direction, the E-step's part and the sampler's
                        fx["jvp_estep"] = np.array([fx["g_l"] * float(d[0]) + float(np.sum(fx["g_d"] * d[1]))
                                                    + float(np.sum(fx["g_x"] * d[2])) for d in slot["jvp"]])
                        fx["jvp_sampler"] = np.array([float(np.sum(fx["g_s"] * d[3])) for d in slot["jvp"]])
                    np.savez(M.fixture_path(name), **fx)
                    print("%-20s written, %d bytes  [%.0f s]" % (name, os.path.getsize(M.fixture_path(name)),
                                                                  time.time() - t0), flush=True)


if __name__ == "__main__":
    main(set(sys.argv[1:]))
