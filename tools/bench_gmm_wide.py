"""Timing of the GMM local step for latent dimensions 9..16 (svae_amd/csrc/gmm_wide.hip): the per-sweep fixed point at
(K, N, T) = (15, 10, 500), (15, 16, 1000), (64, 16, 8192) with its sweep counts, the sampler and the local VJP, and the
training step (run_inference_differentiable + backward) at N = 10, eager and replayed from one captured hipGraph.
Usage: python tools/bench_gmm_wide.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svae_amd import _lib                                        # noqa: E402
from svae_amd.distributions import expfam                        # noqa: E402
from svae_amd.models import gmm                                  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3          # us per call


def problem(K, N, T, seed=0):
    gen = torch.Generator().manual_seed(K + N)
    prior = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=0.05 / K, niw_conc=0.5, generator=gen))
    glob = tuple(x.to(DEV) for x in gmm.init_pgm_param(K, N, alpha=1., niw_conc=1., random_scale=3., generator=gen))
    rng = np.random.default_rng(seed)
    nJ = torch.as_tensor(-0.5 * np.log1p(np.exp(rng.standard_normal((T, N)))), device=DEV)
    nh = torch.as_tensor(3. * rng.standard_normal((T, N)), device=DEV)
    init = gmm.initialize_meanfield(T, K, DEV, torch.Generator(device=DEV).manual_seed(seed))
    return prior, glob, (nJ, nh), init


def main():
    for K, N, T in [(15, 10, 500), (15, 16, 1000), (64, 16, 8192)]:
        prior, glob, node, init = problem(K, N, T)
        lg, gg = expfam.dirichlet_expectedstats(glob[0]), expfam.niw_expectedstats(glob[1])
        o = gmm.meanfield_from_globals(lg, gg, node, init)
        us = timed(lambda: gmm.meanfield_from_globals(lg, gg, node, init, check=False), 10)
        it = int(o["iters"])
        print("GMM wide fixed point [%s] K=%d N=%d T=%d: %.1f us per call, %d sweeps, %.1f us per sweep"
              % (o["path"], K, N, T, us, it, us / max(it, 1)))
        S = 1
        eps = torch.randn(T, S, N, dtype=torch.float64, device=DEV)
        gs = torch.randn(T, S, N, dtype=torch.float64, device=DEV)
        gk = torch.ones(1, dtype=torch.float64, device=DEV)
        gJ, gh = torch.empty_like(node[0]), torch.empty_like(node[1])
        lib, p, st = _lib.load(), _lib.ptr, _lib.current_stream(DEV)
        smp = torch.empty(T, S, N, dtype=torch.float64, device=DEV)
        us_s = timed(lambda: lib.svae_gmm_wide_sample_f64(T, N, S, p(o["gaussian_natparam"]), p(eps), p(smp), st), 50)
        us_v = timed(lambda: lib.svae_gmm_wide_local_vjp_f64(
            T, N, K, S, p(lg), p(gg), p(node[0]), p(node[1]), p(o["gaussian_natparam"]), p(o["label_natparam"]), p(gk),
            p(eps), p(gs), p(gJ), p(gh), st), 50)
        print("  sampler S=1: %.1f us   local VJP (g_kl and g_samples): %.1f us" % (us_s, us_v))

    K, N, T, S = 15, 10, 500, 1
    prior, glob, node, init = problem(K, N, T, 1)
    eps = torch.randn(T, S, N, dtype=torch.float64, device=DEV)

    def step():
        a, b = node[0].clone().requires_grad_(True), node[1].clone().requires_grad_(True)
        s, _, _, lkl = gmm.run_inference_differentiable(prior, glob, (a, b), S, label_init=init, eps=eps, check=False)
        return torch.autograd.grad(lkl + s.sum(), [a, b])
    us_e = timed(step, 10)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    us_g = timed(g.replay, 20)
    print("GMM wide training step K=%d N=%d T=%d: eager %.1f us, graph replay %.1f us" % (K, N, T, us_e, us_g))


if __name__ == "__main__":
    main()
