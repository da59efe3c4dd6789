"""The ORACLE of the LDS parameter-gradient tests pinned to extended precision (runs without a GPU).

tests/test_lds_param_grads_hip.py and tests/test_lds_param_grads_routes_hip.py hold the HIP kernels to the fp64 CPU
autograd of tests/_lds_large_torch.torch_estep.  Here that autograd itself is held to oracle/lds_mp: the derivative of
estep_mp along EVERY coordinate of every one of the seven natural-parameter arrays (jvp_mp, a central difference in 60
digits), contracted with the same random linear functional (`_loss`) of (lognorm, diag E[xx'], E[x][, samples]).
  * shapes n = 3, T = 4 and n = 2, T = 1, B = 2 sequences (so the sums over the batch are pinned too), layouts `homog`
    and `step`; at T = 1 the `step` layout has no pair block -- (0,n,n) arrays, empty gradients -- and the init
    gradients are still checked;
  * with and without samples at ZERO noise: x_t = c_t + G_t x_{t+1} is then E[x_t], and chol(P_t)^-T eps_t has no
    derivative, so the truth of the sample cotangent is <g_s, d E[x]> from the same jvp_mp evaluation;
  * init_J, J11 and J22 are symmetric-matrix arguments: the model is handed over exactly symmetric and the direction is
    E_ij + E_ji, against G_ij + G_ji of the autograd gradient (`_sym` of tests/test_lds_truth_hip.py);
  * metric: normwise per array, max|got - truth| / max|truth|; bound cond * 2^-53 * 100 with cond the larger of
    cond(init_J) and cond(J22) of the draw -- the estimate the MAX_COND comment of tests/test_lds_param_grads_hip.py
    reasons with (cond * eps * growth over the T n^2-term steps, taken as 100)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("mpmath")

import _lds_large_torch as lt  # noqa: E402
from oracle import lds_mp  # noqa: E402
from test_lds_param_grads_hip import NAMES, _inputs, _leaves, _loss  # noqa: E402  (the draws and the functional: imported)
from test_lds_truth_hip import _sym, _sym_blocks  # noqa: E402

B = 2
SYMMETRIC = ("init_J", "J11", "J22")


@functools.lru_cache(maxsize=None)
def _model(n, T, layout):
    """`_inputs`' draw with exactly symmetric init_J / J11 / J22 and zero noise for S = 1; at T = 1 in the `step` layout
    (which `_inputs` cannot draw: no pair block) the pair arrays are empty"""
    seed = 100 * n + 10 * T + (layout == "step")
    empty = T == 1 and layout == "step"
    init, pair, node, g, _ = _inputs(n, T, B, 1, "homog" if empty else layout, seed)
    if empty:
        pair = (np.zeros((0, n, n)), np.zeros((0, n, n)), np.zeros((0, n, n)), np.zeros(0))
    init = (_sym_blocks(init[0]), np.asarray(init[1], float), float(init[2]))
    pair = (_sym_blocks(pair[0]), np.asarray(pair[1], float), _sym_blocks(pair[2]), np.asarray(pair[3], float))
    cond = max([np.linalg.cond(init[0])] + [np.linalg.cond(x) for x in pair[2].reshape(-1, n, n)])
    return init, pair, node, g, float(cond)


def _autograd(n, T, layout, S):
    """the seven parameter gradients of torch_estep's fp64 autograd, as tests/test_lds_param_grads_hip.py's _oracle
    computes them"""
    init, pair, node, g, _ = _model(n, T, layout)
    cpu = torch.device("cpu")
    P = _leaves(init, pair, cpu)
    t = lambda x: torch.as_tensor(np.asarray(x, float), dtype=torch.float64)
    params = (P[0], P[1], P[2].reshape(1), P[3], P[4], P[5], P[6].reshape(-1))
    eps = torch.zeros((B, T, S, n), dtype=torch.float64) if S > 0 else None
    lognorm, dxx, ex, samples, _, _ = lt.torch_estep(params, t(node[0]), t(node[1]), eps=eps)
    _loss(g, (lognorm, dxx, ex, samples), S, cpu).backward()
    return [np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().copy() for x in P]


@functools.lru_cache(maxsize=None)
def _jacobian(n, T, layout):
    """{(array, coordinate): [(d lognorm, d diag E[xx'] (T,n), d E[x] (T,n)) per sequence]} along every coordinate
    direction -- E_ij + E_ji, i <= j, for the symmetric arrays -- by jvp_mp on estep_mp"""
    init, pair, node, _, _ = _model(n, T, layout)
    base = [init[0], init[1], np.asarray(init[2]), pair[0], pair[1], pair[2], pair[3]]
    out = {}
    for k, name in enumerate(NAMES):
        for c in np.ndindex(base[k].shape):
            if name in SYMMETRIC and c[-2] > c[-1]:
                continue
            v = np.zeros(base[k].shape)
            v[c] = 1.0
            if name in SYMMETRIC:
                v[c[:-2] + (c[-1], c[-2])] = 1.0
            d = [None] * 7
            d[k] = v
            direction = ((tuple(d[:3]), tuple(d[3:])), None)
            rows = []
            for b in range(B):
                dl, (_, _, dn) = lds_mp.jvp_mp(lds_mp.estep_mp, ((init, pair), (node[0][b], node[1][b])), direction)
                rows.append((float(dl), np.asarray(dn[0], float), np.asarray(dn[1], float)))
            out[(name, c)] = rows
    return out


@pytest.mark.parametrize("S", [0, 1])
@pytest.mark.parametrize("n,T,layout", [(3, 4, "homog"), (3, 4, "step"), (2, 1, "homog"), (2, 1, "step")])
def test_cpu_autograd_parameter_gradients_against_extended_precision(n, T, layout, S):
    init, pair, node, g, cond = _model(n, T, layout)
    bound = cond * 2.0 ** -53 * 100
    got = dict(zip(NAMES, _autograd(n, T, layout, S)))
    truth = {name: np.zeros_like(a) for name, a in got.items()}
    for (name, c), rows in _jacobian(n, T, layout).items():
        val = 0.0
        for b, (dl, ddxx, dx) in enumerate(rows):
            val += g["ln"][b] * dl + float(np.sum(g["dxx"][b] * ddxx)) + float(np.sum(g["x"][b] * dx))
            if S > 0:
                val += float(np.sum(g["s"][b, :, :S] * dx[:, None, :]))
        truth[name][c] = val
        if name in SYMMETRIC:
            truth[name][c[:-2] + (c[-1], c[-2])] = val
    worst = {}
    for name in NAMES:
        a = _sym(got[name]) if name in SYMMETRIC else got[name]
        t = truth[name]
        assert a.shape == t.shape, name
        if t.size == 0:                                   # T = 1 per step: no pair block, nothing to differentiate
            continue
        if T == 1 and name in ("J11", "J12", "J22", "logZ_pair"):
            assert not a.any() and not t.any(), name      # homogeneous blocks that no step reads: exact zeros
            continue
        worst[name] = float(np.max(np.abs(a - t)) / max(float(np.max(np.abs(t))), 1e-300))
    print("PGORACLE n=%d T=%d %s S=%d cond %.1e bound %.1e: " % (n, T, layout, S, cond, bound)
          + ", ".join("%s %.1e" % kv for kv in worst.items()))
    for name, d in worst.items():
        assert d <= bound, (name, d, bound)
