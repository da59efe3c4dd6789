"""The construction behind the ragged LDS kernels (svae_lds_ragged_*), restated on oracle/lds_numpy.py: a sequence of
length L inside a padded chain of T steps, exact under per-step pair parameters that are the real ones for the pairs
t <= L-2 and the decoupling set Q = (0, 0, -1/2 I, 0) for the pairs t >= L-1, with zero node potentials from step L on.
Helper of tests/test_lds_ragged_cpu.py and of the GPU tests (L = 1 reference)."""
import numpy as np

from oracle import lds_numpy


def two_slot_pair_params(pair, T, L):
    """(T-1,n,n) per-step pair parameters of the padded chain: slot(t) = real if t <= L-2 else Q"""
    J11, J12, J22, logZ = (np.asarray(x, float) for x in pair)
    n = J11.shape[0]
    real = np.arange(T - 1) <= L - 2
    pick = lambda a, q: np.where(real[:, None, None], a[None], q[None])
    return (pick(J11, np.zeros((n, n))), pick(J12, np.zeros((n, n))), pick(J22, -0.5 * np.eye(n)),
            np.where(real, float(logZ), 0.0))


def padded_nodes(node, L):
    """node potentials (T,n) [+ logZ (T)] with zeros from step L on"""
    out = [np.array(x, dtype=float, copy=True) for x in node]
    for x in out:
        x[L:] = 0.0
    return tuple(out)


def truncated_nodes(node, L):
    return tuple(np.asarray(x, float)[:L] for x in node)


def padded_run(natparam, node, L, eps=None):
    """E-step (and sampler) of the padded two-slot chain -> (lognorm, stats, samples | None); the pair statistics
    are the per-step blocks (T-1,n,n)"""
    init, pair = natparam
    T = np.asarray(node[1]).shape[0]
    nodes = padded_nodes(node, L)
    if T == 1:
        lognorm, stats = lds_numpy.natural_lds_estep_general((init, pair), nodes)
        messages, _ = lds_numpy.natural_filter_forward_general(init, pair, lds_numpy._canonical_node_params(nodes))
        pp = pair
    else:
        pp = two_slot_pair_params(pair, T, L)
        lognorm, stats = lds_numpy.natural_lds_estep_general((init, pp), nodes)
        messages, _ = lds_numpy.natural_filter_forward_general(init, pp, lds_numpy._canonical_node_params(nodes))
    samples = None if eps is None else lds_numpy.natural_sample_backward_general(messages, pp, eps)
    return lognorm, stats, samples


def truncated_run(natparam, node, L, eps=None):
    """the same on the sequence cut to its own L steps (homogeneous pair parameters: summed pair statistics)"""
    init, pair = natparam
    nodes = truncated_nodes(node, L)
    lognorm, stats = lds_numpy.natural_lds_estep_general((init, pair), nodes)
    samples = None
    if eps is not None:
        messages, _ = lds_numpy.natural_filter_forward_general(init, pair, lds_numpy._canonical_node_params(nodes))
        samples = lds_numpy.natural_sample_backward_general(messages, pair, eps[:L])
    return lognorm, stats, samples


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0
