"""Long HMM sequences -- the regime the time-chunked routes exist for -- with their long-double truth
(oracle/hmm_longdouble.py) and the bounds the routes are held to.  TEST INFRASTRUCTURE, shared by tests/test_hmm_long_cpu.py
and tests/test_hmm_long_hip.py: problems are named by hashable keys and every truth / fp64-oracle solve is lru_cache'd, so
the ~1 s solves at T = 22 785 run once per session.

Keys (-> problem(key) = (init (K), pair (K,K) or (B,K,K), node (B,T,K), lengths (B))):
  ("parity", B, T, K, chunk, pair_batched)   _hmm_chunked_numpy.parity_problem, the same seeds
  ("range",)                                 long_range_batch()
  ("hostile",)                               hostile_long()
  ("ragged", B, T, K, lengths)               the shared-pair parity problem (chunk 0 in the seed) cut to `lengths`

THE BOUND FOR THE SCALED ROUTES (the chunked kernels, and the serial kernels where no sequence is redone): elementwise
    |got - truth| <= C_SCALED * T * 2^-53 * |truth|      for log Z, E_init, E_states and E_trans alike, no absolute floor
(the smallest marginal of these problems is 1.4e-11 and scaled arithmetic keeps relative accuracy).  C_SCALED is NOT taken
from a kernel: it is 8 x the worst ratio error / (T 2^-53) of the NumPy restatement of the chunked kernels
(_hmm_chunked_numpy.chunked_estep) against truth over LONG_SHAPES, measured on the CPU (RESTATEMENT_RATIO below);
test_hmm_long_cpu.py asserts the restatement stays under C_SCALED / 8, so the constant cannot drift from its measurement.
The factor 8 covers what the restatement does not share with the kernels: FMA contraction, the kernels' exp and reciprocal,
their two-accumulator sums.

THE BOUND FOR REDONE SEQUENCES (fp64 log space, "the reference's own arithmetic"): 8 x the error of oracle/hmm_numpy against
truth on the same input, computed in the test -- for E_states and for E_trans the worst absolute error over the array, held
elementwise; for log Z relative.  The comparator is the reference, never a kernel.  The oracle's outputs are fp64 numbers:
by rounding alone its measured error on an output lies anywhere between 0 and 2^-53 of that output (on two of the seven
hostile sequences of long_range_batch its log Z is the correctly rounded truth, 2e-17 and 7e-17 off), and an error below
one rounding says nothing about the arithmetic.  Each of the three errors is therefore taken as at least one rounding of
its output (redo_bound); on hostile_long every one is far above that and the floor plays no part.
"""
import functools

import numpy as np

import _hmm_chunked_numpy as C
from oracle import hmm_longdouble, hmm_numpy

LD = np.longdouble
EPS = 2.0 ** -53

# (B, T, K, chunk)
LONG_SHAPES = [
    (1, 141, 3, 2),         # 71 chunks: more than a wavefront has lanes
    (1, 4401, 2, 2),        # 2 201 chunks, the last of one step: 137 renormalisations of the scan's mantissa product
    (1, 12001, 2, 2),       # 6 001 chunks: WITHOUT the scan's every-16th renormalisation the product of its normalisers'
                            #               mantissas is 1e-473 (shared pair) / 1e-577 and underflows to log Z = -inf; at
                            #               4401 steps it is 1e-42 / 1e-205 and the renormalisation could be dropped unseen
    (2, 1030, 4, 4),        # 258 chunks
    (2, 769, 8, 256),       # the longest default chunk at the smallest T with a one-step last chunk
    (3, 5700, 5, 128),      # the library's own pick of 128; B C is no multiple of the four rows of a wavefront
    (1, 22785, 8, 256),     # the smallest T = 89 * 256 + 1 above the switch to 256: 90 chunks, a one-step last chunk
    (1, 22785, 16, 256),    # the same at K = 16
    (128, 500, 8, 32),      # the largest batch the default rule still chunks (shared pair only)
]
SHARED_ONLY = {(128, 500, 8, 32)}

# worst |restatement - truth| / (|truth| T 2^-53) over log Z, E_init, E_states, E_trans and the batch, measured on the CPU
# (test_hmm_long_cpu.py::test_restatement_against_truth prints them): (shared pair, (B,K,K) pair)
RESTATEMENT_RATIO = {
    (1, 141, 3, 2): (0.11, 0.08),
    (1, 4401, 2, 2): (0.01, 0.01),
    (1, 12001, 2, 2): (0.01, 0.01),
    (2, 1030, 4, 4): (0.03, 0.03),
    (2, 769, 8, 256): (1.96, 2.25),
    (3, 5700, 5, 128): (0.21, 0.18),
    (1, 22785, 8, 256): (0.11, 0.08),
    (1, 22785, 16, 256): (0.11, 0.11),
    (128, 500, 8, 32): (0.88, None),
}
WORST_RESTATEMENT_RATIO = 2.25       # (2, 769, 8, 256), (B,K,K) pair
C_SCALED = 18.0                      # = 8 * WORST_RESTATEMENT_RATIO


def parity_keys(shape):
    return [("parity", *shape, pb) for pb in ((False,) if shape in SHARED_ONLY else (False, True))]


RANGE_HOSTILE = (0, 63, 64, 65, 127, 128, 129)
RANGE_CHUNK = 8


def long_range_batch():
    """130 sequences built like _hmm_chunked_numpy.range_batch (K = 2, T = 40, chunk = 8, (B,K,K) pair parameters): its
    three hostile kinds -- a -inf transition, the -800 transition that the evidence pays for, node potentials at
    400 sigma -- sit at the ends of the ballot blocks of hmm_chunk_index_kernel (64 lanes), every other sequence is benign.
    -> init, pair (B,2,2), node (B,T,2), hostile (B) bool"""
    rng = np.random.default_rng(130)
    B, T, K = 130, 40, 2
    init = np.log(np.array([0.6, 0.4]))
    base = np.log(np.array([[0.7, 0.3], [0.2, 0.8]]))
    pair = np.stack([base] * B)
    node = rng.standard_normal((B, T, K))
    hostile = np.zeros(B, bool)
    for i, b in enumerate(RANGE_HOSTILE):
        hostile[b] = True
        if i % 3 == 0:
            pair[b, 1, 0] = -np.inf                     # state 1 absorbs
        elif i % 3 == 1:
            pair[b] = np.array([[0.0, -800.0], [-800.0, 0.0]])
            node[b] = 0.1 * rng.standard_normal((T, K))
            node[b, :19, 1] -= 5.0                      # state 0 until step 18 ...
            node[b, 19:, 0] -= 1000.0                   # ... then the evidence pays for the -800 transition
        else:
            node[b] = 400.0 * rng.standard_normal((T, K))
    return init, pair, node, hostile


def hostile_long():
    """one K = 2 sequence of T = 22 785 steps that leaves the range of every scaled route: the only way into the other
    state costs 800 nats, state 0 holds the first half (state 1 at -5 per step), then the evidence pays 1000 per step
    against state 0.  -> init (2), pair (2,2), node (1,T,2)"""
    rng = np.random.default_rng(22785)
    T, K = 22785, 2
    init = np.log(np.array([0.6, 0.4]))
    pair = np.array([[0.0, -800.0], [-800.0, 0.0]])
    node = 0.1 * rng.standard_normal((1, T, K))
    node[0, :T // 2, 1] -= 5.0
    node[0, T // 2:, 0] -= 1000.0
    return init, pair, node


HOSTILE_CHUNK = 256


@functools.lru_cache(maxsize=None)
def problem(key):
    """-> (init, pair, node (B,T,K), lengths (B)) of the problem `key` names, read-only"""
    kind = key[0]
    if kind == "parity":
        init, pair, node = C.parity_problem(*key[1:])
    elif kind == "range":
        init, pair, node, _ = long_range_batch()
    elif kind == "hostile":
        init, pair, node = hostile_long()
    elif kind == "ragged":
        _, B, T, K, lengths = key
        init, pair, node = C.parity_problem(B, T, K, 0, False)
    else:
        raise KeyError(key)
    lengths = np.array(key[4] if kind == "ragged" else [node.shape[1]] * node.shape[0])
    out = (init, pair, node, lengths)
    for x in out:
        x.setflags(write=False)
    return out


def sequence(key, b):
    """(init, pair (K,K), node (lengths[b], K)) of sequence b"""
    init, pair, node, lengths = problem(key)
    return init, (pair[b] if pair.ndim == 3 else pair), node[b, :lengths[b]]


def _freeze(res):
    lz, (ei, et, es) = res
    out = (np.asarray(lz), ei, et, es)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(key, b):
    """(logZ, E_init, E_trans, E_states) of sequence b in long double (the log-space recursion), read-only"""
    return _freeze(hmm_longdouble.hmm_estep(sequence(key, b)))


@functools.lru_cache(maxsize=None)
def truth_scaled(key, b):
    """the same from the second algorithm"""
    return _freeze(hmm_longdouble.hmm_estep_scaled(sequence(key, b)))


@functools.lru_cache(maxsize=None)
def oracle64(key, b):
    """the same from the fp64 log-space oracle (oracle/hmm_numpy.hmm_estep)"""
    with np.errstate(all="ignore"):
        return _freeze(hmm_numpy.hmm_estep(sequence(key, b)))


def rel_err(got, want):
    """worst elementwise |got - want| / |want| in long double (want has no zero where this is used); 0 for empty"""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    r = np.where((got == want), LD(0), r)        # 0 / 0: an exact zero met exactly
    return float(r.max()) if r.size else 0.0


def scaled_ratio(got, key, b):
    """worst |got - truth| / (|truth| T 2^-53) over the four outputs of sequence b -> (ratio, name of the worst output);
    got = (logZ, E_init, E_trans, E_states (>= lengths[b] rows)).  The bound is ratio <= C_SCALED."""
    want = truth(key, b)
    T = want[3].shape[0]
    errs = [rel_err(got[0], want[0]), rel_err(got[1], want[1]), rel_err(got[2], want[2]), rel_err(got[3][:T], want[3])]
    i = int(np.argmax(errs))
    return errs[i] / (T * EPS), ("logZ", "E_init", "E_trans", "E_states")[i]


def redo_errors(got, key, b):
    """(log Z relative, E_states worst absolute, E_trans worst absolute) error of `got` against truth"""
    want = truth(key, b)
    T = want[3].shape[0]
    return np.array([rel_err(got[0], want[0]), float(np.abs(np.asarray(got[3][:T], LD) - want[3]).max()),
                     float(np.abs(np.asarray(got[2], LD) - want[2]).max())])


def redo_bound(key, b):
    """the bound for a sequence redone in fp64 log space, in redo_errors' layout: 8 x the fp64 oracle's own errors on
    this sequence, each taken as at least one rounding of the output it is measured on (2^-53 relative on log Z, 2^-53 of
    the array's largest entry on E_states and E_trans)"""
    want = truth(key, b)
    floor = EPS * np.array([1.0, float(np.abs(want[3]).max()), float(np.abs(want[2]).max())])
    return 8.0 * np.maximum(redo_errors(oracle64(key, b), key, b), floor)


def restatement(key, b, chunk):
    """_hmm_chunked_numpy.chunked_estep of sequence b -> ((logZ, E_init, E_trans, E_states), flagged)"""
    lz, (ei, et, es), bad = C.chunked_estep(sequence(key, b), chunk)
    return (lz, ei, et, es), bool(bad)
