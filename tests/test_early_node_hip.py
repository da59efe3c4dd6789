"""The one-chain-per-wavefront E-step kernel (lds_estep_twoend.hpp, lds_estep_twoend_s4.hpp; up to 512 sequences,
n <= 10) is re-scheduled, never re-computed.  The compile-time switch SVAE_TE_EARLY_NODE, on by default, issues the loads
of the first node potentials with the prologue's batch of parameter loads instead of behind the prologue's set-up.
tests/_variants/libsvae_hip_s4ref.so (`make s4ref`, made by __graft_entry__.build()) is the library with the switch off.
Every output of svae_lds_estep_f64 -- lognorm, E_init, E_pair, E_node_diagxx, E_node_x and the status word -- must have
the SAME BYTES from both builds (NaN payloads and signed zeros included: the comparison is on the raw bytes), and the
default kernel must agree with the row-per-chain kernel, which the switch does not touch.

Shapes.  TS_SHORT takes every remainder of the smoother's straight-line steps and both parities of the meeting node;
TS_LOOP the lengths at which the smoother's four-step loop runs one or two trips; LONG the lengths at which the HBM
record ring starts below a window of LDS records (B = 2: the window holds ~60 records at n = 10) and the benchmark's own
length.  B = 2: LDS record window; 300: records in HBM; 513: the lean kernel without the second wavefront (not changed
here: it pins that the variant library differs in nothing else).

(Two more parts of the request this file was written for are not in the tree: the conditioning inside the split tile was
not built, and the unclamped record ring of the smoother loop was built, measured slower and taken out again, DESIGN
section 4.1.  The grid and the inputs that would have checked them -- exact zeros in J12, signed zeros and subnormals in the
node potentials, a launch behind another one -- are compared all the same: they cost nothing and pin the bytes for
whoever builds either.)"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "tests", "_variants", "libsvae_hip_s4ref.so")

NS = [1, 2, 3, 4, 5, 7, 8, 10]
TS_SHORT = [4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17]
TS_LOOP = [22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 33, 41]
BS = [2, 300, 513]
LONG = [(10, 140, 2), (10, 141, 2), (10, 200, 2), (10, 200, 300), (8, 200, 2), (7, 201, 300)]      # (n, T, B)
OPTIONS = ("twoend", "twoend_full")        # lean records (the default), full records through the options word
LOGNORM_REORDERED_NS = (3, 7)              # row-per-chain kernel only, see tests/test_twoend_schedule_hip.py
OUTPUTS = ("lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x", "info")


def _t(x):
    return torch.as_tensor(np.asarray(x, float), dtype=torch.float64, device="cuda:0")


def _model(n, T, B, seed=None):
    """(natparam, node potentials) of B sequences on the device"""
    from svae_amd.lds.synthetic_data import rand_lds_natparam, rand_node_potentials
    rng = np.random.default_rng(1000 * n + T if seed is None else seed)
    init, pair = rand_lds_natparam(n, rng)
    node = rand_node_potentials((B, T, n), rng, with_logZ=True)
    return (tuple(_t(x) for x in init), tuple(_t(x) for x in pair)), tuple(_t(x) for x in node)


_MODELS = {}


def _grid_model(n, T):
    """the LARGEST batch at (n, T); smaller batches are its head"""
    if (n, T) not in _MODELS:
        _MODELS[(n, T)] = _model(n, T, max(BS))
    return _MODELS[(n, T)]


def _launch(natparam, node, option="twoend", plan=None, infer=False):
    """-> {output: tensor} of one launch (clones: a plan's buffers are overwritten by its next launch)"""
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan, _prepare
    B, T, n = node[1].shape
    if plan is None:
        plan = LDSEStepPlan(B, T, n, "cuda:0", inhomog=natparam[1][0].dim() >= 3, options=_lib.KERNEL_OPTIONS[option])
    args = _prepare(natparam, node, plan)["args"]
    if infer:
        plan.infer(*args, keep_vjp=True)
    else:
        plan.launch(*args)
    torch.cuda.synchronize()
    return {"lognorm": plan.lognorm.clone(), "E_init": plan.E_init.clone(), "E_pair": plan.E_pair.clone(),
            "E_node_diagxx": plan.E_node_diagxx.clone(), "E_node_x": plan.E_node_x.clone(), "info": plan.info.clone()}


def _digest(out):
    return [hashlib.sha1(out[k].cpu().numpy().tobytes()).hexdigest() for k in OUTPUTS]


def _head(node, B):
    return tuple(x[:B].contiguous() for x in node)


def _special_models():
    """{name: (natparam, node)}: inputs on which a changed conditioning of the elimination step could show, n = 10"""
    n, T, B = 10, 13, 3
    out = {}
    (init, pair), node = _model(n, T, B, seed=77)
    # pair potentials of x' = A x + noise with diagonal noise covariance (synthetic_data.rand_lds_natparam's formulas):
    # J12 = (S^-1 A)' has an exact zero wherever A has one
    def pair_of(A):
        rng = np.random.default_rng(78)
        si = 1.0 / (0.5 + rng.random(n))
        temp = si[:, None] * A
        return (_t(-0.5 * A.T @ temp), _t(temp.T), _t(np.diag(-0.5 * si)), pair[3])
    A = 0.3 * np.random.default_rng(79).standard_normal((n, n)) / np.sqrt(n) + 0.5 * np.eye(n)
    A[2, :] = 0.0
    A[:, 5] = 0.0
    A[7, 1] = -0.0
    out["J12 with exact zeros"] = ((init, pair_of(A)), node)
    assert int((out["J12 with exact zeros"][0][1][1] == 0).sum()) >= 2 * n - 1
    out["J12 all zero"] = ((init, pair_of(np.zeros((n, n)))), node)
    h = node[1].clone()
    h[:, 0::3, :] = 0.0
    h[:, 1::3, ::2] = -0.0
    h[:, 2::3, 1::2] = 1e-310
    h[1, :, :] = -1e-310
    out["node_h zeros, negative zeros, subnormals"] = ((init, pair), (node[0], h, node[2]))
    Jn = node[0].clone()
    Jn[:, ::2, ::3] = -1e-300
    Jn[2, :, 4] = -1e-300
    out["node_J down to 1e-300"] = ((init, pair), (Jn, node[1], node[2]))
    Jb = node[0].clone()
    Jb[1, 4, :] = 50.0            # precision -2 J < 0 at one node of sequence 1: its pivots are not positive
    out["a pivot that is not positive"] = ((init, pair), (Jb, node[1], node[2]))
    return out


def _cases():
    """every launch both libraries run: (key, natparam, node, option, infer), in a fixed order"""
    for n in NS:
        for T in TS_SHORT + TS_LOOP:
            natparam, node = _grid_model(n, T)
            for B in BS:
                for opt in OPTIONS:
                    yield "n%d T%d B%d %s" % (n, T, B, opt), natparam, _head(node, B), opt, False
    for n, T, B in LONG:
        natparam, node = _model(n, T, B)
        yield "n%d T%d B%d long" % (n, T, B), natparam, node, "twoend", False
    natparam, node = _model(10, 9, 2)
    yield "training forward n10 T9 B2", natparam, node, "twoend", True
    for name, (natparam, node) in _special_models().items():
        yield "special: " + name, natparam, node, "twoend", False


def _all_digests():
    return {key: _digest(_launch(natparam, node, opt, infer=infer)) for key, natparam, node, opt, infer in _cases()}


def _dump(path):
    """(the variant library's process)"""
    with open(path, "w") as f:
        json.dump(_all_digests(), f)


@pytest.fixture(scope="module")
def digests(tmp_path_factory):
    """({key: digests} of the shipped library, of the variant library): ONE pass over the cases each"""
    assert os.path.exists(VARIANT), "tests/_variants/libsvae_hip_s4ref.so not built (python __graft_entry__.py)"
    path = str(tmp_path_factory.mktemp("s4ref") / "digests.json")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_early_node_hip as m; "
            "from svae_amd import _lib; assert _lib.LIB_PATH.endswith('libsvae_hip_s4ref.so'), _lib.LIB_PATH; "
            "m._dump(%r)" % (ROOT, os.path.join(ROOT, "tests"), path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SVAE_AMD_LIB=VARIANT), timeout=900,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(path) as f:
        ref = json.load(f)
    from svae_amd import _lib
    assert _lib.LIB_PATH.endswith("libsvae_hip.so"), _lib.LIB_PATH
    return _all_digests(), ref


def _differing(got, ref, select):
    assert sorted(got) == sorted(ref)
    keys = [k for k in got if select(k)]
    assert keys
    return ["%s: %s" % (k, [o for o, a, b in zip(OUTPUTS, got[k], ref[k]) if a != b]) for k in keys if got[k] != ref[k]]


@pytest.mark.parametrize("n", NS)
def test_bytes_equal_the_build_with_the_switches_off(digests, n):
    bad = _differing(*digests, lambda k: k.startswith("n%d " % n))
    assert not bad, bad[:20]


def test_training_forward_bytes_equal_the_build_with_the_switches_off(digests):
    bad = _differing(*digests, lambda k: k.startswith("training"))
    assert not bad, bad


def test_special_inputs_bytes_equal_the_build_with_the_switches_off(digests):
    got, ref = digests
    assert len([k for k in got if k.startswith("special")]) == 5
    bad = _differing(got, ref, lambda k: k.startswith("special"))
    assert not bad, bad


def _assert_same_bytes(a, b, what, reordered_lognorm=False):
    for key in OUTPUTS:
        x, y = a[key], b[key]
        if key == "lognorm" and reordered_lognorm:
            # ~ 2 T (n + 1) terms of magnitude <= max(1, |lognorm|) each, summed in two orders: a few ulp per term
            # (tests/test_twoend_schedule_hip.py: before and after every re-scheduling alike at n & 3 == 3)
            T, n = a["E_node_x"].shape[1:]
            bound = 4.0 * 2 * T * (n + 1) * 2.0 ** -53 * max(1.0, float(x.abs().max()))
            assert float((x - y).abs().max()) <= bound, (what, key, float((x - y).abs().max()), bound)
            continue
        same = torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 else torch.equal(x, y)
        assert same, "%s: %s differs" % (what, key)


@pytest.mark.parametrize("n", NS)
def test_default_kernel_equals_the_row_per_chain_kernel(n):
    shapes = [(n, T, B) for T in TS_SHORT + TS_LOOP for B in BS] + [s for s in LONG if s[0] == n]
    for _, T, B in shapes:
        if B in BS and T in TS_SHORT + TS_LOOP:
            natparam, node = _grid_model(n, T)
            node = _head(node, B)
        else:
            natparam, node = _model(n, T, B)
        a, b = _launch(natparam, node, "twoend"), _launch(natparam, node, "twoend_rpc")
        assert bool(torch.isfinite(a["E_node_x"]).all()), (n, T, B)
        _assert_same_bytes(a, b, "n=%d T=%d B=%d" % (n, T, B), reordered_lognorm=n in LOGNORM_REORDERED_NS)


def test_special_inputs_equal_the_row_per_chain_kernel():
    for name, (natparam, node) in _special_models().items():
        a, b = _launch(natparam, node, "twoend"), _launch(natparam, node, "twoend_rpc")
        if name == "a pivot that is not positive":
            # (what the two layouts leave in the outputs of a sequence that is not positive definite is not pinned
            #  anywhere; that both report it is)
            assert int(a["info"][0]) != 0 and int(b["info"][0]) != 0, (a["info"], b["info"])
        else:
            assert int(a["info"][0]) == 0, (name, a["info"])
            _assert_same_bytes(a, b, name)


def test_a_second_launch_of_a_plan_keeps_nothing_of_the_first():
    from svae_amd import _lib
    from svae_amd.lds.lds_inference import LDSEStepPlan
    for B in (2, 300):
        n, T = 10, 29
        (init, pair), node = _model(n, T, B, seed=5)
        (_, pair2), _ = _model(n, T, 1, seed=6)
        plan = LDSEStepPlan(B, T, n, "cuda:0", options=_lib.KERNEL_OPTIONS["twoend"])
        _launch((init, pair), node, plan=plan)
        again = _launch((init, pair2), node, plan=plan)
        _assert_same_bytes(again, _launch((init, pair2), node), "second launch, B=%d" % B)


def test_a_per_step_launch_behind_a_homogeneous_one_of_the_same_shape():
    n, T, B = 10, 13, 2
    (init, pair), node = _model(n, T, B, seed=8)
    rng = np.random.default_rng(9)
    scale = _t(1.0 + 0.05 * rng.random((T - 1, 1, 1)))
    per_step = tuple(x[None] * scale for x in pair[:3]) + (pair[3].reshape(1).repeat(T - 1),)
    fresh = _launch((init, per_step), node)
    _launch((init, pair), node)
    _assert_same_bytes(_launch((init, per_step), node), fresh, "per-step launch behind a homogeneous one")
