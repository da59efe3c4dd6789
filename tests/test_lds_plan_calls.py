"""Characterisation of the host side of the LDS ABI (svae_amd/lds/lds_inference.py): every library call LDSEStepPlan
and the autograd nodes on top of it make -- symbol, integer arguments, which buffer each pointer argument is -- and the
state the plan shows after every method, recorded against a stub library on CPU tensors and compared, exactly, with
tests/golden/lds_plan_calls.json.  No GPU, no built library: `_lib.load` and `_lib.current_stream` are monkeypatched.

The stub answers the size queries (`*_bytes`, `*_doubles`) from a table by symbol name, `svae_lds_inference_is_lean` with
what the scenario sets, and appends one trace entry for every other symbol: [name, arguments...] with integers and floats
verbatim and pointers as "null", "stream", the name of the scenario's tensor, "plan.<buffer>" (+ byte offset inside one),
"ret..." for a tensor the method returned, or "?".

`python tests/test_lds_plan_calls.py --record` rewrites the golden file (the project's own output; it changes only when the
calls are MEANT to change).  Not driven here, because they need a device: the two-stream forward and the backward pass of
lds_large.LDSInferenceLarge (16 <= n <= 64 with gradients or samples), the wait on a helper-stream event in `launch`, and the
wrappers that look for a CUDA device (natural_lds_estep_general and friends, dense node potentials through
lds_inference_differentiable); the GPU suite runs those.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from svae_amd import _lib                                    # noqa: E402
from svae_amd.lds import lds_inference as li                 # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lds_plan_calls.json")
STREAM = 0x57AE40
F64 = torch.float64
SIZES = {"svae_lds_workspace_bytes_ex": 8000, "svae_lds_xl_workspace_bytes": 8800,
         "svae_lds_ragged_workspace_bytes": 12000, "svae_lds_ragged_perstep_workspace_bytes": 16000,
         "svae_lds_vjp_workspace_bytes": 2400, "svae_lds_param_vjp_workspace_bytes": 3200,
         "svae_lds_tile_sigma_offset_bytes": 4000, "svae_lds_tile_vjp_workspace_doubles": 700}
PLAN_BUFFERS = ("ws", "lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x", "info", "reduced", "reduced_ragged",
                "vjp_ws", "param_ws", "_vjp_ws", "_lengths")
OUTPUTS = ("lognorm", "E_init", "E_pair", "E_node_diagxx", "E_node_x")


class Stub(object):
    """Stands in for the ctypes handle of libsvae_hip.so: sizes from SIZES, everything else recorded, return code 0."""

    def __init__(self, run):
        self.run, self.lean, self.sizes = run, 0, dict(SIZES)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if "_bytes" in name or name.endswith("_doubles"):
            return lambda *a: self.sizes.get(name, 1024)
        if name == "svae_lds_inference_is_lean":
            return lambda *a: self.lean

        def call(*a):
            self.run.trace.append([name] + [self.run.describe(x) for x in a])
            return 0
        call.__name__ = name
        return call


class Run(object):
    """One scenario: a stub library, a plan on the CPU, named input tensors and the trace."""

    def __init__(self, mp, B, T, n, **plan_kw):
        self.stub, self.trace, self.named = Stub(self), [], {}
        mp.setattr(_lib, "load", lambda: self.stub)
        mp.setattr(_lib, "current_stream", lambda device: ctypes.c_void_p(STREAM))
        self.B, self.T, self.n = B, T, n
        self.plan = li.LDSEStepPlan(B, T, n, device="cpu", **plan_kw)
        self._outs = [getattr(self.plan, k) for k in OUTPUTS]

    # ---- tensors of the scenario
    def t(self, name, *shape, **kw):
        x = torch.zeros(*shape, dtype=kw.get("dtype", F64))
        if len(shape) >= 2 and shape[-1] == shape[-2] and x.dtype == F64:
            x += torch.eye(shape[-1], dtype=F64)               # (a well-conditioned block: the host condition guard stays off)
        self.named[name] = x
        return x

    def model(self, inhomog=False, pair_batched=False, init_batched=False, logZ=False):
        """The ten positional tensors of launch / infer / filter in the layout asked for."""
        B, T, n = self.B, self.T, self.n
        li_ = (B,) if init_batched else ()
        lp = ((B, T - 1) if pair_batched else (T - 1,)) if inhomog else ()
        out = [self.t("init_J", *li_, n, n), self.t("init_h", *li_, n), self.t("init_logZ", *(li_ or (1,))),
               self.t("J11", *lp, n, n), self.t("J12", *lp, n, n), self.t("J22", *lp, n, n),
               self.t("logZ_pair", *(lp or (1,))), self.t("node_J", B, T, n), self.t("node_h", B, T, n)]
        return tuple(out) + ((self.t("node_logZ", B, T),) if logZ else (None,))

    def lengths(self, values=(5, 2, 3)):
        x = torch.tensor(list(values), dtype=torch.int32)
        self.named["lengths"] = x
        return x

    # ---- pointers -> labels
    def _known(self):
        for name, x in self.named.items():
            yield name, x
        for k in PLAN_BUFFERS:
            x = getattr(self.plan, k, None)
            if isinstance(x, torch.Tensor):
                yield "plan." + k, x

    @staticmethod
    def _lookup(addr, pairs):
        inside = None
        for name, x in pairs:
            lo = x.data_ptr()
            if lo == 0:
                continue
            if addr == lo:
                return name
            if inside is None and lo < addr < lo + x.numel() * x.element_size():
                inside = "%s+%d" % (name, addr - lo)
        return inside

    def describe(self, x):
        if x is None:
            return "null"
        if isinstance(x, ctypes.c_void_p):
            if x.value is None:
                return "null"
            if x.value == STREAM:
                return "stream"
            return self._lookup(x.value, self._known()) or ("?", x.value)      # (resolved once the method has returned)
        if isinstance(x, (bool, int, float)):
            return x
        return "<%s>" % type(x).__name__

    @staticmethod
    def _flat(x, path):
        if isinstance(x, torch.Tensor):
            yield path, x
        elif isinstance(x, (tuple, list)):
            for i, y in enumerate(x):
                for item in Run._flat(y, "%s[%d]" % (path, i)):
                    yield item

    def _resolve(self, first, ret):
        pairs = list(self._known()) + list(self._flat(ret, "ret"))
        for entry in self.trace[first:]:
            for i, a in enumerate(entry):
                if isinstance(a, tuple):
                    entry[i] = self._lookup(a[1], pairs) or "?"

    # ---- one step of a scenario
    def state(self, what):
        p = self.plan
        outs = [getattr(p, k) for k in OUTPUTS]
        same = {k: ("same" if a is b else "new") for k, a, b in zip(OUTPUTS, outs, self._outs)}
        self._outs = outs
        self.trace.append({"after": what, "epoch": p.epoch, "lean": bool(getattr(p, "lean", False)),
                           "has_factor": bool(getattr(p, "has_factor", False)),
                           "has_cross": bool(getattr(p, "has_cross", False)),
                           "lengths_none": getattr(p, "_lengths", None) is None, "ws_bytes": p.ws_bytes,
                           "outputs": same})

    def do(self, what, fn, *args, **kw):
        """Call `fn`, label what it passed to the library (its return value included), record the plan's state."""
        first = len(self.trace)
        keep = kw.pop("_ret", True)
        ret = fn(*args, **kw)
        self._resolve(first, ret if keep else None)
        self.state(what)
        return ret

    def call(self, method, *args, **kw):
        return self.do(method, getattr(self.plan, method), *args, **kw)


SCENARIOS = {}


def scenario(fn):
    SCENARIOS[fn.__name__] = fn
    return fn


@scenario
def launch_plain(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model()
    r.call("launch", *m)
    r.call("launch", *m, keep_factor=True)
    r.call("launch", *m, keep_cross=True)
    r.call("launch", *m, keep_factor=True, keep_cross=True)
    m = r.model(logZ=True)
    r.call("launch", *m)
    r.call("reduce")
    r.call("fresh_outputs")
    r.call("launch", *m)
    return r.trace


@scenario
def launch_perstep(mp):
    r = Run(mp, 3, 5, 4, inhomog=True, pair_batched=True)
    r.call("launch", *r.model(inhomog=True), keep_factor=True, keep_cross=True)
    r.call("launch", *r.model(inhomog=True, pair_batched=True), True, True, True)
    r.call("fresh_outputs")
    return r.trace


@scenario
def launch_tile(mp):
    r = Run(mp, 3, 5, 20)
    m = r.model()
    r.call("launch", *m)
    r.call("launch", *m, keep_factor=True, keep_cross=True)
    r.call("launch", *m, half=1)
    r.call("launch", *m, half=2, keep_sigma=True)
    r.call("launch", *m, half=1, keep_sigma=True)
    r.call("launch", *m, keep_sigma=True)
    r.call("sample", r.t("eps", 3, 5, 2, 20))
    r.call("sample", r.t("eps20", 3, 5, 20, 20))
    r.call("reduce")
    return r.trace


@scenario
def tile_vjp_tail(mp):
    r = Run(mp, 3, 5, 20)
    m = r.model()
    r.call("vjp_tail", 2)
    r.call("vjp_tail", 2, pair_batched=True)
    r.call("launch", *m, half=1)
    r.call("launch", *m, half=2, keep_sigma=True)
    return r.trace


@scenario
def launch_xl(mp):
    r = Run(mp, 3, 5, 70)
    r.call("launch", *r.model())
    r.call("reduce")
    r2 = Run(mp, 2, 4, 70, inhomog=True, pair_batched=True)
    r2.call("launch", *r2.model(inhomog=True, pair_batched=True), pair_batched=True)
    return r.trace + r2.trace


@scenario
def launch_lengths(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model()
    L = r.lengths()
    r.call("launch", *m, lengths=L)
    r.call("reduce")
    r.call("launch", *m, lengths=[5, 2, 3], keep_factor=True)
    r.call("launch", *m, lengths=np.array([1, 5, 4]), keep_cross=True)
    r.call("launch", *m, lengths=L, keep_factor=True, keep_cross=True)
    g = (r.t("g_lognorm", 3), r.t("g_dxx", 3, 5, 4), r.t("g_x", 3, 5, 4))
    r.call("vjp", *g)
    r.call("vjp", *g, lengths=L)
    r.call("reduce")
    r.call("launch", *m)                                  # (a plain launch forgets the lengths)
    r.call("reduce")
    return r.trace


@scenario
def ragged_perstep(mp):
    r = Run(mp, 3, 5, 4, inhomog=True)
    L = r.lengths()
    m = r.model(inhomog=True)
    r.call("launch_ragged_perstep", *m, lengths=L)
    r.call("launch_ragged_perstep", *m, lengths=[5, 2, 3], keep_factor=True)
    mb = r.model(inhomog=True, pair_batched=True, init_batched=True, logZ=True)
    r.call("launch_ragged_perstep", *mb, lengths=L, pair_batched=True, init_batched=True)
    eps = r.t("eps", 3, 5, 2, 4)
    r.call("infer_ragged_perstep", *mb, lengths=L, pair_batched=True, init_batched=True, eps=eps)
    r.call("infer_ragged_perstep", *mb, lengths=L, pair_batched=True, init_batched=True, eps=eps, out=r.t("out", 3, 5, 2, 4))
    r.call("infer_ragged_perstep", *mb, lengths=L, pair_batched=True, init_batched=True)
    m = r.model(inhomog=True)
    r.call("infer_ragged_perstep", *m, lengths=L, eps=eps)
    r.call("launch", *m)
    return r.trace


@scenario
def infer_records(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model()
    eps = r.t("eps", 3, 5, 2, 4)
    r.call("infer", *m)
    r.call("infer", *m, eps=eps)
    r.call("infer", *m, eps=eps, out=r.t("out", 3, 5, 2, 4))
    r.call("infer", *m, eps=eps, keep_vjp=False)
    r.call("infer", *m, keep_vjp=False)
    r.stub.lean = 1
    r.call("infer", *m, eps=eps)
    r.call("vjp", r.t("g_lognorm", 3))                   # (lean: no factor record, the cross record alone serves the VJP)
    r.call("infer", *m, keep_vjp=False)
    r.stub.lean = 0
    r.call("infer", *m, eps=eps, lengths=r.lengths())
    r.call("infer", *m, lengths=[4, 4, 1], keep_vjp=False)
    r.call("infer", *m, eps=eps)
    r2 = Run(mp, 3, 5, 4, inhomog=True, pair_batched=True)
    r2.call("infer", *r2.model(inhomog=True, pair_batched=True, logZ=True), pair_batched=True, eps=r2.t("eps", 3, 5, 1, 4))
    return r.trace + r2.trace


@scenario
def filter_and_sample(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model()
    r.call("filter", *m)
    msgs = dict(J_pred=r.t("J_pred", 3, 5, 4, 4), h_pred=r.t("h_pred", 3, 5, 4), J_filt=r.t("J_filt", 3, 5, 4, 4),
                h_filt=r.t("h_filt", 3, 5, 4))
    r.call("filter", *m, **msgs)
    eps = r.t("eps", 3, 5, 2, 4)
    r.call("sample", eps)
    r.call("sample", eps, out=r.t("out", 3, 5, 2, 4))
    r.call("launch", *m, keep_factor=True)
    r.call("sample", r.t("eps20", 3, 5, 20, 4))
    return r.trace


def _cotangents(r, S, stats=False):
    B, T, n = r.B, r.T, r.n
    g = [r.t("g_lognorm", B), r.t("g_dxx", B, T, n), r.t("g_x", B, T, n), r.t("g_samples", B, T, S, n),
         r.t("eps", B, T, S, n), r.t("samples", B, T, S, n)]
    if stats:
        g += [r.t("g_E_init", B, n * n + n), r.t("g_E_pair", B, T - 1, 3, n, n)]
    return g


@scenario
def vjp_plain(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model()
    g = _cotangents(r, 2)
    r.call("launch", *m, keep_factor=True, keep_cross=True)
    r.call("vjp", *g)
    r.call("vjp", g[0])
    r.call("vjp", g[0], g_E_init=r.t("g_E_init", 3, 20))
    r.call("infer", *m, eps=g[4])
    r.call("vjp", *g)                                    # (OPT_INFER_RECORDS; S of the infer() call)
    r.call("vjp", g[0], g[1], g[2])
    r.call("infer", *m)
    r.call("vjp", g[0])
    return r.trace


@scenario
def vjp_chunked(mp):
    r = Run(mp, 3, 5, 4)
    r.call("launch", *r.model(), keep_factor=True, keep_cross=True)
    g = _cotangents(r, 20)
    r.call("vjp", *g)
    r.call("vjp", *g, param_out=True)
    r.call("vjp", *_cotangents(r, 16))
    return r.trace


@scenario
def vjp_perstep(mp):
    r = Run(mp, 3, 5, 4, inhomog=True, pair_batched=True)
    g = _cotangents(r, 2, stats=True)
    r.call("launch", *r.model(inhomog=True), keep_factor=True, keep_cross=True)
    r.call("vjp", *g)
    r.call("vjp", *g, param_out=True)
    r.call("launch", *r.model(inhomog=True, pair_batched=True), True, True, True)
    r.call("vjp", *g)
    r.call("vjp", *g, dense_out=r.t("dense", 3, 5, 4, 4))
    r.call("vjp", *g, param_out=True)
    r.call("infer", *r.model(inhomog=True, pair_batched=True), pair_batched=True, eps=g[4])
    r.call("vjp", *g, dense_out=r.t("dense", 3, 5, 4, 4))
    r.call("vjp", *g, param_out=True)
    return r.trace


@scenario
def vjp_params_homogeneous(mp):
    r = Run(mp, 3, 5, 4)
    g = _cotangents(r, 2)
    r.call("launch", *r.model(), keep_factor=True, keep_cross=True)
    r.call("vjp", *g, param_out=True)
    r.call("vjp", g[0], param_out=True)
    r0 = Run(mp, 0, 5, 4)                                # (an empty batch: the parameter gradients are zeroed on the host)
    r0.call("launch", *r0.model(), keep_factor=True, keep_cross=True)
    r0.call("vjp", r0.t("g_lognorm", 0), param_out=True)
    return r.trace + r0.trace


def _natparam(m):
    return ((m[0], m[1], m[2]), m[3:7])


def _differentiable(r, m, what, eps=None, grads=("node_J", "node_h"), **kw):
    """Forward through lds_inference_differentiable on r.plan, then backward of the sum of everything differentiable."""
    for k in grads:
        r.named[k].requires_grad_()
    nodes = (m[7], m[8]) + ((m[9],) if m[9] is not None else ())
    out = r.do(what + ".forward", li.lds_inference_differentiable, _natparam(m), nodes, eps=eps, plan=r.plan, **kw)
    flat = [x for _, x in Run._flat(out, "ret") if x.requires_grad]
    r.do(what + ".backward", lambda: sum(x.sum() for x in flat).backward(), _ret=False)
    return out


@scenario
def differentiable_plain(mp):
    r = Run(mp, 3, 5, 4)
    m = r.model(logZ=True)
    _differentiable(r, m, "plain", eps=r.t("eps", 3, 5, 2, 4), grads=("node_J", "node_h", "node_logZ"))
    _differentiable(r, r.model(), "no_samples")
    _differentiable(r, r.model(), "S20", eps=r.t("eps20", 3, 5, 20, 4))      # (launch + sample, chunked VJP)
    r.stub.lean = 1
    _differentiable(r, r.model(), "lean", eps=r.t("eps", 3, 5, 2, 4))
    return r.trace


@scenario
def differentiable_pair_stats(mp):
    r = Run(mp, 3, 5, 4, inhomog=True)
    _differentiable(r, r.model(), "pair_stats_grad", eps=r.t("eps", 3, 5, 2, 4), pair_stats_grad=True)
    _differentiable(r, r.model(inhomog=True), "perstep", eps=r.t("eps", 3, 5, 2, 4))
    r2 = Run(mp, 3, 5, 4, inhomog=True, pair_batched=True)
    _differentiable(r2, r2.model(inhomog=True, pair_batched=True), "pair_batched")
    return r.trace + r2.trace


@scenario
def differentiable_natparam(mp):
    names = ("node_J", "node_h", "init_J", "init_h", "init_logZ", "J11", "J12", "J22", "logZ_pair")
    r = Run(mp, 3, 5, 4)
    _differentiable(r, r.model(), "natparam_grad", eps=r.t("eps", 3, 5, 2, 4), grads=names, natparam_grad=True)
    _differentiable(r, r.model(), "natparam_S20", eps=r.t("eps20", 3, 5, 20, 4), grads=names, natparam_grad=True)
    r2 = Run(mp, 3, 5, 4, inhomog=True)
    _differentiable(r2, r2.model(), "natparam_pair_stats", grads=names, natparam_grad=True, pair_stats_grad=True)
    _differentiable(r2, r2.model(inhomog=True), "natparam_perstep", grads=names[:5] + ("J12",), natparam_grad=True)
    r3 = Run(mp, 3, 5, 4, inhomog=True, pair_batched=True)
    _differentiable(r3, r3.model(inhomog=True, pair_batched=True), "natparam_pair_batched", grads=names, natparam_grad=True)
    return r.trace + r2.trace + r3.trace


@scenario
def differentiable_lengths(mp):
    r = Run(mp, 3, 5, 4)
    _differentiable(r, r.model(logZ=True), "lengths", eps=r.t("eps", 3, 5, 2, 4), grads=("node_J", "node_h", "node_logZ"),
                    lengths=r.lengths())
    _differentiable(r, r.model(), "lengths_list", lengths=[5, 5, 1])
    _differentiable(r, r.model(), "lengths_S20", eps=r.t("eps20", 3, 5, 20, 4), lengths=r.lengths())
    return r.trace


@scenario
def differentiable_tile_forward(mp):
    """16 <= n <= 64 through lds_large.LDSInferenceLarge, as far as it goes without a device: no gradient, no samples."""
    r = Run(mp, 3, 5, 20)
    m = r.model()
    r.do("tile.forward", li.lds_inference_differentiable, _natparam(m), (m[7], m[8]), plan=r.plan)
    return r.trace


def record_all():
    out = {}
    for name, fn in SCENARIOS.items():
        with pytest.MonkeyPatch.context() as mp:
            out[name] = fn(mp)
    return json.loads(json.dumps(out))


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_library_calls_and_plan_state(name, monkeypatch):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(golden) == sorted(SCENARIOS)
    got = json.loads(json.dumps(SCENARIOS[name](monkeypatch)))
    assert len(got) == len(golden[name])
    for i, (a, b) in enumerate(zip(got, golden[name])):
        assert a == b, "entry %d of %s" % (i, name)


# ---- every `raise` of LDSEStepPlan and of the autograd nodes' backward(): type, message, and nothing launched

def _launched(r, **kw):
    m = r.model(**{k: v for k, v in kw.items() if k in ("inhomog", "pair_batched")})
    r.plan.launch(*m, pair_batched=kw.get("pair_batched", False), keep_factor=kw.get("keep_factor", True),
                  keep_cross=kw.get("keep_cross", True), lengths=kw.get("lengths"))
    return m


def _raise_cases():
    """(name, (B, T, n), plan keywords, setup(r) -> callable that must raise, exception, part of the message)"""
    f = lambda *s: torch.zeros(*s, dtype=F64)
    eps = lambda r, S=2: f(r.B, r.T, S, r.n)
    P = dict(inhomog=True)
    PB = dict(inhomog=True, pair_batched=True)
    small, tile, xl = (3, 5, 4), (3, 5, 20), (3, 5, 70)

    def perstep(r, what="launch_ragged_perstep", **kw):
        m = r.model(inhomog=True)
        kw.setdefault("lengths", [5, 2, 3])
        return lambda: getattr(r.plan, what)(*m, **kw)

    def after(setup, then):
        def make(r):
            extra = setup(r)
            return lambda: then(r, extra)
        return make

    V, R = ValueError, RuntimeError
    return [
        ("init_n", small, {}, lambda r: (lambda: li.LDSEStepPlan(3, 5, 129, device="cpu")), V, "outside the supported range"),
        ("init_T", small, {}, lambda r: (lambda: li.LDSEStepPlan(3, 0, 4, device="cpu")), V, "need T >= 1 and B >= 0"),
        ("ragged_n", tile, {}, lambda r: (lambda: r.plan.launch(*r.model(), lengths=[5, 2, 3])), V,
         "launch(lengths=): latent dimension <= 15 (n = 20)"),
        ("ragged_inhomog", small, P, lambda r: (lambda: r.plan.infer(*r.model(inhomog=True), lengths=[5, 2, 3])), V,
         "infer(lengths=): pair parameters shared by the batch and by the steps"),
        ("ragged_pair_batched", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), pair_batched=True, lengths=[5, 2, 3])),
         V, "launch(lengths=): pair parameters shared by the batch"),
        ("lengths_shape", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), lengths=[5, 2])), V,
         "launch(lengths=): lengths must have shape (B,) = (3,), got (2,)"),
        ("lengths_float_tensor", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), lengths=f(3))), V,
         "launch(lengths=): an integer array or tensor"),
        ("lengths_float_array", small, {}, lambda r: (lambda: r.plan.infer(*r.model(), lengths=np.ones(3))), V,
         "infer(lengths=): an integer array or tensor"),
        ("perstep_homog_plan", small, {}, lambda r: perstep(r), V, "launch_ragged_perstep: a plan made with inhomog=True"),
        ("perstep_n", tile, P, lambda r: perstep(r, "infer_ragged_perstep"), V,
         "infer_ragged_perstep: latent dimension <= 15 (n = 20)"),
        ("perstep_no_lengths", small, P, lambda r: perstep(r, lengths=None), V, "launch_ragged_perstep: lengths (B,) is required"),
        ("perstep_layout", small, P, lambda r: perstep(r, pair_batched=True), V,
         "launch_ragged_perstep: J11 must be a contiguous float64 tensor of shape (3, 4, 4, 4) on cpu"),
        ("perstep_init_layout", small, P, lambda r: perstep(r, "infer_ragged_perstep", init_batched=True), V,
         "infer_ragged_perstep: init_J must be a contiguous float64 tensor of shape (3, 4, 4) on cpu"),
        ("perstep_lengths_shape", small, P, lambda r: perstep(r, lengths=[1, 2]), V,
         "launch_ragged_perstep(lengths=): lengths must have shape (B,) = (3,), got (2,)"),
        ("perstep_eps", small, P, lambda r: perstep(r, "infer_ragged_perstep", eps=f(3, 5, 2, 3)), V,
         "eps must be (B,T,S,n) with S >= 1"),
        ("xl_keep", xl, {}, lambda r: (lambda: r.plan.launch(*r.model(), keep_factor=True)), V,
         "E-step halves and kept records (half=, keep_*): latent dimension <= 64 (n = 70 runs the E-step only)"),
        ("xl_infer", xl, {}, lambda r: (lambda: r.plan.infer(*r.model())), V, "infer(): latent dimension <= 64"),
        ("xl_filter", xl, {}, lambda r: (lambda: r.plan.filter(*r.model())), V, "filter(): latent dimension <= 64"),
        ("xl_sample", xl, {}, lambda r: (lambda: r.plan.sample(eps(r))), V, "sample(): latent dimension <= 64"),
        ("xl_vjp", xl, {}, lambda r: (lambda: r.plan.vjp(f(3))), V, "vjp(): latent dimension <= 64"),
        ("xl_vjp_tail", xl, {}, lambda r: (lambda: r.plan.vjp_tail(2)), V, "vjp_tail(): latent dimension <= 64"),
        ("lengths_half", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), half=1, lengths=[5, 2, 3])), V,
         "launch(lengths=): no E-step halves / keep_sigma (latent dimension <= 15)"),
        ("lengths_keep_sigma", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), keep_sigma=True, lengths=[5, 2, 3])), V,
         "launch(lengths=): no E-step halves / keep_sigma"),
        ("half_small", small, {}, lambda r: (lambda: r.plan.launch(*r.model(), half=2)), V,
         "E-step halves: latent dimension > 15 only"),
        ("infer_tile", tile, {}, lambda r: (lambda: r.plan.infer(*r.model())), V,
         "infer(): latent dimension <= 15 (the tile path runs its stages separately)"),
        ("infer_eps", small, {}, lambda r: (lambda: r.plan.infer(*r.model(), eps=f(3, 5, 4))), V,
         "eps must be (B,T,S,n) with S >= 1"),
        ("infer_eps_S0", small, {}, lambda r: (lambda: r.plan.infer(*r.model(), eps=f(3, 5, 0, 4))), V,
         "eps must be (B,T,S,n) with S >= 1"),
        ("vjp_tail_small", small, {}, lambda r: (r.stub.sizes.update(svae_lds_tile_sigma_offset_bytes=0),
                                                 lambda: r.plan.vjp_tail(2))[1], V, "vjp_tail: latent dimension > 15 only"),
        ("sample_eps", small, {}, after(_launched, lambda r, m: r.plan.sample(f(2, 5, 2, 4))), V,
         "eps must be (B,T,S,n) with S >= 1"),
        ("sample_tile_first", tile, {}, lambda r: (lambda: r.plan.sample(eps(r))), R, "sample() needs a preceding launch()"),
        ("sample_ragged", small, {}, after(lambda r: _launched(r, lengths=[5, 2, 3]), lambda r, m: r.plan.sample(eps(r))), R,
         "sample(): the last launch had per-sequence lengths"),
        ("sample_lean", small, {}, after(lambda r: (setattr(r.stub, "lean", 1), r.plan.infer(*r.model(), eps=eps(r))),
                                         lambda r, m: r.plan.sample(eps(r))), R,
         "sample(): the last launch was infer() on lean records"),
        ("sample_first", small, {}, lambda r: (lambda: r.plan.sample(eps(r))), R,
         "sample() needs a preceding launch(..., keep_factor=True)"),
        ("sample_no_factor", small, {}, after(lambda r: _launched(r, keep_factor=False), lambda r, m: r.plan.sample(eps(r))), R,
         "sample() needs a preceding launch(..., keep_factor=True)"),
        ("vjp_lengths_plain", small, {}, after(_launched, lambda r, m: r.plan.vjp(f(3), lengths=[5, 2, 3])), V,
         "vjp(lengths=): the last launch of this plan had no per-sequence lengths"),
        ("vjp_lengths_first", small, {}, lambda r: (lambda: r.plan.vjp(f(3), lengths=[5, 2, 3])), V,
         "vjp(lengths=): the last launch of this plan had no per-sequence lengths"),
        ("vjp_lengths_shape", small, {}, after(lambda r: _launched(r, lengths=[5, 2, 3]),
                                               lambda r, m: r.plan.vjp(f(3), lengths=[5, 2])), V,
         "vjp(lengths=): lengths must have shape (B,) = (3,), got (2,)"),
        ("vjp_ragged_params", small, {}, after(lambda r: _launched(r, lengths=[5, 2, 3]),
                                               lambda r, m: r.plan.vjp(f(3), param_out=True)), V,
         "vjp() after a launch with lengths: no parameter gradients"),
        ("vjp_ragged_dense", small, {}, after(lambda r: _launched(r, lengths=[5, 2, 3]),
                                              lambda r, m: r.plan.vjp(f(3), dense_out=f(3, 5, 4, 4))), V,
         "vjp() after a launch with lengths: no parameter gradients"),
        ("vjp_ragged_stats", small, {}, after(lambda r: _launched(r, lengths=[5, 2, 3]),
                                              lambda r, m: r.plan.vjp(f(3), g_E_init=f(3, 20))), V,
         "vjp() after a launch with lengths: no cotangents of E_init / E_pair"),
        ("vjp_params_tile", tile, {}, after(lambda r: _launched(r, keep_factor=False, keep_cross=False),
                                            lambda r, m: r.plan.vjp(f(3), param_out=True)), V,
         "parameter gradients: latent dimension <= 15 (n = 20)"),
        ("vjp_params_lean", small, {}, after(lambda r: (setattr(r.stub, "lean", 1), r.plan.infer(*r.model())),
                                             lambda r, m: r.plan.vjp(f(3), param_out=True)), V,
         "parameter gradients need the full per-step records"),
        ("vjp_params_dense", small, PB, after(lambda r: _launched(r, **PB),
                                              lambda r, m: r.plan.vjp(f(3), dense_out=f(3, 5, 4, 4), param_out=True)), V,
         "param_out and dense_out are separate calls"),
        ("vjp_first", small, {}, lambda r: (lambda: r.plan.vjp(f(3))), R, "vjp() needs a preceding launch("),
        ("vjp_no_cross", small, {}, after(lambda r: _launched(r, keep_cross=False), lambda r, m: r.plan.vjp(f(3))), R,
         "vjp() needs a preceding launch("),
        ("vjp_no_factor", small, {}, after(lambda r: _launched(r, keep_factor=False), lambda r, m: r.plan.vjp(f(3))), R,
         "vjp() needs a preceding launch("),
        ("vjp_after_perstep_ragged", small, P, after(lambda r: perstep(r, keep_factor=True)(), lambda r, m: r.plan.vjp(f(3))), R,
         "vjp() needs a preceding launch("),
        ("vjp_lean_stats", small, {}, after(lambda r: (setattr(r.stub, "lean", 1), r.plan.infer(*r.model())),
                                            lambda r, m: r.plan.vjp(f(3), g_E_init=f(3, 20))), V,
         "lean records (infer() on a large homogeneous batch): no cotangents of E_init / E_pair"),
        ("vjp_pair_homog", small, {}, after(_launched, lambda r, m: r.plan.vjp(f(3), g_E_pair=f(3, 4, 3, 4, 4))), V,
         "a homogeneous plan keeps only the SUMMED pair statistics"),
        ("vjp_infer_S", small, {}, after(lambda r: r.plan.infer(*r.model(), eps=eps(r)),
                                         lambda r, m: r.plan.vjp(f(3), g_samples=eps(r, 3), eps=eps(r, 3), samples=eps(r, 3))), V,
         "vjp(): 3 sample cotangents for an infer() call that drew 2"),
        ("vjp_dense_lean", small, {}, after(lambda r: (setattr(r.stub, "lean", 1), r.plan.infer(*r.model())),
                                            lambda r, m: r.plan.vjp(f(3), dense_out=f(3, 5, 4, 4))), V,
         "dense node-potential cotangents: at most 16 sample cotangents, full records"),
        ("reduce_perstep", small, P, lambda r: (lambda: r.plan.reduce()), V, "reduce(): per-step pair statistics"),
        ("check_info", small, {}, lambda r: (r.plan.info.fill_(2), lambda: r.plan.check_info())[1], FloatingPointError,
         "LDS E-step: sequence 1 hit a non-positive pivot"),
    ]


@pytest.mark.parametrize("case", _raise_cases(), ids=lambda c: c[0])
def test_plan_raises_before_anything_is_launched(case, monkeypatch):
    name, (B, T, n), plan_kw, setup, exc, message = case
    r = Run(monkeypatch, B, T, n, **plan_kw)
    fails = setup(r)
    epoch, launched = r.plan.epoch, len(r.trace)
    with pytest.raises(exc) as err:
        fails()
    assert message in str(err.value)
    assert r.plan.epoch == epoch and len(r.trace) == launched


BACKWARD_MESSAGE = "LDSEStepPlan was launched again before backward(): the hand-off workspace of this forward pass is gone " \
                   "(use one plan per live autograd graph, or call backward before the next forward)"


@pytest.mark.parametrize("kind", ["nodes", "params", "lengths"])
def test_backward_after_another_launch_raises(kind, monkeypatch):
    r = Run(monkeypatch, 3, 5, 4)
    m = r.model()
    m[8].requires_grad_()
    kw = dict(natparam_grad=True) if kind == "params" else dict(lengths=[5, 2, 3]) if kind == "lengths" else {}
    out = li.lds_inference_differentiable(_natparam(m), (m[7], m[8]), eps=torch.zeros(3, 5, 2, 4, dtype=F64), plan=r.plan, **kw)
    r.plan.launch(*m)
    epoch, launched = r.plan.epoch, len(r.trace)
    with pytest.raises(RuntimeError) as err:
        out[0].sum().backward()
    assert BACKWARD_MESSAGE in str(err.value)
    assert r.plan.epoch == epoch and len(r.trace) == launched


def test_dense_backward_after_another_launch_raises(monkeypatch):
    """(the dense node's forward pass looks for a CUDA device: its backward is entered directly, on a stand-in context)"""
    import types
    r = Run(monkeypatch, 3, 5, 4, inhomog=True, pair_batched=True)
    r.plan.infer(*r.model(inhomog=True, pair_batched=True), pair_batched=True)
    ctx = types.SimpleNamespace(plan=r.plan, epoch=r.plan.epoch - 1, saved_tensors=(None, None), has_logZ=False,
                                has_samples=False)
    epoch, launched = r.plan.epoch, len(r.trace)
    with pytest.raises(RuntimeError) as err:
        li._LDSInferenceDense.backward(ctx, torch.zeros(3, dtype=F64), None, None, None, None)
    assert "the plan of this forward pass was launched again before backward()" in str(err.value)
    assert r.plan.epoch == epoch and len(r.trace) == launched


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_lds_plan_calls.py --record   (rewrites %s)" % GOLDEN)
    with open(GOLDEN, "w") as fh:
        rec = record_all()                                 # (one trace entry per line)
        fh.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(e, sort_keys=True) for e in rec[k]))
                                   for k in sorted(rec)) + "\n}\n")
    print("recorded %d scenarios into %s" % (len(SCENARIOS), GOLDEN))
