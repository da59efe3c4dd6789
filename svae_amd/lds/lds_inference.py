"""Host-side mirror of the reference's LDS E-step wrappers, running on MI355X.

Mirrors /root/reference/svae/lds/lds_inference.py:
  natural_lds_estep_general(natparam, node_params) -> (lognorm, expected_stats)   (:223-229)
  cython_natural_lds_estep_general                   (same contract, :232-237)
with the same argument meaning (NATURAL parameters, time-major, float64) and the same shape
checks / ValueError behaviour as `_canonical_node_params` (:65-82) and `_canonical_init_params`
(:62-63).  New relative to the reference: node potentials may carry a leading batch axis
(B, T, n) -- B conditionally independent sequences sharing (init, pair) parameters -- in which case
every output gains a leading B axis ("sum of per-sequence stats" semantics
are obtained with `reduce_stats`).

All arithmetic happens in libsvae_hip.so (svae_lds_estep_f64); this file only validates, lays out
buffers and launches.  No CPU fallback.
"""
import numpy as np
import torch

from .. import _lib

__all__ = ["LDSEStepPlan", "natural_lds_estep_general", "cython_natural_lds_estep_general",
           "natural_filter_forward_general", "natural_smoother_general", "natural_sample_backward",
           "natural_lds_sample", "cython_natural_lds_sample",
           "natural_lds_inference_general", "cython_natural_lds_inference_general", "reduce_stats",
           "lds_inference_differentiable"]


def _as_dev(x, device, graph=False):
    """float64, contiguous, on `device`; graph: a tensor stays in its autograd graph on the way (else detached)"""
    if isinstance(x, torch.Tensor):
        t = x if graph else x.detach()
    else:
        t = torch.as_tensor(x, dtype=torch.float64)   # (a bare python float would become float32)
    return t.to(device=device, dtype=torch.float64).contiguous()


def _find_device(tensors):
    """The device of the first CUDA tensor among `tensors` (host data mixed in is copied there); the current one if none."""
    for x in tensors:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _canonical_init_params(init_params, device, graph=False):
    """lds_inference.py:62-63: (J, h, sum of the remaining log-normaliser terms)."""
    J, h = _as_dev(init_params[0], device, graph), _as_dev(init_params[1], device, graph)
    logZ = sum(_as_dev(z, device, graph).reshape(()) for z in init_params[2:]) \
        if len(init_params) > 2 else torch.zeros((), dtype=torch.float64, device=device)
    return J, h, logZ.reshape(1).contiguous()


def _canonical_pair_params(pair_params, B, T, n, device, graph=False):
    """Shape checks and device tensors of pair_params = (J11, J12, J22, logZ): (n,n) blocks shared by all steps, per-step
    (T-1,n,n) or per-step, per-sequence (B,T-1,n,n) ones -> (J11, J12, J22, logZ flat, inhomog, pair_batched).
    graph: the tensors stay in their autograd graph (natparam_grad), where a shared logZ must be ONE number too."""
    J11, J12, J22 = (_as_dev(x, device, graph) for x in pair_params[:3])
    logZ_pair = _as_dev(pair_params[3], device, graph).reshape(-1)
    inhomog, pair_batched = J11.dim() >= 3, J11.dim() == 4
    want = {2: (n, n), 3: (T - 1, n, n), 4: (B, T - 1, n, n)}.get(J11.dim())
    if want is None or any(tuple(x.shape) != want for x in (J11, J12, J22)):
        raise ValueError("pair_params must be (n,n), (T-1,n,n) or (B,T-1,n,n)")
    if (inhomog or graph) and logZ_pair.numel() != (1 if not inhomog else B * (T - 1) if pair_batched else T - 1):
        raise ValueError("pair logZ must have one entry per " + ("pair block" if graph else "step"))
    return J11, J12, J22, logZ_pair, inhomog, pair_batched


_default_options = _lib.OPT_DEFAULT
_word_before_accurate = None     # the default word set_accurate_smoother(True) replaced; False puts it back


def set_default_options(options):
    """Kernel-selection word (svae_amd._lib.OPT_*) that plans created WITHOUT an explicit `options` take; returns
    the previous one.  Host-side convenience for the tests and A/B tools that run a whole suite through one
    kernel family -- the library itself holds no selection state: each plan passes its word with every call."""
    global _default_options, _word_before_accurate
    _word_before_accurate = None
    old, _default_options = _default_options, int(options)
    return old


def set_accurate_smoother(on=True):
    """Plans created without an explicit `options` word take the kernels whose smoothed moments (and the gradients through
    them) are accurate to cond * eps, like the reference's factor-and-solve, when `on`:
      * E-step: FULL per-step hand-off records (SVAE_OPT_TWOEND_FULL) instead of the two-ended kernels' lean `[P^-1 | c]`
        records, from which P^-1 J12 is rebuilt by multiplying with the explicit inverse every step (cond^2 * eps);
        + 19 % per step at 512 sequences of n = 10, + 79 % at 4096;
      * inference + VJP (n <= 10, <= 2 samples): the one-call kernels on `[chol(P)^-T | c]` records at EVERY batch size
        (SVAE_OPT_LEAN_ON; the default from 1025 sequences) -- factors of balanced magnitude: cond * eps; 1.7 instead of
        0.7 ms per forward + backward at 512 sequences.
    On a model with cond(J22) = 7.8e7 (the worst of 400 draws of the reference's rand_lds; exactly symmetric blocks),
    normwise from a 50-digit solve (tests/test_lds_truth_hip.py): E-step statistics 2.9e-10 instead of 1.3e-4, training
    forward 5.5e-10 instead of 1.3e-4, node gradients 2.8e-10 (J) / 3.8e-10 (h) instead of 7.1e-5 / 1.1e-4 -- the
    reference's own are 5.4e-10, 4.3e-10 and 1.1e-9 / 7.3e-10;
    on well-conditioned models 1e-12 either way ("Conditioning").  set_accurate_smoother(False) restores
    the word that the last set_accurate_smoother(True) replaced.  Returns the previous default word."""
    global _word_before_accurate
    acc = _lib.OPT_TWOEND_FULL | _lib.OPT_LEAN_ON
    saved = _word_before_accurate
    if on:
        old = set_default_options((_default_options & ~_lib.OPT_LEAN_OFF) | acc)
        _word_before_accurate = old if saved is None else saved
        return old
    if saved is not None:           # undo the last set_accurate_smoother(True): the word it replaced, bits it cleared included
        return set_default_options(saved)
    return set_default_options(_default_options & ~acc)


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))


def _ragged_precheck(natparam, node_params, lengths, what):
    """`lengths=` (per-sequence lengths of one batch): every limit of the ragged kernels as a ValueError, from shapes alone
    -- before anything touches the device.  -> (B, T, n)"""
    if _is_dense_nodes(node_params):
        raise ValueError("%s(lengths=): diagonal node potentials J, h of shape (B,T,n) only -- dense (B,T,n,n) ones are "
                         "folded into per-step pair parameters, which the ragged kernels do not take" % what)
    shp = _shape_of(node_params[1])
    if len(shp) != 3 or _shape_of(node_params[0]) != shp:
        raise ValueError("%s(lengths=): batched node potentials J, h of shape (B,T,n) -- one sequence has one length, T" % what)
    B, T, n = shp
    if n > _lib.LDS_MAX_N:
        raise ValueError("%s(lengths=): latent dimension <= %d (n = %d)" % (what, _lib.LDS_MAX_N, n))
    if len(_shape_of(natparam[1][0])) != 2:
        raise ValueError("%s(lengths=): pair parameters shared by the batch and by the steps, (n,n) blocks -- per-step "
                         "(T-1,n,n) or per-sequence (B,T-1,n,n) ones are not supported with lengths" % what)
    if _shape_of(lengths) != (B,):
        raise ValueError("%s(lengths=): lengths must have shape (B,) = (%d,), got %s" % (what, B, _shape_of(lengths)))
    return B, T, n


class LDSEStepPlan(object):
    """Pre-allocated buffers for repeated E-steps of one shape (B, T, n): the launch itself does no
    allocation, no host<->device copy and no synchronisation.  The sampler and the VJP read the
    workspace of the plan's LAST launch: a plan may be reused for a new forward pass only after the
    backward pass of the previous one (checked through `epoch`).  `options`: kernel-selection word passed with
    every call of this plan (svae_amd._lib.OPT_*, include/svae_hip.h SVAE_OPT_*; None = set_default_options)."""

    def __init__(self, B, T, n, device="cuda", inhomog=False, pair_batched=False, options=None):
        if not (1 <= n <= _lib.LDS_XL_MAX_N):
            raise ValueError("latent dimension n=%d outside the supported range (1..%d)"
                             % (n, _lib.LDS_XL_MAX_N))
        if T < 1 or B < 0:
            raise ValueError("need T >= 1 and B >= 0")
        self.lib = _lib.load()
        self.B, self.T, self.n, self.inhomog = B, T, n, bool(inhomog)
        self.options = _default_options if options is None else int(options)
        self.device = torch.device(device)
        f64 = dict(dtype=torch.float64, device=self.device)
        # (n > 15: the workspace also holds the re-packed pair parameters, one set per sequence if batched)
        workspace_bytes = self.lib.svae_lds_xl_workspace_bytes if self.xl else self.lib.svae_lds_workspace_bytes_ex
        self.ws_bytes = int(workspace_bytes(max(B, 1), T, n, int(self.inhomog), int(bool(pair_batched))))
        self.ws = torch.empty(self.ws_bytes // 8, **f64)
        self._new_outputs()
        self.info = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.reduced = torch.empty(4 * n * n + n + 2, **f64)
        # constants of the reference's statistic tuples (built once: no per-call allocation)
        self.ones_B = torch.ones(B, **f64)
        self.ones_BT = torch.ones(B, T, **f64)
        self.ones_pair = torch.ones(B, max(T - 1, 0), **f64) if self.inhomog \
            else torch.full((B,), float(T - 1), **f64)
        # buffers made on first use: the workspaces of vjp() and of its param_out, the batch sums of a ragged launch, and
        # (lds_large.py) the tile VJP's workspace and the event of work that still reads the hand-off on a helper stream
        self.vjp_ws = self.param_ws = self.reduced_ragged = self._vjp_ws = self._side_event = None
        # launch counter: the sampler / VJP read the workspace of the LAST launch, so an autograd node
        # remembers the launch it belongs to and refuses to run after the plan has been reused
        self.epoch = -1
        self._kept()             # (epoch 0: nothing launched, nothing kept)

    def _kept(self, J12=None, pair_batched=False, has_factor=False, has_cross=False, lean=False, infer_S=None, lengths=None,
              perstep=False):
        """What the launch that just succeeded left behind, all of it at once -- called after EVERY forward launch and from
        nowhere else, so that no field survives from the launch before.  has_factor / has_cross: the records `sample()` /
        `vjp()` read; lean: `infer()` kept lean records; infer_S: the number of samples `infer()` drew (it fixes the record
        format), None after every other launch; lengths: (B,) int32 device tensor while the records are ragged ones;
        perstep: ragged records of per-step pair parameters (the sweeps of svae_lds_ragged_perstep_vjp_f64 read them)."""
        self.epoch += 1
        self._perstep = bool(perstep)
        self.has_factor, self.has_cross, self.lean, self._infer_S = bool(has_factor), bool(has_cross), bool(lean), infer_S
        self._J12, self._pair_batched, self._lengths = J12, bool(pair_batched), lengths
        # E_pair's fourth entry after a ragged launch: the sequence's own number of pairs
        self.pair_counts = None if lengths is None else (lengths.clamp(1, self.T) - 1).to(torch.float64)

    def _new_outputs(self):
        f64 = dict(dtype=torch.float64, device=self.device)
        B, T, n = self.B, self.T, self.n
        self.lognorm = torch.empty(B, **f64)
        self.E_init = torch.empty(B, n * n + n, **f64)
        self.E_pair = torch.empty(B, max(T - 1, 0), 3, n, n, **f64) if self.inhomog else torch.empty(B, 3, n, n, **f64)
        self.E_node_diagxx = torch.empty(B, T, n, **f64)
        self.E_node_x = torch.empty(B, T, n, **f64)

    def _call(self, name, args):
        """The one way into the library's launching entry points: the return code is checked under the name called."""
        _lib.check(getattr(self.lib, name)(*args), name)

    def _forward(self, name, ints, model, outputs=None):
        """A forward entry point: its integers; the pointers of `model` -- the ten tensors of the model and what the entry
        takes behind them (lengths, eps, samples); then the end they all share, [five outputs | info | workspace, its
        size | stream] -- outputs: the statistics, or (filter) lognorm and the four forward messages."""
        if outputs is None:
            outputs = (self.lognorm, self.E_init, self.E_pair, self.E_node_diagxx, self.E_node_x)
        self._call(name, [*ints, *_lib.ptrs((*model, *outputs, self.info, self.ws)), self.ws_bytes,
                          _lib.current_stream(self.device)])

    def _grow_ws(self, need_bytes):
        if self.ws_bytes < need_bytes:
            self.ws = torch.empty(need_bytes // 8, dtype=torch.float64, device=self.device)
            self.ws_bytes = self.ws.numel() * 8

    def _checked_eps(self, eps):
        shape = eps.shape
        if len(shape) != 4 or shape[0] != self.B or shape[1] != self.T or shape[3] != self.n or shape[2] < 1:
            raise ValueError("eps must be (B,T,S,n) with S >= 1")
        return eps.to(device=self.device, dtype=torch.float64).contiguous()

    def live(self):
        """(B,T) bool: step t belongs to sequence b, t < lengths[b] (after a launch with per-sequence lengths)"""
        return torch.arange(self.T, device=self.device)[None, :] < self._lengths[:, None]

    def _ragged(self, lengths, what, pair_batched=False):
        """Checks of a launch with per-sequence lengths (ValueError before anything is launched) -> (B,) int32 device
        tensor (a host `lengths` is copied once, a device one used as it is); grows the workspace by the pair tables."""
        if self.n > _lib.LDS_MAX_N:
            raise ValueError("%s(lengths=): latent dimension <= %d (n = %d)" % (what, _lib.LDS_MAX_N, self.n))
        if self.inhomog or pair_batched:
            raise ValueError("%s(lengths=): pair parameters shared by the batch and by the steps, (n,n) blocks -- per-step "
                             "or per-sequence ones are not supported with lengths" % what)
        return self._ragged_lengths(lengths, what, self.lib.svae_lds_ragged_workspace_bytes)

    def _ragged_lengths(self, lengths, what, workspace_bytes):
        """The length handling of every ragged launch: shape / dtype checks, ONE copy of a host array (a device int32
        tensor is used as it is), and the workspace grown to `workspace_bytes(B, T, n)`."""
        if _shape_of(lengths) != (self.B,):
            raise ValueError("%s(lengths=): lengths must have shape (B,) = (%d,), got %s" % (what, self.B, _shape_of(lengths)))
        if not (isinstance(lengths, torch.Tensor) and lengths.device == self.device and lengths.dtype == torch.int32
                and lengths.is_contiguous()):
            if isinstance(lengths, torch.Tensor) and lengths.is_floating_point():
                raise ValueError("%s(lengths=): an integer array or tensor" % what)
            lengths = torch.as_tensor(np.asarray(lengths) if not isinstance(lengths, torch.Tensor) else lengths)
            if lengths.is_floating_point():
                raise ValueError("%s(lengths=): an integer array or tensor" % what)
            lengths = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        self._grow_ws(int(workspace_bytes(max(self.B, 1), self.T, self.n)))
        return lengths

    def _ragged_perstep(self, lengths, what, pair_batched, init_batched, tensors):
        """Checks of launch_ragged_perstep / infer_ragged_perstep (ValueError before anything is launched) -> lengths."""
        if not self.inhomog:
            raise ValueError("%s: a plan made with inhomog=True (per-step pair statistics (B,T-1,3,n,n))" % what)
        if self.n > _lib.LDS_MAX_N:
            raise ValueError("%s: latent dimension <= %d (n = %d)" % (what, _lib.LDS_MAX_N, self.n))
        if lengths is None:
            raise ValueError("%s: lengths (B,) is required" % what)
        B, T, n = self.B, self.T, self.n
        init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ = tensors
        lead_i = (B,) if init_batched else ()
        lead_p = (B, T - 1) if pair_batched else (T - 1,)
        want = [("init_J", init_J, lead_i + (n, n)), ("init_h", init_h, lead_i + (n,)),
                ("node_J", node_J, (B, T, n)), ("node_h", node_h, (B, T, n))]
        if init_batched:
            want.append(("init_logZ", init_logZ, (B,)))
        if T > 1:
            want += [("J11", J11, lead_p + (n, n)), ("J12", J12, lead_p + (n, n)), ("J22", J22, lead_p + (n, n)),
                     ("logZ_pair", logZ_pair, lead_p)]
        if node_logZ is not None:
            want.append(("node_logZ", node_logZ, (B, T)))
        for name, x, shape in want:
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != shape or x.dtype != torch.float64 \
                    or x.device != self.device or not x.is_contiguous():
                raise ValueError("%s: %s must be a contiguous float64 tensor of shape %s on %s" % (what, name, shape, self.device))
        return self._ragged_lengths(lengths, what, self.lib.svae_lds_ragged_perstep_workspace_bytes)

    def launch_ragged_perstep(self, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ=None,
                              lengths=None, pair_batched=False, init_batched=False, keep_factor=False):
        """The E-step with per-sequence lengths AND per-step pair parameters (svae_lds_ragged_perstep_estep_f64; a plan made
        with inhomog=True, n <= 15).  Pair parameters (T-1,n,n) / (T-1), or with pair_batched (B,T-1,n,n) / (B,T-1); the init
        potential (n,n), (n), (1), or with init_batched one per sequence, (B,n,n), (B,n), (B).  lengths (B,): as in `launch`.
        Per sequence b of length L the results are those of the sequence cut at L; E_pair[b, L-1:] and E_node_*[b, L:] are 0;
        pair parameters at t >= L-1 and node potentials at t >= L are never read.  `sample()` and `vjp()` cannot follow."""
        model = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ)
        lengths = self._ragged_perstep(lengths, "launch_ragged_perstep", pair_batched, init_batched, model)
        self._forward("svae_lds_ragged_perstep_estep_f64", (self.B, self.T, self.n, int(bool(pair_batched)),
                      int(bool(init_batched)), int(bool(keep_factor)), self.options), model + (lengths,))
        self._kept(J12, pair_batched, has_factor=keep_factor, lengths=lengths)       # (no cross moments: vjp() refuses)

    def infer_ragged_perstep(self, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ=None,
                             lengths=None, pair_batched=False, init_batched=False, eps=None, out=None, keep_vjp=False):
        """launch_ragged_perstep + the ragged sampler in one call (svae_lds_ragged_perstep_inference_f64).  eps (B,T,S,n) or
        None -> samples (0 at t >= lengths[b]; eps there is never read) or None.
        keep_vjp=True (svae_lds_ragged_perstep_inference_keep_f64): the same outputs, and the launch keeps the factor region
        and the cross moments, so that `vjp()` can follow -- with g_E_init / g_E_pair, without dense_out / param_out."""
        S = 0
        if eps is not None:
            eps = self._checked_eps(eps)
            S = eps.shape[2]
        model = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ)
        lengths = self._ragged_perstep(lengths, "infer_ragged_perstep", pair_batched, init_batched, model)
        if S and out is None:
            out = torch.empty_like(eps)
        if keep_vjp:
            self._forward("svae_lds_ragged_perstep_inference_keep_f64", (self.B, self.T, self.n, S, int(bool(pair_batched)),
                          int(bool(init_batched)), 1, self.options), model + (lengths, eps, out))
            self._kept(J12, pair_batched, has_factor=True, has_cross=True, lengths=lengths, perstep=True)
            return out if eps is not None else None
        self._forward("svae_lds_ragged_perstep_inference_f64", (self.B, self.T, self.n, S, int(bool(pair_batched)),
                      int(bool(init_batched)), self.options), model + (lengths, eps, out))
        self._kept(J12, pair_batched, has_factor=S > 0, lengths=lengths)
        return out if eps is not None else None

    @property
    def xl(self):
        """65 <= n <= 128: the E-step runs on svae_lds_xl_estep_f64, which keeps no record for a sampler or a VJP."""
        return self.n > _lib.LDS_TILE_MAX_N

    def _no_xl(self, what):
        if self.xl:
            raise ValueError("%s: latent dimension <= %d (n = %d runs the E-step only)" % (what, _lib.LDS_TILE_MAX_N, self.n))

    def launch(self, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h,
               node_logZ=None, pair_batched=False, keep_factor=False, keep_cross=False, half=0, keep_sigma=False,
               lengths=None):
        """Raw launch on the current stream.  All arguments: contiguous float64 device tensors.
        lengths (B,) int array / tensor (n <= 15, shared pair parameters): sequence b occupies steps 0 .. lengths[b]-1;
        svae_lds_ragged_estep_f64 -- statistics, records and gradients of every sequence are those of the sequence
        truncated to its length, everything at t >= lengths[b] is 0 and the inputs there are never used.
        half (16 <= n <= 64 only): 1 = the forward half of the E-step (filter, hand-off, lognorm), 2 = the backward half
        (smoother + statistics from the hand-off of a preceding half=1 launch); 0 = both.
        keep_sigma (16 <= n <= 64 only, after `vjp_tail`): the backward half leaves the smoothed covariances in the
        first section of the VJP workspace behind the hand-off (SVAE_KEEP_SIGMA), which saves the VJP its phase 0."""
        model = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ)
        keep = int(bool(keep_factor)) | (2 if keep_cross else 0)
        if lengths is not None:
            if half or keep_sigma:
                raise ValueError("launch(lengths=): no E-step halves / keep_sigma (latent dimension <= %d)" % _lib.LDS_MAX_N)
            lengths = self._ragged(lengths, "launch", pair_batched)
            self._forward("svae_lds_ragged_estep_f64", (self.B, self.T, self.n, 0, 0, keep, self.options), model + (lengths,))
            self._kept(J12, has_factor=keep_factor, has_cross=keep_cross, lengths=lengths)
            return
        if self.xl:
            # 65 <= n <= 128: E-step only; the plan's options word (kernel choice of the smaller paths) does not apply
            if half or keep_factor or keep_cross or keep_sigma:
                self._no_xl("E-step halves and kept records (half=, keep_*)")
            self._forward("svae_lds_xl_estep_f64", (self.B, self.T, self.n, int(self.inhomog), int(pair_batched), 0, 0), model)
            self._kept(J12, pair_batched)
            return
        if self._side_event is not None:   # work on a helper stream still reads the hand-off this launch overwrites (lds_large.py)
            torch.cuda.current_stream(self.device).wait_event(self._side_event)
            self._side_event = None
        small = self.n <= _lib.LDS_MAX_N
        if not small:
            # tile kernel: its hand-off always serves the sampler / VJP kernels (lds_large.py)
            keep = _lib.KEEP_SIGMA if (keep_sigma and half != 1) else 0
        options = self.options
        if half:
            if small:
                raise ValueError("E-step halves: latent dimension > %d only" % _lib.LDS_MAX_N)
            options |= _lib.OPT_TILE_FORWARD if half == 1 else _lib.OPT_TILE_BACKWARD
        self._forward("svae_lds_estep_f64", (self.B, self.T, self.n, int(self.inhomog), int(pair_batched), keep, options), model)
        self._kept(J12, pair_batched, keep_factor and small, keep_cross and small)

    def fresh_outputs(self):
        """New output tensors for the next launch (lognorm, E_init, E_pair, E_node_*): a caller that hands the outputs on
        -- the autograd node below -- returns them as they are instead of copying them out of buffers the next launch
        would overwrite (two of them are (B,T,n): 2 x 65 MB at 4096 x 200 x 10)."""
        self._new_outputs()

    def infer(self, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ=None,
              pair_batched=False, eps=None, out=None, keep_vjp=True, lengths=None):
        """E-step + backward sampler in ONE call (svae_lds_inference_f64 = cython_natural_lds_inference_general,
        lds_inference.py:196-202), keeping what `vjp()` needs.  eps (B,T,S,n) or None (no sampling) -> samples or None.
        For large homogeneous batches (n <= 10, S <= 2, B > 2048, or OPT_LEAN_ON) the library keeps LEAN per-step
        records (csrc/lds_lean_estep.hpp): the same results with a fifth of the hand-off traffic; `sample()` cannot
        follow such a launch (`self.lean`).  keep_vjp=False: forward values only -- no cross-moment record, and lean
        records then also serve per-step / per-sequence pair parameters; `vjp()` cannot follow.
        lengths (B,): per-sequence lengths as in `launch` (svae_lds_ragged_inference_f64: full records at every batch size,
        any number of samples); eps[b, lengths[b]:] is never used and the samples there are 0."""
        self._no_xl("infer()")
        if self.n > _lib.LDS_MAX_N:
            raise ValueError("infer(): latent dimension <= %d (the tile path runs its stages separately)" % _lib.LDS_MAX_N)
        S = 0
        if eps is not None:
            eps = self._checked_eps(eps)
            S = eps.shape[2]
            if out is None:
                out = torch.empty_like(eps)
        model = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ)
        keep_vjp = bool(keep_vjp)
        if lengths is not None:
            lengths = self._ragged(lengths, "infer", pair_batched)
            self._forward("svae_lds_ragged_inference_f64", (self.B, self.T, self.n, S, 0, 0, int(keep_vjp), self.options),
                          model + (lengths, eps, out))
            self._kept(J12, has_factor=keep_vjp or S > 0, has_cross=keep_vjp, lengths=lengths)
        else:
            self._forward("svae_lds_inference_f64", (self.B, self.T, self.n, S, int(self.inhomog), int(pair_batched),
                          int(keep_vjp), self.options), model + (eps, out))
            lean = bool(self.lib.svae_lds_inference_is_lean(self.B, self.T, self.n, S, int(self.inhomog), int(keep_vjp),
                                                            self.options))
            self._kept(J12, pair_batched, not lean and (keep_vjp or S > 0), keep_vjp, lean, infer_S=S)
        return out if eps is not None else None

    def vjp_tail(self, S, pair_batched=False):
        """16 <= n <= 64: the workspace of svae_lds_tile_vjp_f64 for S sample cotangents as a view BEHIND the hand-off in
        the plan's own buffer (grown if necessary -- call it before the launch whose hand-off the VJP will read), at
        svae_lds_tile_sigma_offset_bytes: where a launch with keep_sigma leaves the smoothed covariances."""
        self._no_xl("vjp_tail()")
        B, T, n = max(self.B, 1), self.T, self.n
        off = int(self.lib.svae_lds_tile_sigma_offset_bytes(B, T, n, int(self.inhomog), int(bool(pair_batched)))) // 8
        nws = int(self.lib.svae_lds_tile_vjp_workspace_doubles(B, T, n, S))
        if off == 0:
            raise ValueError("vjp_tail: latent dimension > %d only" % _lib.LDS_MAX_N)
        self._grow_ws((off + nws) * 8)
        return self.ws[off:off + nws]

    def filter(self, init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h,
               node_logZ=None, pair_batched=False, J_pred=None, h_pred=None, J_filt=None, h_filt=None):
        """Filter-only launch (svae_lds_filter_f64): lognorm, optional forward messages, and the hand-off
        `sample()` needs."""
        self._no_xl("filter()")
        model = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ)
        self._forward("svae_lds_filter_f64", (self.B, self.T, self.n, int(self.inhomog), int(pair_batched), self.options),
                      model, outputs=(self.lognorm, J_pred, h_pred, J_filt, h_filt))
        self._kept(J12, pair_batched, has_factor=True)

    def sample(self, eps, out=None):
        """Backward sampling from the messages of the last `launch(..., keep_factor=True)`.
        eps: (B,T,S,n) standard-normal draws -> samples (B,T,S,n)
        [natural_sample_backward, cython_lds_inference.pyx:310-355]."""
        self._no_xl("sample()")
        eps = self._checked_eps(eps)
        if self.n > _lib.LDS_MAX_N:
            # 16 <= n <= 64: noise-factor kernel + recursion kernel on the tile kernel's hand-off (lds_large.py)
            from .lds_large import sample_from_handoff
            if self.epoch == 0:
                raise RuntimeError("sample() needs a preceding launch()")
            return sample_from_handoff(self, eps)
        if self._lengths is not None:
            raise RuntimeError("sample(): the last launch had per-sequence lengths -- draw the samples in that call, infer(..., eps, lengths=)")
        if self.lean:
            raise RuntimeError("sample(): the last launch was infer() on lean records -- its samples were drawn there")
        if not self.has_factor:
            raise RuntimeError("sample() needs a preceding launch(..., keep_factor=True)")
        if out is None:
            out = torch.empty_like(eps)
        p = _lib.ptr
        self._call("svae_lds_sample_f64", (self.B, self.T, self.n, eps.shape[2], self.options, p(eps), p(out), p(self.ws),
                                           self.ws_bytes, _lib.current_stream(self.device)))
        return out

    def vjp(self, g_lognorm, g_E_node_diagxx=None, g_E_node_x=None, g_samples=None, eps=None,
            samples=None, g_E_init=None, g_E_pair=None, dense_out=None, param_out=False, lengths=None):
        """Vector-Jacobian product w.r.t. the node potentials of the last
        `launch(..., keep_factor=True, keep_cross=True)` [+ `sample`]: returns (g_node_J, g_node_h)
        (B,T,n) each; g_node_logZ[b,t] = g_lognorm[b].  Replaces the reference's natural_filter_grad /
        natural_smoother_general_grad / natural_sample_backward_grad
        (cython_lds_inference.pyx:92-145, 236-306, 357-409).  g_E_init (B, n*n+n) and, with per-step
        pair parameters, g_E_pair (B,T-1,3,n,n) are the cotangents of the remaining statistics
        (_compute_stats_grad, :212-234) -- what the SLDS-SVAE differentiates.  dense_out (B,T,n,n): also receives
        -2 Pbar_t, the (unsymmetrised) cotangent of a DENSE node potential J_t (svae_lds_estep_vjp_dense_f64).
        param_out=True (n <= 15, full records): returns (g_node_J, g_node_h, (g_init_J, g_init_h, g_init_logZ, g_J11,
        g_J12, g_J22, g_logZ_pair)) -- the cotangents of the natural parameters in the layout of the launch, summed over
        what each is shared over; g_init_J / g_J11 / g_J22 symmetrised, g_J12 full (svae_lds_estep_vjp_params_f64).  The
        node gradients are the same bits as without it.
        lengths: after a launch with per-sequence lengths the sweeps are the ragged ones (svae_lds_ragged_vjp_f64) with the
        lengths of that launch -- passing them again is optional (they must be the same); the cotangents at
        t >= lengths[b] are never used, the gradients there are 0.  No statistics cotangents, dense_out or param_out.
        After infer_ragged_perstep(..., keep_vjp=True) the sweeps are those of svae_lds_ragged_perstep_vjp_f64: g_E_init and
        the per-step g_E_pair are accepted (g_E_pair[b, lengths[b]-1:] is never used), dense_out / param_out are not."""
        self._no_xl("vjp()")
        ragged = self._lengths is not None
        if lengths is not None and not ragged:
            raise ValueError("vjp(lengths=): the last launch of this plan had no per-sequence lengths")
        if ragged:
            if lengths is not None and _shape_of(lengths) != (self.B,):
                raise ValueError("vjp(lengths=): lengths must have shape (B,) = (%d,), got %s" % (self.B, _shape_of(lengths)))
            if param_out or dense_out is not None:
                raise ValueError("vjp() after a launch with lengths: no parameter gradients (param_out / natparam_grad) and "
                                 "no dense node-potential cotangents")
            if (g_E_init is not None or g_E_pair is not None) and not self._perstep:
                raise ValueError("vjp() after a launch with lengths: no cotangents of E_init / E_pair (pair_stats_grad)")
        lean = self.lean
        if param_out:
            if self.n > _lib.LDS_MAX_N:
                raise ValueError("parameter gradients: latent dimension <= %d (n = %d)" % (_lib.LDS_MAX_N, self.n))
            if lean:
                raise ValueError("parameter gradients need the full per-step records: the last forward pass of this plan "
                                 "kept lean ones (make the plan with options | OPT_LEAN_OFF)")
            if dense_out is not None:
                raise ValueError("param_out and dense_out are separate calls")
        if not (self.has_cross and (lean or self.has_factor)):
            raise RuntimeError("vjp() needs a preceding launch(..., keep_factor=True, keep_cross=True) or infer()")
        if lean and (g_E_init is not None or g_E_pair is not None):
            raise ValueError("lean records (infer() on a large homogeneous batch): no cotangents of E_init / E_pair")
        if g_E_pair is not None and not self.inhomog:
            raise ValueError("a homogeneous plan keeps only the SUMMED pair statistics; their cotangents go through "
                             "the per-step layout: lds_inference_differentiable(..., pair_stats_grad=True)")
        f64 = dict(dtype=torch.float64, device=self.device)
        c = lambda x: None if x is None else x.to(**f64).contiguous()
        g_lognorm, g_E_node_diagxx, g_E_node_x = c(g_lognorm), c(g_E_node_diagxx), c(g_E_node_x)
        g_samples, eps, samples = c(g_samples), c(eps), c(samples)
        g_E_init, g_E_pair = c(g_E_init), c(g_E_pair)
        S = 0 if g_samples is None else g_samples.shape[2]
        options = self.options
        if self._infer_S is not None:
            # the workspace was written by infer(): the VJP is told so and takes the S of that call (it fixes the format)
            if g_samples is not None and S != self._infer_S:
                raise ValueError("vjp(): %d sample cotangents for an infer() call that drew %d" % (S, self._infer_S))
            options |= _lib.OPT_INFER_RECORDS
            S = self._infer_S
        if S > 16:
            # the kernels take 16 sample cotangents per launch; the VJP is linear in the cotangents: the first chunk
            # travels with all the others, the remaining chunks alone
            first = self.vjp(g_lognorm, g_E_node_diagxx, g_E_node_x, g_samples[:, :, :16], eps[:, :, :16],
                             samples[:, :, :16], g_E_init, g_E_pair, param_out=param_out)
            gJ, gh = first[0], first[1]
            zero = torch.zeros_like(g_lognorm)
            for s0 in range(16, S, 16):
                more = self.vjp(zero, None, None, g_samples[:, :, s0:s0 + 16], eps[:, :, s0:s0 + 16],
                                samples[:, :, s0:s0 + 16], param_out=param_out)
                gJ += more[0]
                gh += more[1]
                if param_out:
                    for x, y in zip(first[2], more[2]):
                        x += y
            return (gJ, gh, first[2]) if param_out else (gJ, gh)
        B, T, n = self.B, self.T, self.n
        if self.vjp_ws is None:
            self.vjp_ws_bytes = int(self.lib.svae_lds_vjp_workspace_bytes(max(B, 1), T, n))
            self.vjp_ws = torch.empty(self.vjp_ws_bytes // 8, **f64)
        gJ = torch.empty(B, T, n, **f64)
        gh = torch.empty(B, T, n, **f64)
        p = _lib.ptr
        workspaces = [p(self.ws), self.ws_bytes, p(self.vjp_ws), self.vjp_ws_bytes, _lib.current_stream(self.device)]
        if ragged and self._perstep:
            self._call("svae_lds_ragged_perstep_vjp_f64", [B, T, n, S, int(self._pair_batched), self.options] + _lib.ptrs(
                (self._J12, g_lognorm, g_E_node_diagxx, g_E_node_x, g_E_init, g_E_pair, g_samples, eps, samples,
                 self.E_pair, self.E_node_x, self._lengths, gJ, gh)) + workspaces)
            return gJ, gh
        if ragged:
            self._call("svae_lds_ragged_vjp_f64", [B, T, n, S, 0, 0, self.options] + _lib.ptrs(
                (g_lognorm, g_E_node_diagxx, g_E_node_x, g_samples, eps, samples, self._lengths, gJ, gh)) + workspaces)
            return gJ, gh
        # what the three entry points begin with: shape, layout and options, then the thirteen pointers up to (gJ, gh)
        pb = self._pair_batched
        head = [B, T, n, S, int(self.inhomog), int(pb), options] + _lib.ptrs(
            (self._J12, g_lognorm, g_E_node_diagxx, g_E_node_x, g_E_init, g_E_pair, g_samples, eps, samples,
             self.E_pair, self.E_node_x, gJ, gh))
        if param_out:
            if self.param_ws is None:
                self.param_ws_bytes = int(self.lib.svae_lds_param_vjp_workspace_bytes(max(B, 1), T, n, int(self.inhomog), int(pb)))
                self.param_ws = torch.empty(self.param_ws_bytes // 8, **f64)
            lead = ((B, max(T - 1, 0)) if pb else (max(T - 1, 0),)) if self.inhomog else ()
            out = (torch.empty(n, n, **f64), torch.empty(n, **f64), torch.empty(1, **f64),
                   torch.empty(*lead, n, n, **f64), torch.empty(*lead, n, n, **f64), torch.empty(*lead, n, n, **f64),
                   torch.empty(*lead, **f64) if self.inhomog else torch.empty(1, **f64))
            workspaces[4:4] = [p(self.param_ws), self.param_ws_bytes]            # (in front of the stream)
            self._call("svae_lds_estep_vjp_params_f64", head + _lib.ptrs(out) + workspaces)
            if B == 0:
                for x in out:
                    x.zero_()
            return gJ, gh, out
        if dense_out is not None:
            if S > 16 or lean:
                raise ValueError("dense node-potential cotangents: at most 16 sample cotangents, full records")
            self._call("svae_lds_estep_vjp_dense_f64", head + [p(dense_out)] + workspaces)
        else:
            self._call("svae_lds_estep_vjp_ex_f64", head + workspaces)
        return gJ, gh

    def reduce(self):
        """Deterministic batch sums [sum E_init | sum E_pair | sum lognorm | B] (homogeneous); after a launch with
        per-sequence lengths one more slot, sum_b (lengths[b] - 1): the pair count, which is not B (T-1) then."""
        if self.inhomog:
            raise ValueError("reduce(): per-step pair statistics (B,T-1,3,n,n) have no batch-summed form here")
        stats = (self.E_init, self.E_pair, self.lognorm)
        stream = [_lib.current_stream(self.device)]
        if self._lengths is not None:
            # [sum E_init | sum E_pair | sum lognorm | B | sum_b (lengths[b] - 1)]: one more slot, the pair count
            if self.reduced_ragged is None:
                self.reduced_ragged = torch.empty(4 * self.n * self.n + self.n + 3, dtype=torch.float64, device=self.device)
            self._call("svae_lds_ragged_reduce_stats_f64",
                       [self.B, self.T, self.n] + _lib.ptrs(stats + (self._lengths, self.reduced_ragged)) + stream)
            return self.reduced_ragged
        self._call("svae_lds_xl_reduce_stats_f64" if self.xl else "svae_lds_reduce_stats_f64",
                   [self.B, self.n] + _lib.ptrs(stats + (self.reduced,)) + stream)
        return self.reduced

    def check_info(self):
        """Synchronising check of the device-side status word (the reference never checks LAPACK
        `info`, cython_gaussian_grads.pxd:54-76; we do, on request)."""
        v = int(self.info.item())
        if v != 0:
            self.info.zero_()
            raise FloatingPointError("LDS E-step: sequence %d hit a non-positive pivot "
                                     "(potentials not positive definite; through models.lds.run_inference also: the "
                                     "global natural parameters are not valid -- a scale matrix that is not positive "
                                     "definite, kappa <= 0 or nu <= n - 1; with lengths= also: a length outside 1..T)"
                                     % (v - 1))


def require_sampler_range(n, what):
    """The sampler and the VJPs stop at n = 64 (the XL E-step, 65 <= n <= 128, keeps no record for them): ValueError before
    anything is launched."""
    if int(n) > _lib.LDS_TILE_MAX_N:
        raise ValueError("%s: the sampler and the VJPs take latent dimension <= %d (n = %d: E-step only, "
                         "natural_lds_estep_general)" % (what, _lib.LDS_TILE_MAX_N, int(n)))


def _is_dense_nodes(node_params):
    if not isinstance(node_params, (tuple, list)) or len(node_params) < 2:
        return False
    nd = lambda x: x.dim() if isinstance(x, torch.Tensor) else np.ndim(x)
    return nd(node_params[0]) == nd(node_params[1]) + 1


def _fold_dense_nodes(natparam, node_params):
    """Dense node potentials J (T,n,n) / (B,T,n,n) of the reference's Python path (`natural_condition_on_general`,
    svae/lds/gaussian.py:46-49; `_canonical_node_params`, lds_inference.py:65-82 -- the compiled path takes diagonal ones
    only, cython_lds_inference.pyx:43).  Every step of the filter, the smoother and the sampler sees the node potential of
    step t only in the sum J_pred[t] + Jo[t] (+ J11[t]) -- `natural_predict`, `natural_rts_backward_step`,
    `natural_condition_on(J_filt, ., ., J11, J12)` -- so the off-diagonal part of Jo[t] is exactly a contribution to the
    pair block of x_t: J11[t] += offdiag(Jo[t]) for t < T-1 and J22[T-2] += offdiag(Jo[T-1]) (init_J for T = 1), with
    per-step, per-sequence pair parameters.  The kernels then run with the diagonal of Jo; only the forward MESSAGES differ
    by these terms (put back in `natural_filter_forward_general`).
    -> (natparam', node_params' batched (B,T,n), info)"""
    init_params, pair_params = natparam
    dev = _find_device(list(node_params) + list(init_params[:2]))
    node_J, node_h = _as_dev(node_params[0], dev), _as_dev(node_params[1], dev)
    node_logZ = _as_dev(node_params[2], dev) if len(node_params) == 3 else None
    batched = node_h.dim() == 3
    if node_h.dim() not in (2, 3) or node_J.shape[:-1] != node_h.shape or node_J.shape[-1] != node_h.shape[-1]:
        raise ValueError("dense node potentials must be J (T,n,n), h (T,n) or J (B,T,n,n), h (B,T,n)")
    if not batched:
        node_J, node_h = node_J[None], node_h[None]
        node_logZ = None if node_logZ is None else node_logZ[None]
    B, T, n = node_h.shape
    diag = torch.diagonal(node_J, dim1=-2, dim2=-1).contiguous()
    off = node_J - torch.diag_embed(diag)
    off = 0.5 * (off + off.transpose(-1, -2))          # (the factorisations read one triangle: symmetric part)
    J11, J12, J22 = (_as_dev(x, dev) for x in pair_params[:3])
    lz = _as_dev(pair_params[3], dev).reshape(-1)
    homog = J11.dim() == 2
    if T == 1:
        if B != 1:
            raise ValueError("dense node potentials with T = 1: one sequence per call (the initial potential is shared)")
        init_params = (_as_dev(init_params[0], dev) + off[0, 0],) + tuple(init_params[1:])
        pair = (J11, J12, J22, lz)
    else:
        def per_seq(x):
            x = x if x.dim() == 4 else (x[None] if x.dim() == 3 else x[None, None])
            return x.expand(B, T - 1, n, n).clone()
        J11, J12, J22 = per_seq(J11), per_seq(J12), per_seq(J22)
        lz = (lz.reshape(1, -1) if lz.numel() in (1, T - 1) else lz.reshape(B, T - 1)).expand(B, T - 1).contiguous().reshape(-1)
        J11 += off[:, :T - 1]
        J22[:, T - 2] += off[:, T - 1]
        pair = (J11, J12, J22, lz)
    nodes = (diag, node_h.contiguous()) + ((node_logZ,) if node_logZ is not None else ())
    return (init_params, pair), nodes, dict(off=off, homog=homog, batched=batched, B=B, T=T, n=n)


def _dense_stats(stats, info):
    """Statistics of a folded launch in the reference's dense form: E_node = (E[x x'] (T,n,n), E[x], 1) --
    `make_node_stats`, lds_inference.py:163-166 -- and, for homogeneous pair parameters, the pair statistics summed over
    time (:172-173)."""
    Ei, Ep, En = stats
    B, T, n = info["B"], info["T"], info["n"]
    if T > 1:
        ExxT = torch.cat([Ep[0], Ep[2][:, -1:]], dim=1)
        if info["homog"]:
            Ep = (Ep[0].sum(1), Ep[1].sum(1), Ep[2].sum(1), Ep[3].sum(1))
    else:
        ExxT = Ei[0][:, None].clone()
    En = (ExxT, En[1], En[2])
    if not info["batched"]:
        sq = lambda tup: tuple(x[0] for x in tup)
        Ei, Ep, En = sq(Ei), sq(Ep), sq(En)
    return Ei, Ep, En


# Homogeneous pair parameters that arrive as HOST data (NumPy arrays / CPU tensors: what a caller coming from the reference
# passes) are looked at before they go to the device: beyond this condition number of J11 / J22 a plan made on the spot takes
# the cond * eps kernels (set_accurate_smoother's option bits) for that call.  Two n x n SVDs on the host, no device
# synchronisation; device-resident parameters -- the fast path -- are never inspected.  None switches the guard off.
CONDITION_GUARD_THRESHOLD = 1e6


def _host_condition_options(pair_params):
    """option bits for a plan created on the spot: the accurate kernels when the pair blocks are host data and ill-conditioned"""
    if CONDITION_GUARD_THRESHOLD is None:
        return 0
    blocks = []
    for x in (pair_params[0], pair_params[2]):
        if isinstance(x, torch.Tensor):
            if x.is_cuda:
                return 0
            x = x.detach().numpy()
        x = np.asarray(x, dtype=float)
        if x.ndim != 2 or x.shape[0] != x.shape[1] or x.shape[0] > 15 or not np.all(np.isfinite(x)):
            return 0
        blocks.append(x)
    try:
        worst = max(float(np.linalg.cond(b)) for b in blocks)
    except np.linalg.LinAlgError:
        return 0
    return (_lib.OPT_TWOEND_FULL | _lib.OPT_LEAN_ON) if worst > CONDITION_GUARD_THRESHOLD else 0


def _guarded_plan_options(pair_params, inhomog=False):
    """`options` of a plan an entry point creates on the spot: None (the default word), or the default word with the
    accurate kernels' bits when the homogeneous pair blocks are host data and ill-conditioned (_host_condition_options)"""
    guard = 0 if inhomog else _host_condition_options(pair_params)
    return ((_default_options & ~_lib.OPT_LEAN_OFF) | guard) if guard else None


def _prepare(natparam, node_params, plan):
    """Shape checks / canonical device tensors shared by the E-step, filter and sampler wrappers
    (`_canonical_node_params`, `_canonical_init_params`, lds_inference.py:59-82)."""
    init_params, pair_params = natparam
    if not isinstance(node_params, (tuple, list)) or len(node_params) not in (2, 3):
        raise ValueError("node_params must be (J, h) or (J, h, logZ)")
    dev = _find_device(list(node_params) + list(init_params[:2]))
    node_J, node_h = _as_dev(node_params[0], dev), _as_dev(node_params[1], dev)
    node_logZ = _as_dev(node_params[2], dev) if len(node_params) == 3 else None
    if node_J.dim() == 3 and node_h.dim() == 2:
        raise ValueError("dense (T,n,n) node potentials: through natural_lds_estep_general / natural_lds_sample / "
                         "natural_lds_inference_general / natural_filter_forward_general (folded into per-step pair "
                         "parameters there); the kernels and the differentiable path take diagonal ones, like the "
                         "reference's compiled path (cython_lds_inference.pyx:43)")
    batched = node_h.dim() == 3
    if node_J.shape != node_h.shape or node_h.dim() not in (2, 3):
        raise ValueError("node potentials must both be (T,n) or (B,T,n)")
    if not batched:
        node_J, node_h = node_J[None], node_h[None]
        node_logZ = None if node_logZ is None else node_logZ[None]
    B, T, n = node_h.shape
    if node_logZ is not None and tuple(node_logZ.shape) != (B, T):
        raise ValueError("node logZ must be (T,) / (B,T)")

    init_J, init_h, init_logZ = _canonical_init_params(init_params, dev)
    if tuple(init_J.shape) != (n, n) or tuple(init_h.shape) != (n,):
        raise ValueError("init_params shapes do not match the node potentials")
    J11, J12, J22, logZ_pair, inhomog, pair_batched = _canonical_pair_params(pair_params, B, T, n, dev)
    if plan is None:
        plan = LDSEStepPlan(B, T, n, dev, inhomog, pair_batched, options=_guarded_plan_options(pair_params, inhomog))
    elif (plan.B, plan.T, plan.n, plan.inhomog) != (B, T, n, inhomog):
        raise ValueError("plan shape mismatch")
    return dict(plan=plan, batched=batched, B=B, T=T, n=n, inhomog=inhomog, pair_batched=pair_batched,
                args=(init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ))


def natural_lds_estep_general(natparam, node_params, plan=None, check=False, keep_factor=False, lengths=None):
    """E-step = filter + smoother (lds_inference.py:223-237).

    natparam = (init_params, pair_params); init_params = (-1/2 J0, h0, logZ...) and
    pair_params = (J11, J12, J22, logZ) homogeneous (n,n) or per-step (T-1,n,n)
    [or (B,T-1,n,n) with batched nodes]; node_params = (J, h[, logZ]) with diagonal J of shape
    (T,n) or (B,T,n).

    Returns (lognorm, (E_init_stats, E_pair_stats, E_node_stats)) shaped like the reference's
    (cython_lds_inference.pyx:197-210); with a batch axis first when the nodes are batched.

    Accuracy: lognorm is at cond * eps; the smoothed moments of the default kernels for n <= 15 at cond^2 * eps (1e-12 on
    well-conditioned models, within 1e-5 of the reference up to cond(J22) ~ 1e7); set_accurate_smoother() (or a plan with
    SVAE_OPT_TWOEND_FULL) selects the cond * eps kernels.

    Asynchronous like the reference is silent: no host synchronisation unless `check=True`, which reads
    the device-side status word and raises FloatingPointError for potentials that are not positive
    definite (the reference ignores LAPACK `info`, cython_gaussian_grads.pxd:54-76); `plan.check_info()`
    does the same later.  The returned tensors are views of the plan's buffers: valid until its next launch.

    lengths (B,) int array / tensor: sequences of different lengths in one batch (n <= 15, (n,n) pair parameters, diagonal
    node potentials (B,T,n)): sequence b occupies steps 0 .. lengths[b]-1.  lognorm, E_init, E_pair and E_node[:, :L] of
    every sequence are those of the sequence truncated to its length L (E_pair: sums over its own L-1 pairs, fourth entry
    L-1); the node statistics at t >= L are 0 (the constant 1 included) and node_params[b, L:] are never used (they may
    be NaN).  A length outside 1..T raises the status word (`check=True` / `plan.check_info()`).
    """
    if lengths is not None:
        _ragged_precheck(natparam, node_params, lengths, "natural_lds_estep_general")
    if _is_dense_nodes(node_params):
        if plan is not None:
            raise ValueError("dense node potentials: the plan is built internally (per-step, per-sequence pair layout)")
        natparam, node_params, info = _fold_dense_nodes(natparam, node_params)
        lognorm, stats = natural_lds_estep_general(natparam, node_params, check=check, keep_factor=keep_factor)
        return (lognorm if info["batched"] else lognorm[0]), _dense_stats(stats, info)
    return _estep(natparam, node_params, plan, check, keep_factor, lengths=lengths)[:2]


def _estep(natparam, node_params, plan=None, check=False, keep_factor=False, eps=None, lengths=None):
    """natural_lds_estep_general on diagonal node potentials -> (lognorm, expected_stats, samples).  eps (B,T,S,n): E-step +
    sampler in ONE call (plan.infer, forward values only: lean records for large homogeneous batches); None: no samples."""
    q = _prepare(natparam, node_params, plan)
    plan, batched, B, n, inhomog = q["plan"], q["batched"], q["B"], q["n"], q["inhomog"]
    samples = None
    if eps is not None:
        samples = plan.infer(*q["args"], q["pair_batched"], eps, keep_vjp=False, lengths=lengths)
    else:
        plan.launch(*q["args"], q["pair_batched"], keep_factor, lengths=lengths)
    if check:
        plan.check_info()

    ExxT0 = plan.E_init[:, :n * n].reshape(B, n, n)
    Ex0 = plan.E_init[:, n * n:]
    if inhomog:
        Ep = (plan.E_pair[:, :, 0], plan.E_pair[:, :, 1], plan.E_pair[:, :, 2], plan.ones_pair)
    else:
        Ep = (plan.E_pair[:, 0], plan.E_pair[:, 1], plan.E_pair[:, 2], plan.ones_pair)
    En = (plan.E_node_diagxx, plan.E_node_x, plan.ones_BT)
    if lengths is not None:
        Ep = Ep[:3] + (plan.pair_counts,)
        En = (plan.E_node_diagxx, plan.E_node_x, plan.live().to(torch.float64))
    Ei = (ExxT0, Ex0, plan.ones_B, plan.ones_B)
    lognorm = plan.lognorm
    if not batched:
        sq = lambda tup: tuple(x[0] for x in tup)
        return lognorm[0], (sq(Ei), sq(Ep), sq(En)), samples
    return lognorm, (Ei, Ep, En), samples


cython_natural_lds_estep_general = natural_lds_estep_general


def natural_filter_forward_general(init_params, pair_params, node_params, plan=None, check=False):
    """The forward filter alone, with its messages: ((J_pred, h_pred), (J_filt, h_filt)), lognorm in the
    reference's scaling (natural parameters: J = -1/2 precision), shapes (T,n,n) / (T,n) [(B,...) when
    the nodes are batched] -- `natural_filter_forward_general` (cython_lds_inference.pyx:28-90, result
    :84-87; Python twin lds_inference.py:86-106).  The plan's workspace afterwards serves `plan.sample`."""
    if _is_dense_nodes(node_params):
        if plan is not None:
            raise ValueError("dense node potentials: the plan is built internally")
        (ip, pp), nodes, info = _fold_dense_nodes((init_params, pair_params), node_params)
        ((Jp, hp), (Jf, hf)), lognorm = natural_filter_forward_general(ip, pp, nodes, check=check)
        off, T = info["off"], info["T"]
        Jf[:, :T - 1] += off[:, :T - 1]        # J_filt[t] = J_pred[t] + Jo[t]: the part that was folded into J11[t]
        Jp[:, T - 1] -= off[:, T - 1]          # ... and the part the last prediction (or the initial potential) carried
        if not info["batched"]:
            return ((Jp[0], hp[0]), (Jf[0], hf[0])), lognorm[0]
        return ((Jp, hp), (Jf, hf)), lognorm
    q = _prepare((init_params, pair_params), node_params, plan)
    plan, B, T, n = q["plan"], q["B"], q["T"], q["n"]
    if n > _lib.LDS_MAX_N:
        raise ValueError("filter messages: latent dimension <= %d" % _lib.LDS_MAX_N)
    f64 = dict(dtype=torch.float64, device=plan.device)
    Jp, Jf = torch.empty(B, T, n, n, **f64), torch.empty(B, T, n, n, **f64)
    hp, hf = torch.empty(B, T, n, **f64), torch.empty(B, T, n, **f64)
    plan.filter(*q["args"], q["pair_batched"], Jp, hp, Jf, hf)
    if check:
        plan.check_info()
    lognorm = plan.lognorm
    if not q["batched"]:
        return ((Jp[0], hp[0]), (Jf[0], hf[0])), lognorm[0]
    return ((Jp, hp), (Jf, hf)), lognorm


def _model_from_messages(forward_messages, pair_params):
    """The LDS whose forward filter reproduces the given messages: init = the first predicted message, node potential of
    step t = filtered - predicted message of step t.  For messages that came out of a forward filter with these pair
    parameters -- every call site of the reference (lds_inference.py:196-202, 232-237, 260-264) -- the smoother / sampler
    of this model IS the reference's smoother / sampler on the messages."""
    (Jp, hp), (Jf, hf) = forward_messages
    dev = _find_device([hf])
    Jp, hp, Jf, hf = (_as_dev(x, dev) for x in (Jp, hp, Jf, hf))
    batched = hf.dim() == 3
    if not batched:
        Jp, hp, Jf, hf = Jp[None], hp[None], Jf[None], hf[None]
    if Jp.dim() != 4 or Jp.shape != Jf.shape or hp.shape != hf.shape or Jp.shape[:3] != hp.shape:
        raise ValueError("forward_messages = ((J_pred, h_pred), (J_filt, h_filt)) with J (T,n,n) and h (T,n) [or a leading B axis]")
    dJ, dh = Jf - Jp, hf - hp
    if Jp.shape[0] > 1:             # one initial potential for the batch: differences of the first predictions join the node
        dJ[1:, 0] += Jp[1:, 0] - Jp[0, 0]
        dh[1:, 0] += hp[1:, 0] - hp[0, 0]
    dg = torch.diagonal(dJ, dim1=-2, dim2=-1)
    off = float((dJ - torch.diag_embed(dg)).abs().max())
    dense = off > 1e-12 * max(float(dJ.abs().max()), 1e-300)
    natparam = ((Jp[0, 0].contiguous(), hp[0, 0].contiguous(), torch.zeros((), dtype=torch.float64, device=dev)),
                pair_params)
    nodes = (dJ if dense else dg.contiguous(), dh)
    if not batched:
        nodes = tuple(x[0] for x in nodes)
    return natparam, nodes


def natural_smoother_general(forward_messages, pair_params):
    """RTS smoother + expected statistics on CALLER-SUPPLIED forward messages: (E_init, E_pair, E_node) as the
    reference's tuples -- `natural_smoother_general(forward_messages, pair_params)`, the second of the functions the
    reference imports from its compiled module (lds_inference.py:18-24; cython_lds_inference.pyx:149-210).
    forward_messages = ((J_pred, h_pred), (J_filt, h_filt)) in the reference's scaling (natural parameters), as
    `natural_filter_forward_general` returns them [(B,T,...) batched].  See _model_from_messages for what is assumed of
    the messages."""
    natparam, nodes = _model_from_messages(forward_messages, pair_params)
    return natural_lds_estep_general(natparam, nodes)[1]


def natural_sample_backward(forward_messages, pair_params, num_samples, eps=None, generator=None):
    """Backward sampling on caller-supplied forward messages -> samples (T,S,n) [(B,T,S,n)]:
    `natural_sample_backward(forward_messages, pair_params, num_samples)` (lds_inference.py:18-24;
    cython_lds_inference.pyx:310-355).  `eps` (T,S,n) as in natural_lds_inference_general (the reference draws
    flipud(randn(T,S,n)) inside, :333)."""
    natparam, nodes = _model_from_messages(forward_messages, pair_params)
    return natural_lds_sample(natparam, nodes, num_samples, eps=eps, generator=generator)


def natural_lds_sample(natparam, node_params, num_samples=1, eps=None, plan=None, generator=None, lengths=None):
    """Filter + backward sampling WITHOUT the smoother: `cython_natural_lds_sample`
    (lds_inference.py:260-264) -> samples (T,S,n) [(B,T,S,n) batched].  `eps` as in
    natural_lds_inference_general.  lengths (B,): as in natural_lds_inference_general (the ragged kernels have no
    filter-only form: this is that call with the statistics dropped)."""
    require_sampler_range(_shape_of(node_params[1])[-1], "natural_lds_sample")
    if lengths is not None:
        _ragged_precheck(natparam, node_params, lengths, "natural_lds_sample")
        return natural_lds_inference_general(natparam, node_params, num_samples=num_samples, eps=eps, plan=plan,
                                             generator=generator, lengths=lengths)[0]
    if _is_dense_nodes(node_params):
        if plan is not None:
            raise ValueError("dense node potentials: the plan is built internally")
        natparam, node_params, info = _fold_dense_nodes(natparam, node_params)
        if eps is not None and not info["batched"]:
            eps = torch.as_tensor(eps, dtype=torch.float64)[None]
        samples = natural_lds_sample(natparam, node_params, num_samples, eps, None, generator)
        return samples if info["batched"] else samples[0]
    nh = node_params[1]
    if int(nh.shape[-1]) > _lib.LDS_MAX_N:
        # 16 <= n <= 64: the tile kernels have no filter-only form; the sampler works on the hand-off of the tile
        # E-step (same eps -> sample map), so this is the E-step + sampler with the statistics dropped
        return natural_lds_inference_general(natparam, node_params, num_samples=num_samples, eps=eps, plan=plan,
                                             generator=generator)[0]
    q = _prepare(natparam, node_params, plan)
    plan = q["plan"]
    plan.filter(*q["args"], q["pair_batched"])
    S = int(num_samples)
    if eps is None:
        eps = torch.randn(plan.B, plan.T, S, plan.n, dtype=torch.float64, device=plan.device, generator=generator)
    else:
        eps = torch.as_tensor(eps, dtype=torch.float64)
        eps = eps if q["batched"] else eps[None]
    samples = plan.sample(eps)
    return samples if q["batched"] else samples[0]


cython_natural_lds_sample = natural_lds_sample


def natural_lds_inference_general(natparam, node_params, num_samples=None, eps=None, plan=None,
                                  generator=None, lengths=None):
    """E-step + backward sampling: (samples, expected_stats, lognorm), mirroring
    `cython_natural_lds_inference_general` (lds_inference.py:196-202).  samples: (T,S,n), or (T,n) when
    num_samples is None as in the Python path (:109-124); batched nodes add a leading B axis.
    The reference draws its noise from the global NumPy RNG inside the sampler
    (cython_lds_inference.pyx:333); here `eps` (B,T,S,n) / (T,S,n) may be passed in, else it is drawn
    from `generator` on the device.
    lengths (B,): per-sequence lengths as in natural_lds_estep_general; samples[b, :L] are the truncated sequence's for
    eps[b, :L], samples[b, L:] are 0 and eps[b, L:] is never used."""
    require_sampler_range(_shape_of(node_params[1])[-1], "natural_lds_inference_general")
    if lengths is not None:
        _ragged_precheck(natparam, node_params, lengths, "natural_lds_inference_general")
    if _is_dense_nodes(node_params):
        if plan is not None:
            raise ValueError("dense node potentials: the plan is built internally")
        natparam, node_params, info = _fold_dense_nodes(natparam, node_params)
        if eps is not None and not info["batched"]:
            eps = torch.as_tensor(eps, dtype=torch.float64)[None]
        samples, stats, lognorm = natural_lds_inference_general(natparam, node_params, num_samples, eps, None, generator)
        if not info["batched"]:
            samples, lognorm = samples[0], lognorm[0]
        return samples, _dense_stats(stats, info), lognorm
    batched = (node_params[1].ndim if hasattr(node_params[1], "ndim") else torch.as_tensor(node_params[1]).dim()) == 3
    S = 1 if num_samples is None else int(num_samples)
    if plan is None:
        nh = torch.as_tensor(node_params[1])
        B, T, n = (nh.shape if batched else (1,) + tuple(nh.shape))
        pdim = torch.as_tensor(natparam[1][0]).dim()
        plan = LDSEStepPlan(B, T, n, "cuda", pdim >= 3, pdim == 4, options=_guarded_plan_options(natparam[1], pdim != 2))
    if eps is None:
        eps = torch.randn(plan.B, plan.T, S, plan.n, dtype=torch.float64, device=plan.device,
                          generator=generator)
    else:
        eps = torch.as_tensor(eps, dtype=torch.float64)
        eps = eps if batched else eps[None]
    if plan.n <= _lib.LDS_MAX_N and eps.dim() == 4 and (eps.shape[2] <= 16 or lengths is not None):
        # ONE call (svae_lds_inference_f64 = the reference's composite, lds_inference.py:196-202)
        lognorm, stats, samples = _estep(natparam, node_params, plan, keep_factor=True, eps=eps, lengths=lengths)
    else:
        lognorm, stats = natural_lds_estep_general(natparam, node_params, plan=plan, keep_factor=True)
        samples = plan.sample(eps)
    if num_samples is None:
        samples = samples[:, :, 0]
    if not batched:
        samples = samples[0]
    return samples, stats, lognorm


cython_natural_lds_inference_general = natural_lds_inference_general


def reduce_stats(plan):
    """Sum over the batch of the global statistics, unpacked like the reference tuples:
    ((sum ExxT0, sum Ex0, B, B), (sum E_pair[0..2], B*(T-1)), sum lognorm).  This is the buffer
    all-reduced across GPUs before the natural-gradient step (svae.py:33-34)."""
    n, B, T = plan.n, plan.B, plan.T
    r = plan.reduce()
    nn = n * n
    Ei = (r[:nn].reshape(n, n), r[nn:nn + n], float(B), float(B))
    o = nn + n
    Ep = (r[o:o + nn].reshape(n, n), r[o + nn:o + 2 * nn].reshape(n, n),
          r[o + 2 * nn:o + 3 * nn].reshape(n, n), float(B * (T - 1)))
    return Ei, Ep, r[o + 3 * nn]


def require_same_launch(ctx, message="LDSEStepPlan was launched again before backward(): the hand-off workspace of this "
                        "forward pass is gone (use one plan per live autograd graph, or call backward before the next forward)"):
    """The plan of an autograd node, if its last launch is still the node's forward pass (ctx.epoch); else RuntimeError."""
    if ctx.plan.epoch != ctx.epoch:
        raise RuntimeError(message)
    return ctx.plan


def _backward_prologue(ctx, g_lognorm, g_samples, **relaunched):
    """What the backward passes below begin with -> (plan, g_lognorm (zeros for None), (g_samples, eps, samples) for
    plan.vjp: all None unless samples were drawn and their cotangent arrived)"""
    plan = require_same_launch(ctx, **relaunched)
    if g_lognorm is None:
        g_lognorm = torch.zeros_like(plan.lognorm)
    if not ctx.has_samples or g_samples is None:
        return plan, g_lognorm, (None, None, None)
    return plan, g_lognorm, (g_samples,) + tuple(ctx.saved_tensors)


class _LDSInference(torch.autograd.Function):
    """Differentiable (w.r.t. the node potentials) E-step + sampler, the torch counterpart of the
    reference's three autograd primitives (lds_inference.py:26-39).  Forward: one E-step launch
    (+ sampler); backward: the two VJP sweeps.  With homogeneous pair parameters the global
    statistics (E_init, E_pair sums) are returned non-differentiable, as in the reference's use
    (svae.py:21 `saved.stats`); with per-step pair parameters (the SLDS, slds_svae.py:295-300)
    E_init and the per-step E_pair carry gradients too."""

    @staticmethod
    def forward(ctx, node_J, node_h, node_logZ, eps, plan, params, pair_batched, lengths=None):
        init_J, init_h, init_logZ, J11, J12, J22, logZ_pair = params
        ctx.ragged = lengths is not None
        # Large batches, eager: the launch writes into FRESH output tensors that are handed to autograd as they are (the
        # copies out of the plan's buffers are 0.3 ms of a 3 ms step at 4096 x 200 x 10).  Small batches and anything
        # under stream capture keep the copies: a captured step must write into buffers that outlive the capture, and
        # replacing the plan's buffers inside a capture of the whole make_gradfun step crashed hipStreamEndCapture
        # (ROCm 7.2; bench.py extra[9]) -- there the copies are a few microseconds.
        _copy_out = plan.B <= 1024 or torch.cuda.is_current_stream_capturing()
        if not _copy_out:
            plan.fresh_outputs()
        if eps is None or eps.shape[2] <= 16 or lengths is not None:
            # one call: E-step + sampler (lean per-step records for large homogeneous batches)
            samples = plan.infer(init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                                 pair_batched, eps, lengths=lengths)
            if samples is None:
                samples = torch.zeros(0, dtype=torch.float64, device=plan.device)
        else:
            plan.launch(init_J, init_h, init_logZ, J11, J12, J22, logZ_pair, node_J, node_h, node_logZ,
                        pair_batched, True, True)
            samples = plan.sample(eps)
        ctx.plan, ctx.has_logZ, ctx.has_samples = plan, node_logZ is not None, eps is not None
        ctx.epoch = plan.epoch
        ctx.set_materialize_grads(False)       # an output nobody differentiated arrives as None, not as zeros
        ctx.save_for_backward(eps if eps is not None else samples, samples)
        E_init, E_pair = plan.E_init, plan.E_pair
        if _copy_out:
            E_init, E_pair = E_init.clone(), E_pair.clone()
        if not plan.inhomog:
            ctx.mark_non_differentiable(E_init, E_pair)
        if _copy_out:
            return (plan.lognorm.clone(), plan.E_node_diagxx.clone(), plan.E_node_x.clone(), samples, E_init, E_pair)
        return (plan.lognorm, plan.E_node_diagxx, plan.E_node_x, samples, E_init, E_pair)

    @staticmethod
    def backward(ctx, g_lognorm, g_dxx, g_x, g_samples, g_init, g_pair):
        plan, g_lognorm, sampled = _backward_prologue(ctx, g_lognorm, g_samples)
        if not plan.inhomog:
            g_init = g_pair = None
        gJ, gh = plan.vjp(g_lognorm, g_dxx, g_x, *sampled, g_init, g_pair)
        gz = g_lognorm[:, None].expand(plan.B, plan.T).clone() if ctx.has_logZ else None
        if ctx.ragged:
            if gz is not None:      # (select: the cotangent of a sequence that does not exist is not propagated)
                gz = torch.where(plan.live(), gz, torch.zeros_like(gz))
            return gJ, gh, gz, None, None, None, None, None
        return gJ, gh, gz, None, None, None, None


class _LDSRaggedPerstepInference(torch.autograd.Function):
    """_LDSInference for a ragged batch with per-step pair parameters (the final pass of the ragged SLDS): forward
    infer_ragged_perstep(keep_vjp=True), backward ONE vjp() call with the cotangents of E_init and of the per-step E_pair.
    Differentiable w.r.t. the node potentials, once; the pair parameters and the init potential are fixed inputs."""

    @staticmethod
    def forward(ctx, node_J, node_h, node_logZ, eps, plan, params, lengths, pair_batched, init_batched):
        samples = plan.infer_ragged_perstep(*params, node_J, node_h, node_logZ, lengths=lengths, pair_batched=pair_batched,
                                            init_batched=init_batched, eps=eps, keep_vjp=True)
        if samples is None:
            samples = torch.zeros(0, dtype=torch.float64, device=plan.device)
        ctx.plan, ctx.has_logZ, ctx.has_samples = plan, node_logZ is not None, eps is not None
        ctx.epoch = plan.epoch
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(eps if eps is not None else samples, samples)
        # (copies: vjp() reads S~_{t+1} back from the plan's own E_pair / E_node_x, which must not move)
        return (plan.lognorm.clone(), plan.E_node_diagxx.clone(), plan.E_node_x.clone(), samples, plan.E_init.clone(),
                plan.E_pair.clone())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lognorm, g_dxx, g_x, g_samples, g_init, g_pair):
        plan, g_lognorm, sampled = _backward_prologue(ctx, g_lognorm, g_samples)
        gJ, gh = plan.vjp(g_lognorm, g_dxx, g_x, *sampled, g_init, g_pair)
        gz = None
        if ctx.has_logZ:            # (select: the cotangent of a step that does not exist is not propagated)
            gz = g_lognorm[:, None].expand(plan.B, plan.T)
            gz = torch.where(plan.live(), gz, torch.zeros_like(gz))
        return gJ, gh, gz, None, None, None, None, None, None


class _LDSInferenceParams(torch.autograd.Function):
    """_LDSInference with the seven natural parameters (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair) as
    differentiable inputs too -- the gradients the reference's Python path has through autograd (lds_inference.py:205-218).
    Forward: the same launches; backward: the same sweeps plus the parameter blocks of the packed second sweep and their
    deterministic reduction (svae_lds_estep_vjp_params_f64).  n <= 15, full records."""

    @staticmethod
    def forward(ctx, node_J, node_h, node_logZ, eps, plan, pair_batched, *params):
        ctx.param_shapes = [tuple(x.shape) for x in params]
        return _LDSInference.forward(ctx, node_J, node_h, node_logZ, eps, plan, tuple(x.detach() for x in params), pair_batched)

    @staticmethod
    def backward(ctx, g_lognorm, g_dxx, g_x, g_samples, g_init, g_pair):
        plan, g_lognorm, sampled = _backward_prologue(ctx, g_lognorm, g_samples)
        if not plan.inhomog:
            g_init = g_pair = None
        gJ, gh, gp = plan.vjp(g_lognorm, g_dxx, g_x, *sampled, g_init, g_pair, param_out=True)
        gz = g_lognorm[:, None].expand(plan.B, plan.T).clone() if ctx.has_logZ else None
        need = ctx.needs_input_grad[6:]
        gp = tuple(g.reshape(shape) if want else None for g, shape, want in zip(gp, ctx.param_shapes, need))
        return (gJ, gh, gz, None, None, None) + gp


class _LDSInferenceDense(torch.autograd.Function):
    """E-step + sampler with DENSE node potentials J (B,T,n,n) -- the reference's Python path, differentiable end to end
    there (lds_inference.py:65-82, 205-218) -- differentiable w.r.t. (J, h[, logZ]).  Forward: the off-diagonal part of
    J_t is folded into per-step, per-sequence pair parameters (_fold_dense_nodes) and the kernels run on its diagonal;
    backward: J_t enters the recursions only through the pivot block P_t, so its cotangent is the whole of P_t's,
    -2 Pbar_t, which the second VJP sweep holds in registers (svae_lds_estep_vjp_dense_f64) -- symmetrised here, because
    the forward pass reads the symmetric part of J_t.  Outputs are the per-step launch's: (lognorm, E[x] (B,T,n),
    samples, E_init, per-step E_pair (B,T-1,3,n,n)); the caller assembles E[x x'] (B,T,n,n) from E_pair with torch ops."""

    @staticmethod
    def forward(ctx, node_J, node_h, node_logZ, eps, natparam):
        nodes_in = (node_J.detach(), node_h.detach()) + ((node_logZ.detach(),) if node_logZ is not None else ())
        (ip, pp), nodes, info = _fold_dense_nodes(natparam, nodes_in)
        B, T, n = info["B"], info["T"], info["n"]
        if T < 2:
            raise ValueError("differentiable dense node potentials: T >= 2")
        dev = nodes[1].device
        plan = LDSEStepPlan(B, T, n, dev, inhomog=True, pair_batched=True)
        init_J, init_h, init_logZ = _canonical_init_params(ip, dev)
        J11, J12, J22 = (x.contiguous() for x in pp[:3])
        samples = plan.infer(init_J, init_h, init_logZ, J11, J12, J22, pp[3].reshape(-1).contiguous(),
                             nodes[0].contiguous(), nodes[1].contiguous(), nodes[2].contiguous() if len(nodes) == 3 else None,
                             True, eps)
        ctx.plan, ctx.epoch, ctx.has_logZ, ctx.has_samples = plan, plan.epoch, node_logZ is not None, eps is not None
        if samples is None:
            samples = torch.zeros(0, dtype=torch.float64, device=dev)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(eps if eps is not None else samples, samples)
        return plan.lognorm.clone(), plan.E_node_x.clone(), samples, plan.E_init.clone(), plan.E_pair.clone()

    @staticmethod
    def backward(ctx, g_lognorm, g_x, g_samples, g_init, g_pair):
        plan, g_lognorm, sampled = _backward_prologue(
            ctx, g_lognorm, g_samples, message="the plan of this forward pass was launched again before backward()")
        dense = torch.empty(plan.B, plan.T, plan.n, plan.n, dtype=torch.float64, device=plan.device)
        _, gh = plan.vjp(g_lognorm, None, g_x, *sampled, g_init, g_pair, dense_out=dense)
        gJ = 0.5 * (dense + dense.transpose(-1, -2))
        gz = g_lognorm[:, None].expand(plan.B, plan.T).clone() if ctx.has_logZ else None
        return gJ, gh, gz, None, None


def _dense_inference_differentiable(natparam, node_params, eps):
    node_J, node_h = node_params[0], node_params[1]
    node_logZ = node_params[2] if len(node_params) == 3 else None
    if node_h.dim() != 3 or node_J.dim() != 4:
        raise ValueError("dense node potentials: J (B,T,n,n), h (B,T,n)")
    cont = lambda x: None if x is None else x.to(torch.float64).contiguous()
    homog = torch.as_tensor(natparam[1][0]).dim() == 2
    lognorm, ex, samples, E_init, E_pair = _LDSInferenceDense.apply(cont(node_J), cont(node_h), cont(node_logZ), cont(eps),
                                                                    natparam)
    ExxT = torch.cat([E_pair[:, :, 0], E_pair[:, -1:, 2]], dim=1)          # E[x_t x_t'] (B,T,n,n): make_node_stats, :163-166
    if homog:
        E_pair = E_pair.sum(1)                                           # (B,3,n,n), differentiable (:172-173)
    return lognorm, (ExxT, ex), (samples if eps is not None else None), (E_init, E_pair)


def _natparam_inference_differentiable(natparam, node_params, eps, plan, pair_stats_grad):
    """lds_inference_differentiable(..., natparam_grad=True): the parameters stay in the autograd graph on their way to
    the kernels' layout (device, float64, contiguous; the init logZ terms summed; (n,n) blocks repeated over time for
    pair_stats_grad), so the cotangents the kernels return in that layout reach the caller's tensors through torch."""
    init_params, pair_params = natparam
    node_J, node_h = node_params[0], node_params[1]
    node_logZ = node_params[2] if len(node_params) == 3 else None
    if not (isinstance(node_h, torch.Tensor) and isinstance(node_J, torch.Tensor)) or node_h.dim() != 3 \
            or node_J.shape != node_h.shape:
        raise ValueError("natparam_grad=True: diagonal node potentials J, h of shape (B,T,n)")
    B, T, n = node_h.shape
    if n > _lib.LDS_MAX_N:
        raise ValueError("natparam_grad=True: latent dimension <= %d (n = %d)" % (_lib.LDS_MAX_N, n))
    dev = node_h.device
    init_J, init_h, init_logZ = _canonical_init_params(init_params, dev, graph=True)
    if tuple(init_J.shape) != (n, n) or tuple(init_h.shape) != (n,):
        raise ValueError("init_params shapes do not match the node potentials")
    J11, J12, J22, logZ_pair, inhomog, pair_batched = _canonical_pair_params(pair_params, B, T, n, dev, graph=True)
    sum_pairs = bool(pair_stats_grad) and not inhomog
    if sum_pairs:
        J11, J12, J22 = (x.expand(max(T - 1, 0), n, n) for x in (J11, J12, J22))
        logZ_pair = logZ_pair.expand(max(T - 1, 0))
        inhomog = True
    if plan is None:
        word = _guarded_plan_options(pair_params, np.ndim(pair_params[0]) != 2)
        word = _default_options if word is None else word
        plan = LDSEStepPlan(B, T, n, dev, inhomog, pair_batched, options=(word & ~_lib.OPT_LEAN_ON) | _lib.OPT_LEAN_OFF)
    elif (plan.B, plan.T, plan.n, plan.inhomog) != (B, T, n, inhomog):
        raise ValueError("plan shape / layout mismatch (pair_stats_grad=True needs a per-step plan: inhomog=True)")
    S = 0 if eps is None else int(eps.shape[2])
    if S <= 16 and plan.lib.svae_lds_inference_is_lean(B, T, n, S, int(inhomog), 1, plan.options):
        raise ValueError("natparam_grad=True needs the full per-step records: this plan's options keep lean ones for this "
                         "shape (make the plan with options | OPT_LEAN_OFF)")
    cont = lambda x: None if x is None else x.to(torch.float64).contiguous()
    params = tuple(x.contiguous() for x in (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair))
    out = _LDSInferenceParams.apply(cont(node_J), cont(node_h), cont(node_logZ), cont(eps), plan, pair_batched, *params)
    lognorm, dxx, ex, samples, E_init, E_pair = out
    if sum_pairs:
        E_pair = E_pair.sum(1)
    return lognorm, (dxx, ex), (samples if eps is not None else None), (E_init, E_pair)


def lds_inference_differentiable(natparam, node_params, eps=None, plan=None, pair_stats_grad=False, natparam_grad=False,
                                 lengths=None):
    """(lognorm (B), (E_node_diagxx, E_node_x) (B,T,n), samples (B,T,S,n) | None, (E_init, E_pair)):
    differentiable w.r.t. node_params = (J (B,T,n), h (B,T,n)[, logZ (B,T)]) through torch autograd.
    Dense node potentials J (B,T,n,n) (the reference's Python path) are accepted too: the first statistic is then the full
    E[x x'] (B,T,n,n), and the gradient w.r.t. J is the symmetric (B,T,n,n) matrix (_LDSInferenceDense).
    Pair parameters (n,n), (T-1,n,n) or (B,T-1,n,n); in the per-step cases E_init (B, n*n+n) and
    E_pair (B,T-1,3,n,n) are differentiable too.

    pair_stats_grad=True with HOMOGENEOUS pair parameters makes E_init and the summed E_pair (B,3,n,n)
    differentiable as well -- the homogeneous branch of the reference's `_compute_stats_grad`
    (cython_lds_inference.pyx:229-231: the cotangent of a sum is the same block at every step): the launch
    uses the per-step layout with the (n,n) parameters repeated over time (T-1 copies, L2-resident), and the
    sum over time is a torch reduction whose backward broadcasts the cotangent to the per-step blocks the
    VJP kernel consumes.  Costs the per-step statistics' HBM traffic, so it is opt-in (no model of the
    reference differentiates these: svae.py:21 keeps them in `saved.stats`).

    natparam_grad=True (n <= 15) lets autograd flow into the natural parameters as well: whichever of init_J, init_h, the
    init logZ terms, J11, J12, J22 and the pair logZ are tensors that require grad receive their gradient -- a shared
    (n,n) parameter the sum over batch and time, a (T-1,n,n) one the sum over the batch.  The gradients of init_J / J11 /
    J22 are symmetric matrices (the forward pass reads the symmetric part), that of J12 is a full one.  The call runs on
    the full per-step records: a plan made here has the lean records switched off; a caller's plan that would keep lean
    records raises ValueError.  The node gradients and (up to 1024 sequences) the forward outputs are the same bits as
    without the flag.

    lengths (B,) int array / tensor (n <= 15, (n,n) pair parameters, diagonal node potentials): per-sequence lengths as in
    natural_lds_estep_general.  Outputs and gradients of sequence b up to its length L are the truncated sequence's;
    every output and every gradient at t >= L is 0, and node_params[b, L:], eps[b, L:] and the cotangents arriving at
    t >= L are never used (they may be NaN).  Not with natparam_grad or pair_stats_grad."""
    if lengths is not None:
        if natparam_grad:
            raise ValueError("lds_inference_differentiable(lengths=): no parameter gradients (natparam_grad=True) with lengths")
        if pair_stats_grad:
            raise ValueError("lds_inference_differentiable(lengths=): no gradients of the pair statistics "
                             "(pair_stats_grad=True) with lengths")
        _ragged_precheck(natparam, node_params, lengths, "lds_inference_differentiable")
    if natparam_grad:
        return _natparam_inference_differentiable(natparam, node_params, eps, plan, pair_stats_grad)
    init_params, pair_params = natparam
    node_J, node_h = node_params[0], node_params[1]
    node_logZ = node_params[2] if len(node_params) == 3 else None
    require_sampler_range(node_h.shape[-1], "lds_inference_differentiable")
    dev = node_h.device
    if node_h.dim() == 3 and node_J.dim() == 4:
        # DENSE node potentials (the reference's Python path, lds_inference.py:65-82): differentiable since round 6 --
        # returns E[x x'] (B,T,n,n) in place of its diagonal, like the reference's make_node_stats (:163-166)
        if plan is not None or pair_stats_grad:
            raise ValueError("dense node potentials: the plan is built internally; the pair statistics are differentiable as they are")
        return _dense_inference_differentiable(natparam, node_params, eps)
    if node_h.dim() != 3 or node_J.shape != node_h.shape:
        raise ValueError("lds_inference_differentiable: node potentials J, h of shape (B,T,n), or dense J (B,T,n,n)")
    B, T, n = node_h.shape
    init_J, init_h, init_logZ = _canonical_init_params(init_params, dev)
    J11, J12, J22, logZ_pair, inhomog, pair_batched = _canonical_pair_params(pair_params, B, T, n, dev)
    sum_pairs = bool(pair_stats_grad) and not inhomog
    if sum_pairs:
        J11, J12, J22 = (x.expand(max(T - 1, 0), n, n).contiguous() for x in (J11, J12, J22))
        logZ_pair = logZ_pair.reshape(1).expand(max(T - 1, 0)).contiguous()
        inhomog = True
    if plan is None:
        plan = LDSEStepPlan(B, T, n, dev, inhomog, pair_batched,
                            options=_guarded_plan_options(pair_params, np.ndim(pair_params[0]) != 2))
    elif plan.inhomog != inhomog:
        raise ValueError("plan layout mismatch (pair_stats_grad=True needs a per-step plan: inhomog=True)")
    params = (init_J, init_h, init_logZ, J11, J12, J22, logZ_pair)
    cont = lambda x: None if x is None else x.to(torch.float64).contiguous()
    fn = _LDSInference
    if n > _lib.LDS_MAX_N:
        from .lds_large import LDSInferenceLarge as fn     # tile-kernel forward, tile VJP kernels backward
    if lengths is not None:
        lengths = plan._ragged(lengths, "lds_inference_differentiable", pair_batched)      # (checks; one host -> device copy)
        out = fn.apply(cont(node_J), cont(node_h), cont(node_logZ), cont(eps), plan, params, pair_batched, lengths)
    else:
        out = fn.apply(cont(node_J), cont(node_h), cont(node_logZ), cont(eps), plan, params, pair_batched)
    lognorm, dxx, ex, samples, E_init, E_pair = out
    if sum_pairs:
        E_pair = E_pair.sum(1)                     # (B,3,n,n), differentiable
    return lognorm, (dxx, ex), (samples if eps is not None else None), (E_init, E_pair)
