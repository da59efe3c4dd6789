"""HMM E-step on MI355X; mirrors /root/reference/svae/hmm/hmm_inference.py.

  hmm_estep(natparam) -> (log_normalizer, (E_init, E_trans, E_states))      (:21-41)
  hmm_logZ(natparam)  -> log_normalizer                                      (:12-17, pyx:93-121)
  redone_sequences(workspace, B, T, K) -> which sequences of that E-step took the log-space route
  hmm_estep_chunked(natparam, chunk) -> hmm_estep for LONG sequences, the steps cut into chunks worked on side by side;
  hmm_logZ_chunked(natparam, chunk) its log-normaliser alone; chunked_redone_sequences(workspace, B, T, K, chunk) which
                                 sequences the serial route recomputed; K <= 16 (csrc/hmm_estep_chunked.hip)
  hmm_viterbi(natparam) -> most probable state path (and its score)          (:54-63; csrc/hmm_viterbi.hip)
  hmm_viterbi_chunked(natparam, chunk) -> hmm_viterbi for LONG sequences, the steps cut into chunks decoded side by side;
                                 K <= 16 (csrc/hmm_viterbi_chunked.hip)
  hmm_sample(natparam, num_samples) -> state paths drawn from the posterior  (csrc/hmm_sample.hip)
  sample_redone_sequences(workspace, B, T, K) -> which sequences of that call had their filter redone in log space
  hmm_estep_differentiable(natparam) -> hmm_estep's outputs, with gradients of all four to all three inputs
                                                                             (csrc/hmm_estep_vjp.hip)
  hmm_estep_perstep(natparam) -> hmm_estep for PER-STEP transition potentials, pair (T-1,K,K) or (B,T-1,K,K); E_trans is
                                 then per step too, (…,T-1,K,K)                (csrc/hmm_estep_perstep.hip)
  hmm_logZ_perstep(natparam), hmm_logZ_perstep_differentiable(natparam) -> its log-normaliser, with gradients to all three
  hmm_estep_perstep_differentiable(natparam) -> hmm_estep_perstep's outputs, with gradients of all four to all three
                                 inputs; hmm_estep_perstep_vjp is its backward pass (csrc/hmm_estep_perstep_vjp.hip)
  hmm_viterbi_perstep(natparam), hmm_sample_perstep(natparam, num_samples) -> hmm_viterbi / hmm_sample for per-step
                                 transition potentials                        (csrc/hmm_viterbi_perstep.hip, hmm_sample_perstep.hip)

natparam = (init_params (K), pair_params (K,K), node_params (T,K)) are LOG potentials, as in the
reference.  New: node_params may be (B,T,K) (and pair_params (B,K,K)); outputs then carry a leading
batch axis.  All arithmetic in libsvae_hip.so (svae_hmm_estep_f64); no CPU fallback.

Per-sequence lengths: every function takes lengths= (B,) integers with (B,T,K) node potentials -- one padded batch,
sequence b occupying steps 0 .. lengths[b]-1.  logZ, E_init, E_trans, E_states[b, :L], states[b, :L] and the score are
those of the sequence cut to its length; E_states[b, L:] is exactly 0, states[b, L:] is -1, and nothing stored at
t >= L is read (it may be NaN).  A length outside 1..T is device data: clamped, and recorded in a persistent status
word that check=True (or check_lengths_status) reads (svae_hmm_ragged_estep_f64 / svae_hmm_ragged_viterbi_f64 /
svae_hmm_ragged_sample_f64; sampled labels are (B,S,T) with states[b, :, L:] = -1, and u[b, :, L:] is not read either).
"""
import numpy as np
import torch

from .. import _lib

HMM_MAX_K = 64      # (K <= 16: DPP-row kernels; 17 .. 64: one wavefront per sequence, csrc/hmm_estep_wide.hip)


def _dev64(x, device):
    # dtype given up front: torch.as_tensor(python_float) alone would round to float32
    t = x.detach() if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float64)
    return t.to(device=device, dtype=torch.float64).contiguous()


_STATUS = {}


def _status_word(device):
    """The persistent (1,) int32 status word of a device, handed to the ragged kernels as their `info` pointer: they only
    ever OR into it (a length outside 1..T), so an earlier call's failure survives later clean ones until it is read."""
    key = str(torch.device(device))
    word = _STATUS.get(key)
    if word is None:
        _STATUS[key] = word = torch.zeros(1, dtype=torch.int32, device=device)
    return word


def check_lengths_status(device=None):
    """Read (synchronising) and clear the status word of `device`; FloatingPointError if a ragged call since the last
    check saw a length outside 1..T."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    word = _status_word(dev)
    if int(word.item()) != 0:
        word.zero_()
        raise FloatingPointError("hmm: a sequence length outside 1..T was clamped (lengths= is device data)")


def _lengths_arg(lengths, node_params):
    """Validate lengths= against the node potentials BEFORE anything is converted or launched; the (B,) int32 device
    tensor (a contiguous int32 device tensor is used as it is, a host array is copied once)."""
    shape = tuple(node_params.shape) if hasattr(node_params, "shape") else np.shape(node_params)
    if len(shape) != 3:
        raise ValueError("lengths= needs batched node_params (B,T,K)")
    is_t = isinstance(lengths, torch.Tensor)
    ls = tuple(lengths.shape) if is_t else np.shape(lengths)
    if ls != (shape[0],):
        raise ValueError("lengths must have shape (B,) = (%d,), got %r" % (shape[0], ls))
    if (lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool) if is_t \
            else np.asarray(lengths).dtype.kind not in "iu":
        raise ValueError("lengths must be integers")
    dev = node_params.device if isinstance(node_params, torch.Tensor) and node_params.is_cuda \
        else torch.device("cuda", torch.cuda.current_device())
    if is_t:
        return lengths.to(device=dev, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.asarray(lengths).astype(np.int32), device=dev)


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _node_shape(node_s):
    """(B, T, K, batched) of node potentials of shape node_s; ValueError for a wrong rank, K outside 1..64 or T = 0"""
    if len(node_s) not in (2, 3):
        raise ValueError("node_params must be (T,K) or (B,T,K)")
    batched = len(node_s) == 3
    B = node_s[0] if batched else 1
    T, K = node_s[-2:]
    if not (1 <= K <= HMM_MAX_K):
        raise ValueError("number of states K=%d outside 1..%d" % (K, HMM_MAX_K))
    if T < 1:
        raise ValueError("node_params has no steps")
    return B, T, K, batched


def _shapes(natparam):
    """(B, T, K, batched, pair_batched) of a natparam with ONE transition matrix per sequence -- init (K), pair (K,K) or
    (B,K,K), node (T,K) or (B,T,K) --, from shapes alone: every refusal is a ValueError raised before anything is
    converted, copied or launched (no device is touched)."""
    init_s, pair_s, node_s = (_shape_of(x) for x in natparam)
    B, T, K, batched = _node_shape(node_s)
    pair_batched = len(pair_s) == 3
    if init_s != (K,) or pair_s[-2:] != (K, K) or len(pair_s) not in (2, 3) or (pair_batched and pair_s[0] != B):
        raise ValueError("init/pair parameter shapes do not match the node potentials")
    return B, T, K, batched, pair_batched


def _on_device(natparam, lengths):
    """(lens, dev, (init, pair, node)) of a call whose shapes have been accepted: the validated (B,) int32 lengths or
    None, the device, and the three leaves there as contiguous float64 (only their addresses are passed on)"""
    node_params = natparam[2]
    lens = None if lengths is None else _lengths_arg(lengths, node_params)
    dev = node_params.device if isinstance(node_params, torch.Tensor) and node_params.is_cuda \
        else torch.device("cuda", torch.cuda.current_device())
    return lens, dev, tuple(_dev64(x, dev) for x in natparam)


def _workspace(workspace, nbytes, B, T, K, dev):
    """(tensor, its size in bytes): the caller's workspace as it is, else a fresh one of nbytes(B, T, K) bytes"""
    if workspace is not None:
        return workspace, workspace.numel() * workspace.element_size()
    wsb = int(nbytes(max(B, 1), T, K))
    return torch.empty(wsb, dtype=torch.uint8, device=dev), wsb


def _call(name, dev, lens, check, *args):
    """Entry point `name` of the library on args and the current stream of dev: RuntimeError for a return code other than
    0; then, for a call with lengths and check=True, the status word is read"""
    _lib.check(getattr(_lib.load(), name)(*args, _lib.current_stream(dev)), name)
    if lens is not None and check:
        check_lengths_status(dev)


def _info(lens, dev):
    return None if lens is None else _lib.ptr(_status_word(dev))


def _unbatch(batched, *xs):
    """xs, without their leading batch axis for an unbatched call (None stays None)"""
    return xs if batched else tuple(None if x is None else x[0] for x in xs)


def _sample_shapes(num_samples, u, B, T, batched):
    """S = num_samples as an int; ValueError for a count that is no integer >= 1, B S T labels that a 32-bit index
    cannot address, or uniforms of another shape than (B,S,T) ((S,T) for the unbatched call)"""
    S = int(num_samples)
    if S != num_samples or S < 1:
        raise ValueError("num_samples must be an integer >= 1, got %r" % (num_samples,))
    if B * S * T >= 2 ** 31:
        raise ValueError("B * num_samples * T = %d is not below 2^31" % (B * S * T))
    if u is not None and _shape_of(u) != ((B, S, T) if batched else (S, T)):
        raise ValueError("u must have shape %r, got %r" % ((B, S, T) if batched else (S, T), _shape_of(u)))
    return S


def _uniforms(u, generator, B, S, T, dev):
    """the (B,S,T) float64 uniforms on dev: the caller's, or drawn there with `generator`"""
    if u is None:
        return torch.rand(B, S, T, dtype=torch.float64, device=dev, generator=generator)
    return _dev64(u, dev).reshape(B, S, T)


def _cotangents(cotangents, shapes, batched):
    """[g_logZ, g_init, g_trans, g_states] of cotangents = (g_logZ, (g_init, g_trans, g_states)), each None or of its
    shape in `shapes` (without the batch axis for an unbatched call): ValueError otherwise"""
    g_logZ, (g_init, g_trans, g_states) = cotangents
    cots = [g_logZ, g_init, g_trans, g_states]
    for name, x, shape in zip(("g_logZ", "g_init", "g_trans", "g_states"), cots, shapes):
        want = shape if batched else shape[1:]
        if x is not None and _shape_of(x) != want:
            raise ValueError("%s must have shape %r, got %r" % (name, want, _shape_of(x)))
    return cots


def hmm_estep(natparam, workspace=None, lengths=None, check=False):
    B, T, K, batched, pair_batched = _shapes(natparam)
    lens, dev, leaves = _on_device(natparam, lengths)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_workspace_bytes, B, T, K, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    logZ = torch.empty(B, **f64)
    E_init, E_trans, E_states = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
    model, out = (B, T, K, int(pair_batched), *map(p, leaves)), (p(logZ), p(E_init), p(E_trans), p(E_states))
    if lens is not None:
        _call("svae_hmm_ragged_estep_f64", dev, lens, check, *model, p(lens), *out, _info(lens, dev), p(ws), wsb)
    else:
        _call("svae_hmm_estep_f64", dev, None, False, *model, *out, p(ws), wsb)
    logZ, E_init, E_trans, E_states = _unbatch(batched, logZ, E_init, E_trans, E_states)
    return logZ, (E_init, E_trans, E_states)


def redone_sequences(workspace, B, T, K):
    """Which sequences of the last hmm_estep call on `workspace` left the range of the scaled recursions and were
    recomputed in log space: a (B,) bool tensor read from the REDO words the kernels write into the first record of
    every sequence (csrc/hmm_args.hpp: record stride and flag entry 50 / 49 for K <= 16, KP + 2 / KP + 1 with KP = 32 or 64
    padded states above).  A fallback is never silent: by its operation count a sequence costs roughly 10x more on that route (an estimate, not
    a measurement), and this says which did.
    For an indexed launch (the SLDS sweep) B counts the rows of the arrays, not the slots of the launch."""
    if not (1 <= K <= HMM_MAX_K):
        raise ValueError("number of states K=%d outside 1..%d" % (K, HMM_MAX_K))
    kp = 32 if K <= 32 else 64
    rec, flag = (50, 49) if K <= 16 else (kp + 2, kp + 1)
    ws = workspace.reshape(-1)
    if ws.dtype != torch.float64 or ws.numel() < B * T * rec:
        raise ValueError("workspace is not the float64 workspace of a (B=%d, T=%d, K=%d) E-step" % (B, T, K))
    return ws[:B * T * rec].view(B, T * rec)[:, flag] != 0


def hmm_logZ(natparam, lengths=None):
    return hmm_estep(natparam, lengths=lengths)[0]


# ---- the E-step partitioned in time (svae_hmm_chunked_estep_f64, csrc/hmm_estep_chunked.hip) -------------------------------
HMM_CHUNKED_MAX_K = 16


def _chunked_shapes(natparam, chunk, what="E-step", serial="hmm_estep", default="svae_hmm_chunked_default_chunk"):
    """(B, T, K, batched, pair_batched, chunk) of a chunked call, from shapes alone (hmm_estep's refusals, then K > 16 and
    a chunk that is no integer >= 2); chunk=None is resolved to the library's pick, which needs no device.  what / serial /
    default: the chunked unit's name, the serial function a K > 16 refusal points to, and the entry that picks the chunk
    (its name, or a callable of (B, T, K))"""
    B, T, K, batched, pair_batched = _shapes(natparam)
    if K > HMM_CHUNKED_MAX_K:
        raise ValueError("number of states K=%d above %d: the time-chunked %s has DPP-row kernels only; use %s"
                         % (K, HMM_CHUNKED_MAX_K, what, serial))
    if chunk is None:
        pick = default if callable(default) else getattr(_lib.load(), default)
        chunk = max(2, int(pick(B, T, K)))
    elif isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 2:
        raise ValueError("chunk must be an integer >= 2, got %r" % (chunk,))
    return B, T, K, batched, pair_batched, int(min(chunk, 2 ** 31 - 1))


def _chunked_call(natparam, chunk, workspace, want_stats):
    B, T, K, batched, pair_batched, chunk = _chunked_shapes(natparam, chunk)
    _, dev, leaves = _on_device(natparam, None)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lambda b, t, k: lib.svae_hmm_chunked_workspace_bytes(b, t, k, chunk), B, T, K, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    logZ = torch.empty(B, **f64)
    stats = (torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)) if want_stats \
        else (None, None, None)
    _call("svae_hmm_chunked_estep_f64", dev, None, False, B, T, K, int(pair_batched), chunk, *map(p, leaves), p(logZ),
          *map(p, stats), p(ws), wsb)
    return _unbatch(batched, logZ, *stats)


def hmm_estep_chunked(natparam, chunk=None, workspace=None):
    """hmm_estep for LONG sequences: the T steps are cut into chunks of `chunk` steps that the chip works on side by side
    (per chunk a K x K transfer operator, a scan over the chunks, then the E-step of every chunk; include/svae_hip.h,
    svae_hmm_chunked_estep_f64), where hmm_estep runs one chain of T dependent steps per sequence whatever the batch.
    natparam and the result (logZ, (E_init, E_trans, E_states)) are hmm_estep's -- (T,K) or (B,T,K) node potentials, a
    shared or (B,K,K) pair parameter --, to rounding; K <= 16.  The range contract is hmm_estep's: a sequence that leaves
    the range of the scaled chunked arithmetic is recomputed whole by hmm_estep's kernels, and
    chunked_redone_sequences(workspace, B, T, K, chunk) says which were.
    chunk: an integer >= 2; None takes svae_hmm_chunked_default_chunk(B, T, K); chunk >= T is hmm_estep, bit for bit.
    workspace: a contiguous device tensor of at least svae_hmm_chunked_workspace_bytes(B, T, K, chunk) bytes."""
    logZ, E_init, E_trans, E_states = _chunked_call(natparam, chunk, workspace, True)
    return logZ, (E_init, E_trans, E_states)


def hmm_logZ_chunked(natparam, chunk=None):
    """The log-normaliser of hmm_estep_chunked alone, bit for bit: the chunk operators and the scan over them, without
    the per-chunk E-step -- K forward filters over `chunk` steps and a scan over T / chunk operators."""
    return _chunked_call(natparam, chunk, None, False)[0]


def chunked_redone_sequences(workspace, B, T, K, chunk):
    """Which sequences of the last hmm_estep_chunked call on `workspace` left the range of the chunked arithmetic and
    were recomputed by the serial route: a (B,) bool tensor read from the B int32 route words the workspace opens with
    (csrc/hmm_args.hpp).  The counterpart of redone_sequences; a call with chunk >= T is the serial route for every
    sequence, writes no route word and reports none."""
    if not (1 <= K <= HMM_CHUNKED_MAX_K):
        raise ValueError("number of states K=%d outside 1..%d" % (K, HMM_CHUNKED_MAX_K))
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 2:
        raise ValueError("chunk must be an integer >= 2, got %r" % (chunk,))
    ws = workspace.reshape(-1)
    need = int(_lib.load().svae_hmm_chunked_workspace_bytes(max(B, 1), T, K, int(min(chunk, 2 ** 31 - 1))))
    if ws.numel() * ws.element_size() < need:
        raise ValueError("workspace is smaller than that of a (B=%d, T=%d, K=%d, chunk=%d) chunked E-step" % (B, T, K, chunk))
    if chunk >= T:
        return torch.zeros(B, dtype=torch.bool, device=ws.device)
    return ws.view(torch.uint8)[:4 * B].view(torch.int32) != 0


def hmm_viterbi(natparam, workspace=None, return_score=False, lengths=None, check=False):
    """Most probable state path under the LOG potentials hmm_estep takes (entries may be -inf):
    labels torch.int32 (T,), or (B,T) when node_params is (B,T,K); with return_score also the path's score
    (0-d, or (B)).  The arithmetic is defined in include/svae_hip.h (svae_hmm_viterbi_f64): fp64 additions in a fixed
    order, ties to the lowest index -- labels and score are reproducible bit for bit.
    workspace: any contiguous device tensor of at least svae_hmm_viterbi_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers, see the module docstring -- labels from a sequence's length on are -1."""
    B, T, K, batched, pair_batched = _shapes(natparam)
    lens, dev, leaves = _on_device(natparam, lengths)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_viterbi_workspace_bytes, B, T, K, dev)
    states = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev) if return_score else None
    model = (B, T, K, int(pair_batched), *map(p, leaves))
    if lens is not None:
        _call("svae_hmm_ragged_viterbi_f64", dev, lens, check, *model, p(lens), p(states), p(score), _info(lens, dev),
              p(ws), wsb)
    else:
        _call("svae_hmm_viterbi_f64", dev, None, False, *model, p(states), p(score), p(ws), wsb)
    states, score = _unbatch(batched, states, score)
    return (states, score) if return_score else states


def hmm_viterbi_chunked(natparam, chunk=None, workspace=None, return_score=False):
    """hmm_viterbi for LONG sequences: the T steps are cut into chunks of `chunk` steps that the chip works on side by side
    (per chunk a K x K max-plus operator, a scan over the chunks for the recursion's value at every chunk boundary, then
    every chunk decoded and chased from all K of its end states at once, the end states resolved across the chunks and the
    labels gathered; include/svae_hip.h, svae_hmm_chunked_viterbi_f64), where hmm_viterbi runs one chain of T dependent
    steps and a backtrace of T look-ups per sequence whatever the batch.  natparam and the result are hmm_viterbi's --
    (T,K) or (B,T,K) node potentials, a shared or (B,K,K) pair parameter, entries finite or -inf; int32 labels (T,) or
    (B,T), with return_score also the score --; K <= 16; there is no lengths=.
    Against hmm_viterbi: (a) chunk >= T runs hmm_viterbi's launch and nothing else, the same bits; (b) where every fp64
    add of the recursion is exact (potentials that are multiples of 2^-q with T max|potential| 2^q < 2^53, -inf included)
    labels and score are hmm_viterbi's bit for bit, ties included; (c) otherwise the labels are a path whose serially
    summed score lies within 4 T 2^-53 A of hmm_viterbi's score, and so does the returned score, A = max|init| +
    sum_t max_k |node_t| + (T-1) max|pair| over the finite entries; (d) NaN inputs give unspecified labels in 0..K-1 and no
    fault; (e) the outputs are reproducible bit for bit (no atomics), the call is asynchronous, allocates nothing inside
    the library and is safe under graph capture.
    chunk: an integer >= 2; None takes svae_hmm_chunked_viterbi_default_chunk(B, T, K).
    workspace: a contiguous, 16-byte aligned device tensor of at least svae_hmm_chunked_viterbi_workspace_bytes(B, T, K,
    chunk) bytes."""
    B, T, K, batched, pair_batched, chunk = _chunked_shapes(natparam, chunk, "Viterbi decoder", "hmm_viterbi",
                                                            "svae_hmm_chunked_viterbi_default_chunk")
    _, dev, leaves = _on_device(natparam, None)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lambda b, t, k: lib.svae_hmm_chunked_viterbi_workspace_bytes(b, t, k, chunk), B, T, K, dev)
    states = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev) if return_score else None
    _call("svae_hmm_chunked_viterbi_f64", dev, None, False, B, T, K, int(pair_batched), chunk, *map(p, leaves), p(states),
          p(score), p(ws), wsb)
    states, score = _unbatch(batched, states, score)
    return (states, score) if return_score else states


def hmm_sample(natparam, num_samples=1, u=None, generator=None, workspace=None, return_logZ=False, lengths=None,
               check=False):
    """State paths drawn from the posterior p(z | potentials) under the LOG potentials hmm_viterbi takes (entries may be
    -inf), by forward filtering and backward sampling: labels torch.int32 (S,T), or (B,S,T) when node_params is (B,T,K),
    S = num_samples; labels[:, s] is a (B,T) label array of the form hmm_viterbi returns.  With return_logZ also the
    log-normaliser the filter computes (0-d, or (B)).  The arithmetic is defined in include/svae_hip.h
    (svae_hmm_sample_f64): a state with a forbidden (-inf) transition or observation is never drawn.  The filter keeps
    the E-step's range contract: a sequence that leaves the range of the scaled recursion is filtered again, all of it,
    in log space, and sample_redone_sequences(workspace, B, T, K) says which were.
    u: the uniforms, (B,S,T) ((S,T) for the unbatched call); None draws torch.rand fp64 on the device with `generator`.
    workspace: any contiguous device tensor of at least svae_hmm_sample_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers, see the module docstring -- labels from a sequence's length on are -1."""
    B, T, K, batched, pair_batched = _shapes(natparam)
    S = _sample_shapes(num_samples, u, B, T, batched)
    lens, dev, leaves = _on_device(natparam, lengths)
    u = _uniforms(u, generator, B, S, T, dev)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_sample_workspace_bytes, B, T, K, dev)
    states = torch.empty(B, S, T, dtype=torch.int32, device=dev)
    logZ = torch.empty(B, dtype=torch.float64, device=dev) if return_logZ else None
    model = (B, T, K, S, int(pair_batched), *map(p, leaves))
    if lens is not None:
        _call("svae_hmm_ragged_sample_f64", dev, lens, check, *model, p(lens), p(u), p(states), p(logZ),
              _info(lens, dev), p(ws), wsb)
    else:
        _call("svae_hmm_sample_f64", dev, None, False, *model, p(u), p(states), p(logZ), p(ws), wsb)
    states, logZ = _unbatch(batched, states, logZ)
    return (states, logZ) if return_logZ else states


def hmm_sample_chunked(natparam, num_samples=1, u=None, generator=None, chunk=None, workspace=None, return_logZ=False):
    """hmm_sample for LONG sequences: the T steps are cut into chunks of `chunk` steps that the chip works on side by side
    (the chunked E-step's operators and forward scan for the filtered message at every chunk boundary, every chunk
    filtered from there, then -- the uniforms being fixed -- every backward draw as a map from the next state to this one,
    chased, resolved and gathered as the chunked Viterbi decoder does its back-pointers; include/svae_hip.h,
    svae_hmm_chunked_sample_f64), where hmm_sample runs a filter of T and a draw of T dependent steps per chain whatever
    the batch.  natparam and the result are hmm_sample's -- (T,K) or (B,T,K) node potentials, a shared or (B,K,K) pair
    parameter, entries finite or -inf; int32 labels (S,T) or (B,S,T), with return_logZ also the log-normaliser, which is
    hmm_logZ_chunked's bit for bit at the same chunk --; K <= 16; there is no lengths=.
    The weights and the selection rule are hmm_sample's, on filtered distributions that differ from its own in rounding;
    chunk >= T runs hmm_sample's launches and nothing else, the same bits.  The range contract is hmm_sample's: a sequence
    that leaves the range of the scaled chunked arithmetic is filtered again, all of it, in log space and drawn with the
    log-space weights, and sample_redone_sequences(workspace, B, T, K) says which were (it reads this call's workspace
    unchanged).  NaN potentials give unspecified labels in 0..K-1 and no fault.  The outputs are reproducible bit for bit
    (no atomics); the call is asynchronous, allocates nothing inside the library and is safe under graph capture.
    u: the uniforms, (B,S,T) ((S,T) for the unbatched call); None draws torch.rand fp64 on the device with `generator`.
    chunk: an integer >= 2; None takes svae_hmm_chunked_sample_default_chunk(B, T, K, S).
    workspace: a contiguous, 16-byte aligned device tensor of at least svae_hmm_chunked_sample_workspace_bytes(B, T, K, S,
    chunk) bytes."""
    B, T, K, batched, pair_batched = _shapes(natparam)
    S = _sample_shapes(num_samples, u, B, T, batched)
    B, T, K, batched, pair_batched, chunk = _chunked_shapes(
        natparam, chunk, "sampler", "hmm_sample", lambda b, t, k: _lib.load().svae_hmm_chunked_sample_default_chunk(b, t, k, S))
    _, dev, leaves = _on_device(natparam, None)
    u = _uniforms(u, generator, B, S, T, dev)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lambda b, t, k: lib.svae_hmm_chunked_sample_workspace_bytes(b, t, k, S, chunk), B, T, K, dev)
    states = torch.empty(B, S, T, dtype=torch.int32, device=dev)
    logZ = torch.empty(B, dtype=torch.float64, device=dev) if return_logZ else None
    _call("svae_hmm_chunked_sample_f64", dev, None, False, B, T, K, S, int(pair_batched), chunk, *map(p, leaves), p(u),
          p(states), p(logZ), p(ws), wsb)
    states, logZ = _unbatch(batched, states, logZ)
    return (states, logZ) if return_logZ else states


def sample_redone_sequences(workspace, B, T, K):
    """Which sequences of the last hmm_sample call on `workspace` left the range of the scaled filter and were filtered
    again in log space: a (B,) bool tensor read from the records themselves (csrc/hmm_sample_kernel.hpp: B T KP doubles,
    KP = 16, 32 or 64; a scaled record a_t sums to 1 and so has a positive entry, a log-space record log a_t has none).
    The counterpart of redone_sequences for the sampler; with lengths= every sequence has its step-0 record.
    It reads the workspace of an hmm_sample_chunked call unchanged: that call keeps the same records at the head of its
    workspace, and a sequence that left the range of its chunked stages is filtered again in log space in the same way."""
    if not (1 <= K <= HMM_MAX_K):
        raise ValueError("number of states K=%d outside 1..%d" % (K, HMM_MAX_K))
    kp = 16 if K <= 16 else (32 if K <= 32 else 64)
    ws = workspace.reshape(-1)
    if ws.dtype != torch.float64 or ws.numel() < B * T * kp:
        raise ValueError("workspace is not the float64 workspace of a (B=%d, T=%d, K=%d) sampling call" % (B, T, K))
    return ~(ws[:B * T * kp].view(B, T * kp)[:, :K] > 0).any(dim=1)


class _HMMLogZ(torch.autograd.Function):
    """log Z of a batch of HMMs, differentiable w.r.t. the node log-potentials: the gradient is the
    matrix of state marginals the same kernel launch returns (hmm_logZ_grad, cython_hmm_inference.pyx:
    126-166, restricted to the node argument -- all the SLDS-SVAE differentiates, slds_svae.py:150-155)."""

    @staticmethod
    def forward(ctx, node_params, init_params, pair_params, lengths=None):
        logZ, (_, _, E_states) = hmm_estep((init_params, pair_params, node_params), lengths=lengths)
        ctx.save_for_backward(E_states)
        return logZ

    @staticmethod
    def backward(ctx, g):
        (E_states,) = ctx.saved_tensors
        return g.reshape(g.shape + (1,) * (E_states.dim() - g.dim())) * E_states, None, None, None


def hmm_logZ_differentiable(natparam, lengths=None):
    """hmm_logZ with gradients flowing to node_params ((T,K) or (B,T,K)).  With lengths= the gradient is g * E_states of
    the same launch: exactly 0 from a sequence's length on."""
    init_params, pair_params, node_params = natparam
    return _HMMLogZ.apply(node_params, init_params, pair_params, lengths)


def hmm_estep_vjp(natparam, cotangents, workspace=None, lengths=None, check=False):
    """The reverse-mode derivative of hmm_estep (svae_hmm_estep_vjp_f64, include/svae_hip.h): cotangents = (g_logZ,
    (g_init, g_trans, g_states)) in the shapes hmm_estep returns, each may be None (zero).  Returns the PER-SEQUENCE
    gradients (d_init (B,K), d_pair (B,K,K), d_node (B,T,K)) -- without the leading axis for unbatched (T,K) node
    potentials --; a shared init or pair parameter's gradient is their sum over the batch.
    workspace: a contiguous float64 device tensor of at least svae_hmm_estep_vjp_workspace_bytes(B,T,K) bytes; afterwards
    vjp_redone_sequences(workspace, B, T, K) says which sequences took the log-space route."""
    B, T, K, batched, pair_batched = _shapes(natparam)
    cots = _cotangents(cotangents, ((B,), (B, K), (B, K, K), (B, T, K)), batched)
    lens, dev, leaves = _on_device(natparam, lengths)
    cots = [None if x is None else _dev64(x, dev) for x in cots]
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_estep_vjp_workspace_bytes, B, T, K, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    d_init, d_pair, d_node = torch.empty(B, K, **f64), torch.empty(B, K, K, **f64), torch.empty(B, T, K, **f64)
    model, grads = (B, T, K, int(pair_batched), *map(p, leaves)), (*map(p, cots), p(d_init), p(d_pair), p(d_node))
    if lens is not None:
        _call("svae_hmm_ragged_estep_vjp_f64", dev, lens, check, *model, p(lens), *grads, _info(lens, dev), p(ws), wsb)
    else:
        _call("svae_hmm_estep_vjp_f64", dev, None, False, *model, *grads, p(ws), wsb)
    return _unbatch(batched, d_init, d_pair, d_node)


def vjp_redone_sequences(workspace, B, T, K):
    """Which sequences of the last hmm_estep_vjp call on `workspace` left the range of the scaled recursions and were
    recomputed in log space: a (B,) bool tensor read from the route flags behind the workspace's records
    (csrc/hmm_estep_vjp_kernel.hpp: B T 2 KP doubles of records, KP = 16, 32 or 64, then one flag per sequence).  The
    counterpart of redone_sequences for the E-step's derivative."""
    if not (1 <= K <= HMM_MAX_K):
        raise ValueError("number of states K=%d outside 1..%d" % (K, HMM_MAX_K))
    kp = 16 if K <= 16 else (32 if K <= 32 else 64)
    ws = workspace.reshape(-1)
    if ws.dtype != torch.float64 or ws.numel() < B * T * 2 * kp + B:
        raise ValueError("workspace is not the float64 workspace of a (B=%d, T=%d, K=%d) E-step derivative" % (B, T, K))
    return ws[B * T * 2 * kp:B * T * 2 * kp + B] != 0


class _HMMEStep(torch.autograd.Function):
    """hmm_estep with its reverse-mode derivative: forward is hmm_estep unchanged, backward one call of
    svae_hmm_estep_vjp_f64 (or its ragged form) on the saved potentials."""

    @staticmethod
    def forward(ctx, init_params, pair_params, node_params, lengths, check):
        logZ, (E_init, E_trans, E_states) = hmm_estep((init_params, pair_params, node_params), lengths=lengths, check=check)
        ctx.save_for_backward(init_params, pair_params, node_params)
        ctx.lengths = lengths
        return logZ, E_init, E_trans, E_states

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logZ, g_init, g_trans, g_states):
        init_params, pair_params, node_params = ctx.saved_tensors
        d_init, d_pair, d_node = hmm_estep_vjp((init_params, pair_params, node_params),
                                               (g_logZ, (g_init, g_trans, g_states)), lengths=ctx.lengths)
        if node_params.dim() == 3:
            d_init = d_init.sum(0)                    # shared parameters receive the batch sum
            if pair_params.dim() == 2:
                d_pair = d_pair.sum(0)
        need = ctx.needs_input_grad
        like = lambda d, x: d.to(device=x.device, dtype=x.dtype)          # noqa: E731
        return (like(d_init, init_params) if need[0] else None, like(d_pair, pair_params) if need[1] else None,
                like(d_node, node_params) if need[2] else None, None, None)


def hmm_estep_differentiable(natparam, lengths=None, check=False):
    """hmm_estep -> (logZ, (E_init, E_trans, E_states)) with gradients of all four outputs flowing to whichever of
    init_params (K), pair_params (K,K) or (B,K,K) and node_params (T,K) or (B,T,K) require them (torch tensors on the
    device).  The outputs are those of hmm_estep, bit for bit; the backward pass is one call of svae_hmm_estep_vjp_f64
    (once differentiable): a shared init or pair parameter receives the sum over the batch, a per-sequence pair parameter
    its own block.  With lengths= the gradient is that of every sequence cut to its length: exactly 0 from there on."""
    init_params, pair_params, node_params = natparam
    for x in (init_params, pair_params, node_params):
        if not isinstance(x, torch.Tensor):
            raise TypeError("hmm_estep_differentiable takes torch tensors")
    logZ, E_init, E_trans, E_states = _HMMEStep.apply(init_params, pair_params, node_params, lengths, check)
    return logZ, (E_init, E_trans, E_states)


# ---- per-step transition potentials (svae_hmm_perstep_estep_f64, csrc/hmm_estep_perstep.hip) --------------------------------
def _perstep_shapes(natparam):
    """(B, T, K, batched, pair_batched) of a per-step natparam, from shapes alone: every refusal is a ValueError raised
    before anything is converted, copied or launched."""
    init_s, pair_s, node_s = (_shape_of(x) for x in natparam)
    B, T, K, batched = _node_shape(node_s)
    if init_s != (K,):
        raise ValueError("init_params must have shape (K,) = (%d,), got %r" % (K, init_s))
    if len(pair_s) not in (3, 4):
        raise ValueError("per-step pair_params must be (T-1,K,K) or (B,T-1,K,K), got %r" % (pair_s,))
    pair_batched = len(pair_s) == 4
    if pair_batched and not batched:
        raise ValueError("per-sequence pair_params (B,T-1,K,K) need batched node_params (B,T,K)")
    if pair_s[-2:] != (K, K):
        raise ValueError("pair_params must end in (K,K) = (%d,%d), got %r" % (K, K, pair_s))
    if pair_s[-3] != T - 1:
        raise ValueError("pair_params must hold T-1 = %d per-step matrices, got %d" % (T - 1, pair_s[-3]))
    if pair_batched and pair_s[0] != B:
        raise ValueError("pair_params has batch %d, node_params %d" % (pair_s[0], B))
    return B, T, K, batched, pair_batched


def hmm_estep_perstep(natparam, workspace=None, lengths=None, check=False, want_trans=True):
    """The E-step of an HMM whose transition potentials change with time:
        log p(z) ∝ init[z_0] + sum_t pair[t][z_t][z_{t+1}] + sum_t node[t][z_t]
    natparam = (init (K), pair (T-1,K,K) or (B,T-1,K,K), node (T,K) or (B,T,K)), LOG potentials, finite or -inf.
    Returns (logZ, (E_init, E_trans, E_states)) with E_trans PER STEP, (…,T-1,K,K): E_trans[…,t] is the posterior pairwise
    marginal of (z_t, z_{t+1}) -- or None with want_trans=False (the other three do not change a bit).  Unbatched node
    potentials return unbatched results.  One route, log space throughout (include/svae_hip.h): there is no fallback.
    workspace: a contiguous float64 device tensor of at least svae_hmm_perstep_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers, see the module docstring -- E_states[b, L:] and E_trans[b, L-1:] are exactly 0, and neither
    node[b, L:] nor pair[b, L-1:] is read."""
    B, T, K, batched, pair_batched = _perstep_shapes(natparam)
    lens, dev, leaves = _on_device(natparam, lengths)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_perstep_workspace_bytes, B, T, K, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    logZ = torch.empty(B, **f64)
    E_init, E_states = torch.empty(B, K, **f64), torch.empty(B, T, K, **f64)
    E_trans = torch.empty(B, T - 1, K, K, **f64) if want_trans else None
    _call("svae_hmm_perstep_estep_f64", dev, lens, check, B, T, K, int(pair_batched), *map(p, leaves), p(lens),
          p(logZ), p(E_init), p(E_trans), p(E_states), _info(lens, dev), p(ws), wsb)
    logZ, E_init, E_trans, E_states = _unbatch(batched, logZ, E_init, E_trans, E_states)
    return logZ, (E_init, E_trans, E_states)


def hmm_logZ_perstep(natparam, lengths=None):
    """The log-normaliser of hmm_estep_perstep alone (the per-step pair marginals are not formed)."""
    return hmm_estep_perstep(natparam, lengths=lengths, want_trans=False)[0]


class _HMMLogZPerstep(torch.autograd.Function):
    """log Z of HMMs with per-step transition potentials, differentiable w.r.t. all three natural parameters: the
    gradients are the expected statistics of the same launch (E_init, the per-step E_trans, E_states), summed over the
    batch where a parameter is shared."""

    @staticmethod
    def forward(ctx, init_params, pair_params, node_params, lengths):
        logZ, (E_init, E_trans, E_states) = hmm_estep_perstep((init_params, pair_params, node_params), lengths=lengths)
        ctx.save_for_backward(E_init, E_trans, E_states)
        ctx.pair_batched = pair_params.dim() == 4
        ctx.like = [(x.device, x.dtype) for x in (init_params, pair_params, node_params)]
        return logZ

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        E_init, E_trans, E_states = ctx.saved_tensors
        g = g.to(device=E_states.device, dtype=E_states.dtype)
        d_init, d_pair, d_node = g[..., None] * E_init, g[..., None, None, None] * E_trans, g[..., None, None] * E_states
        if E_states.dim() == 3:
            d_init = d_init.sum(0)                    # shared parameters receive the batch sum
            if not ctx.pair_batched:
                d_pair = d_pair.sum(0)
        need = ctx.needs_input_grad
        out = [d.to(device=dv, dtype=dt) if n else None for d, (dv, dt), n in zip((d_init, d_pair, d_node), ctx.like, need)]
        return out[0], out[1], out[2], None


def hmm_logZ_perstep_differentiable(natparam, lengths=None):
    """hmm_logZ_perstep with gradients flowing to init (K), pair (T-1,K,K) or (B,T-1,K,K) and node (T,K) or (B,T,K)
    (torch tensors): E_init, the per-step E_trans and E_states of the same launch, times the incoming cotangent, summed
    over the batch where the parameter is shared.  With lengths= they are exactly 0 from a sequence's length on (node
    steps >= L, pair steps >= L-1).  The training path of time-varying transitions; once differentiable."""
    init_params, pair_params, node_params = natparam
    for x in (init_params, pair_params, node_params):
        if not isinstance(x, torch.Tensor):
            raise TypeError("hmm_logZ_perstep_differentiable takes torch tensors")
    return _HMMLogZPerstep.apply(init_params, pair_params, node_params, lengths)


def hmm_estep_perstep_vjp(natparam, cotangents, workspace=None, lengths=None, check=False, want_pair=True):
    """The reverse-mode derivative of hmm_estep_perstep (svae_hmm_perstep_estep_vjp_f64, include/svae_hip.h): natparam as
    there; cotangents = (g_logZ, (g_init, g_trans, g_states)) in the shapes hmm_estep_perstep returns -- g_trans PER STEP,
    (…,T-1,K,K) --, each may be None (zero).  Returns the PER-SEQUENCE gradients (d_init (B,K), d_pair (B,T-1,K,K),
    d_node (B,T,K)) -- without the leading axis for unbatched (T,K) node potentials --; a shared init or pair parameter's
    gradient is their sum over the batch.  want_pair=False returns d_pair = None and skips the pass that forms it (the pair
    parameters need no gradient); d_init and d_node do not change a bit.  One route, log space throughout: nothing is
    flagged or redone.
    workspace: a contiguous float64 device tensor of at least svae_hmm_perstep_estep_vjp_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers -- the gradient of every sequence cut to its length; d_node[b, L:] and d_pair[b, L-1:] are
    exactly 0, and nothing of the potentials or cotangents from there on is read."""
    B, T, K, batched, pair_batched = _perstep_shapes(natparam)
    cots = _cotangents(cotangents, ((B,), (B, K), (B, T - 1, K, K), (B, T, K)), batched)
    lens, dev, leaves = _on_device(natparam, lengths)
    cots = [None if x is None else _dev64(x, dev) for x in cots]
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_perstep_estep_vjp_workspace_bytes, B, T, K, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    d_init, d_node = torch.empty(B, K, **f64), torch.empty(B, T, K, **f64)
    d_pair = torch.empty(B, T - 1, K, K, **f64) if want_pair else None
    _call("svae_hmm_perstep_estep_vjp_f64", dev, lens, check, B, T, K, int(pair_batched), *map(p, leaves), p(lens),
          *map(p, cots), p(d_init), p(d_pair), p(d_node), _info(lens, dev), p(ws), wsb)
    return _unbatch(batched, d_init, d_pair, d_node)


class _HMMEStepPerstep(torch.autograd.Function):
    """hmm_estep_perstep with its reverse-mode derivative: forward is hmm_estep_perstep unchanged, backward one call of
    svae_hmm_perstep_estep_vjp_f64 on the saved potentials (without d_pair when the pair parameters need no gradient)."""

    @staticmethod
    def forward(ctx, init_params, pair_params, node_params, lengths, check):
        logZ, (E_init, E_trans, E_states) = hmm_estep_perstep((init_params, pair_params, node_params), lengths=lengths,
                                                              check=check)
        ctx.save_for_backward(init_params, pair_params, node_params)
        ctx.lengths = lengths
        return logZ, E_init, E_trans, E_states

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logZ, g_init, g_trans, g_states):
        init_params, pair_params, node_params = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_init, d_pair, d_node = hmm_estep_perstep_vjp((init_params, pair_params, node_params),
                                                       (g_logZ, (g_init, g_trans, g_states)), lengths=ctx.lengths,
                                                       want_pair=need[1])
        if node_params.dim() == 3:
            d_init = d_init.sum(0)                    # shared parameters receive the batch sum
            if need[1] and pair_params.dim() == 3:
                d_pair = d_pair.sum(0)
        like = lambda d, x: d.to(device=x.device, dtype=x.dtype)          # noqa: E731
        return (like(d_init, init_params) if need[0] else None, like(d_pair, pair_params) if need[1] else None,
                like(d_node, node_params) if need[2] else None, None, None)


def hmm_estep_perstep_differentiable(natparam, lengths=None, check=False):
    """hmm_estep_perstep -> (logZ, (E_init, E_trans, E_states)) with gradients of all four outputs flowing to whichever of
    init (K), pair (T-1,K,K) or (B,T-1,K,K) and node (T,K) or (B,T,K) require them (torch tensors on the device).  The
    outputs are those of hmm_estep_perstep, bit for bit; the backward pass is one call of svae_hmm_perstep_estep_vjp_f64
    (once differentiable): a shared init or pair parameter receives the sum over the batch, a per-sequence pair parameter
    its own block; pair parameters that need no gradient (a recognition network that emits node potentials only) skip the
    pass that forms it.  With lengths= the gradient is that of every sequence cut to its length: exactly 0 from there on."""
    init_params, pair_params, node_params = natparam
    for x in (init_params, pair_params, node_params):
        if not isinstance(x, torch.Tensor):
            raise TypeError("hmm_estep_perstep_differentiable takes torch tensors")
    logZ, E_init, E_trans, E_states = _HMMEStepPerstep.apply(init_params, pair_params, node_params, lengths, check)
    return logZ, (E_init, E_trans, E_states)


def hmm_viterbi_perstep(natparam, workspace=None, return_score=False, lengths=None, check=False):
    """hmm_viterbi for the natparam hmm_estep_perstep takes -- init (K), pair (T-1,K,K) or (B,T-1,K,K), node (T,K) or
    (B,T,K), LOG potentials, finite or -inf: labels torch.int32 (T,) or (B,T); with return_score also the path's score
    (0-d, or (B)).  The arithmetic is hmm_viterbi's with the step's own matrix (include/svae_hip.h,
    svae_hmm_perstep_viterbi_f64): labels and score are reproducible bit for bit, ties to the lowest index.
    workspace: any contiguous device tensor of at least svae_hmm_viterbi_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers, see the module docstring -- labels from a sequence's length on are -1, and neither node[b, L:]
    nor pair[b, L-1:] is read."""
    B, T, K, batched, pair_batched = _perstep_shapes(natparam)
    lens, dev, leaves = _on_device(natparam, lengths)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_viterbi_workspace_bytes, B, T, K, dev)
    states = torch.empty(B, T, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev) if return_score else None
    _call("svae_hmm_perstep_viterbi_f64", dev, lens, check, B, T, K, int(pair_batched), *map(p, leaves), p(lens),
          p(states), p(score), _info(lens, dev), p(ws), wsb)
    states, score = _unbatch(batched, states, score)
    return (states, score) if return_score else states


def hmm_sample_perstep(natparam, num_samples=1, u=None, generator=None, workspace=None, return_logZ=False, lengths=None,
                       check=False):
    """hmm_sample for the natparam hmm_estep_perstep takes: state paths drawn from the posterior by forward filtering and
    backward sampling, labels torch.int32 (S,T) or (B,S,T), S = num_samples; with return_logZ also the log-normaliser the
    filter computes (0-d, or (B)) -- bit for bit hmm_logZ_perstep's: the filter is the E-step's forward sweep.  One route,
    log space throughout (include/svae_hip.h, svae_hmm_perstep_sample_f64): nothing is flagged or redone; a state with a
    forbidden (-inf) transition or observation is never drawn.
    u: the uniforms, (B,S,T) ((S,T) for the unbatched call); None draws torch.rand fp64 on the device with `generator`.
    workspace: a contiguous device tensor of at least svae_hmm_perstep_workspace_bytes(B,T,K) bytes.
    lengths: (B,) integers, see the module docstring -- labels from a sequence's length on are -1, and none of node[b, L:],
    pair[b, L-1:] and u[b, :, L:] is read."""
    B, T, K, batched, pair_batched = _perstep_shapes(natparam)
    S = _sample_shapes(num_samples, u, B, T, batched)
    lens, dev, leaves = _on_device(natparam, lengths)
    u = _uniforms(u, generator, B, S, T, dev)
    lib, p = _lib.load(), _lib.ptr
    ws, wsb = _workspace(workspace, lib.svae_hmm_perstep_workspace_bytes, B, T, K, dev)
    states = torch.empty(B, S, T, dtype=torch.int32, device=dev)
    logZ = torch.empty(B, dtype=torch.float64, device=dev) if return_logZ else None
    _call("svae_hmm_perstep_sample_f64", dev, lens, check, B, T, K, S, int(pair_batched), *map(p, leaves), p(lens),
          p(u), p(states), p(logZ), _info(lens, dev), p(ws), wsb)
    states, logZ = _unbatch(batched, states, logZ)
    return (states, logZ) if return_logZ else states
