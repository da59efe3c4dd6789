"""Drop-in for the reference's compiled LDS module (svae/lds/cython_lds_inference.pyx): the six names that
svae/lds/lds_inference.py:18-24 imports, with the reference's `(result, intermediates)` conventions, plus torch autograd
wrappers of the three reverse-mode primitives.

Forward values come from the functions of lds_inference.py, called as they are.  The `*_grad` functions run the HIP
kernels of svae_amd/csrc/lds_prim_vjp.hpp (svae_lds_filter_vjp_f64, svae_lds_smoother_vjp_f64,
svae_lds_sample_vjp_f64), which rebuild every per-step factor from the forward messages: `intermediates` only holds
tensors the caller already has.  Scaling and layouts are the reference's (natural parameters, J = -1/2 precision); an
optional leading batch axis B is accepted everywhere.  Host ndarray inputs give ndarray outputs, device tensors give
tensors on the same device.  No function writes into its arguments.  Latent dimension n <= 15 (_lib.LDS_MAX_N); the
sampler's gradient takes num_samples <= 16.  Like the reference (which ignores LAPACK `info`), a pivot that is not
positive definite is not reported: the gradients are then NaN.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from . import lds_inference as _li

__all__ = ["natural_filter_forward_general", "natural_filter_grad", "natural_smoother_general",
           "natural_smoother_general_grad", "natural_sample_backward", "natural_sample_backward_grad",
           "filter_forward_differentiable", "smoother_differentiable", "sample_backward_differentiable"]

_f64 = torch.float64


def _is_host(x):
    return not (isinstance(x, torch.Tensor) and x.is_cuda)


def _dev(x, device):
    if isinstance(x, torch.Tensor):         # no copy when it already fits: the kernels only read their inputs
        return x.detach().to(device=device, dtype=_f64).contiguous()
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(device).contiguous()


def _out(x, host):
    if isinstance(x, (tuple, list)):
        return type(x)(_out(y, host) for y in x)
    if host and isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return x


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _check_n(n):
    if n < 1 or n > _lib.LDS_MAX_N:
        raise ValueError("latent dimension n = %d: the reverse-mode primitives take 1 <= n <= %d" % (n, _lib.LDS_MAX_N))


def _pairs(pair_params, B, T, n, device):
    """(J11, J12, J22) device tensors + (inhomog, pair_batched), shapes checked as in lds_inference._prepare."""
    J11, J12, J22 = (_dev(x, device) for x in pair_params[:3])
    want = {2: (n, n), 3: (T - 1, n, n), 4: (B, T - 1, n, n)}.get(J11.dim())
    if want is None or any(tuple(x.shape) != want for x in (J11, J12, J22)):
        raise ValueError("pair_params must be (n,n), (T-1,n,n) or (B,T-1,n,n) for n = %d, T = %d" % (n, T))
    return (J11, J12, J22), J11.dim() >= 3, J11.dim() == 4


def _messages(forward_messages, device):
    (Jp, hp), (Jf, hf) = forward_messages
    Jp, hp, Jf, hf = (_dev(x, device) for x in (Jp, hp, Jf, hf))
    batched = hf.dim() == 3
    if not batched:
        Jp, hp, Jf, hf = Jp[None], hp[None], Jf[None], hf[None]
    if Jp.dim() != 4 or Jp.shape != Jf.shape or hp.shape != hf.shape or Jp.shape[:3] != hp.shape \
            or Jp.shape[-1] != Jp.shape[-2]:
        raise ValueError("forward_messages = ((J_pred, h_pred), (J_filt, h_filt)) with J (T,n,n) and h (T,n) "
                         "[or a leading B axis]")
    _check_n(hf.shape[-1])
    return (Jp, hp, Jf, hf), batched


def _like(x, shape, device):
    """a cotangent as a fresh contiguous device tensor of `shape` (None -> zeros)"""
    if x is None:
        return torch.zeros(shape, dtype=_f64, device=device)
    t = _dev(x, device)
    if tuple(t.shape) != tuple(shape):
        t = t.reshape(shape)
    return t


def _stream(device):
    return _lib.current_stream(device)


class _Inter(object):
    """the `intermediates` of this module: device tensors the caller already holds, and the layout flags"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ----------------------------------------------------------------------------------------------------------------- filter
def natural_filter_forward_general(init_params, pair_params, node_params):
    """cython_lds_inference.pyx:28-90 -> ((((J_pred, h_pred), (J_filt, h_filt)), lognorm), intermediates)."""
    host = _is_host(node_params[1])
    h = node_params[1]
    n = int(np.shape(h)[-1])
    _check_n(n)
    (msgs, lognorm) = _li.natural_filter_forward_general(init_params, pair_params, node_params)
    (Jp, hp), (Jf, hf) = msgs
    batched = hf.dim() == 3
    dev = hf.device
    B, T = (hf.shape[0], hf.shape[1]) if batched else (1, hf.shape[0])
    pairs, inhomog, pair_batched = _pairs(pair_params, B, T, n, dev)
    inter = _Inter(kind="filter", pairs=pairs, inhomog=inhomog, pair_batched=pair_batched,
                   Jf=(Jf if batched else Jf[None]).contiguous(), hf=(hf if batched else hf[None]).contiguous(),
                   B=B, T=T, n=n, batched=batched, host=host)
    return _out((((Jp, hp), (Jf, hf)), lognorm), host), inter


def natural_filter_grad(g, intermediates):
    """cython_lds_inference.pyx:92-145 -> (g_J_node (T,n), g_h_node (T,n), g_logZ_node (T,)) [(B,...) batched]."""
    it = intermediates
    ((gJp, ghp), (gJf, ghf)), glog = g
    dev, B, T, n = it.Jf.device, it.B, it.T, it.n
    gJp, gJf = (_like(x, (B, T, n, n), dev) for x in (gJp, gJf))
    ghp, ghf = (_like(x, (B, T, n), dev) for x in (ghp, ghf))
    glog = _like(glog, (B,), dev)
    gJn = torch.empty(B, T, n, dtype=_f64, device=dev)
    ghn = torch.empty(B, T, n, dtype=_f64, device=dev)
    gzn = torch.empty(B, T, dtype=_f64, device=dev)
    J11, J12, _ = it.pairs
    p = _lib.ptr
    rc = _lib.load().svae_lds_filter_vjp_f64(B, T, n, int(it.inhomog), int(it.pair_batched), p(J11), p(J12),
                                              p(it.Jf), p(it.hf), p(gJp), p(ghp), p(gJf), p(ghf), p(glog),
                                              p(gJn), p(ghn), p(gzn), None, _stream(dev))
    _lib.check(rc, "svae_lds_filter_vjp_f64")
    out = (gJn, ghn, gzn) if it.batched else (gJn[0], ghn[0], gzn[0])
    return _out(out, it.host)


# --------------------------------------------------------------------------------------------------------------- smoother
def natural_smoother_general(forward_messages, pair_params):
    """cython_lds_inference.pyx:149-210 -> ((E_init, E_pair, E_node), intermediates)."""
    host = _is_host(forward_messages[1][1])
    dev = _device_of(forward_messages[1][1], forward_messages[0][0])
    (Jp, hp, Jf, hf), batched = _messages(forward_messages, dev)
    B, T, n = hf.shape
    pairs, inhomog, pair_batched = _pairs(pair_params, B, T, n, dev)
    msgs = ((Jp, hp), (Jf, hf)) if batched else ((Jp[0], hp[0]), (Jf[0], hf[0]))
    stats = _li.natural_smoother_general(msgs, pair_params)
    inter = _Inter(kind="smoother", pairs=pairs, inhomog=inhomog, pair_batched=pair_batched,
                   msgs=(Jp, hp, Jf, hf), B=B, T=T, n=n, batched=batched, host=host)
    return _out(stats, host), inter


def _message_grads(it, gJp, ghp, gJf, ghf):
    out = ((gJp, ghp), (gJf, ghf))
    if not it.batched:
        out = ((gJp[0], ghp[0]), (gJf[0], ghf[0]))
    return _out(out, it.host)


def natural_smoother_general_grad(g, intermediates):
    """cython_lds_inference.pyx:236-306 -> ((g_J_pred, g_h_pred), (g_J_filt, g_h_filt)).  The scalar "ones" entries of
    g are accepted and ignored; any statistic's cotangent may be None (zero)."""
    it = intermediates
    dev, B, T, n = it.msgs[0].device, it.B, it.T, it.n
    g_init, g_pair, g_node = g
    gi = None
    if g_init is not None and (g_init[0] is not None or g_init[1] is not None):
        gi = torch.cat([_like(g_init[0], (B, n * n), dev), _like(g_init[1], (B, n), dev)], dim=1).contiguous()
    gp = None
    if T > 1 and g_pair is not None and any(x is not None for x in g_pair[:3]):
        shp = (B, T - 1, n, n) if it.inhomog else (B, n, n)
        gp = torch.stack([_like(x, shp, dev) for x in g_pair[:3]], dim=-3).contiguous()
    gdxx = _like(g_node[0], (B, T, n), dev) if g_node is not None and g_node[0] is not None else None
    gx = _like(g_node[1], (B, T, n), dev) if g_node is not None and g_node[1] is not None else None
    gJp, gJf = (torch.empty(B, T, n, n, dtype=_f64, device=dev) for _ in range(2))
    ghp, ghf = (torch.empty(B, T, n, dtype=_f64, device=dev) for _ in range(2))
    lib = _lib.load()
    nbytes = lib.svae_lds_smoother_vjp_workspace_bytes(B, T, n)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    J11, J12, J22 = it.pairs
    Jp, hp, Jf, hf = it.msgs
    p = _lib.ptr
    rc = lib.svae_lds_smoother_vjp_f64(B, T, n, int(it.inhomog), int(it.pair_batched), p(J11), p(J12), p(J22),
                                       p(Jp), p(hp), p(Jf), p(hf), p(gi), p(gp), p(gdxx), p(gx),
                                       p(gJp), p(ghp), p(gJf), p(ghf), None,
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream(dev))
    _lib.check(rc, "svae_lds_smoother_vjp_f64")
    return _message_grads(it, gJp, ghp, gJf, ghf)


# ---------------------------------------------------------------------------------------------------------------- sampler
def natural_sample_backward(forward_messages, pair_params, num_samples, eps=None):
    """cython_lds_inference.pyx:310-355 -> (samples (T,S,n) [(B,T,S,n)], intermediates).  eps (T,S,n) [(B,T,S,n)]
    with eps[t] the noise applied at step t; drawn here (torch.randn) when None."""
    host = _is_host(forward_messages[1][1])
    dev = _device_of(forward_messages[1][1], forward_messages[0][0])
    (Jp, hp, Jf, hf), batched = _messages(forward_messages, dev)
    B, T, n = hf.shape
    S = int(num_samples)
    pairs, inhomog, pair_batched = _pairs(pair_params, B, T, n, dev)
    if eps is None:
        eps = torch.randn(B, T, S, n, dtype=_f64, device=dev)
    else:
        eps = _dev(eps, dev)
        if not batched:
            eps = eps[None]
        if tuple(eps.shape) != (B, T, S, n):
            raise ValueError("eps must be (T,S,n) [(B,T,S,n)]")
    msgs = ((Jp, hp), (Jf, hf)) if batched else ((Jp[0], hp[0]), (Jf[0], hf[0]))
    samples = _li.natural_sample_backward(msgs, pair_params, S, eps=eps if batched else eps[0])
    sb = (samples if batched else samples[None]).contiguous()
    inter = _Inter(kind="sampler", pairs=pairs, inhomog=inhomog, pair_batched=pair_batched,
                   msgs=(Jp, hp, Jf, hf), eps=eps, samples=sb, S=S, B=B, T=T, n=n, batched=batched, host=host)
    return _out(samples, host), inter


def natural_sample_backward_grad(g_samples, intermediates):
    """cython_lds_inference.pyx:357-409 -> ((g_J_pred, g_h_pred), (g_J_filt, g_h_filt)); the prediction parts are zero."""
    it = intermediates
    dev, B, T, n, S = it.msgs[0].device, it.B, it.T, it.n, it.S
    if S > 16:
        raise ValueError("natural_sample_backward_grad: num_samples <= 16 (svae_lds_sample_vjp_f64); got %d" % S)
    gs = _like(g_samples, (B, T, S, n), dev)
    gJp, gJf = (torch.empty(B, T, n, n, dtype=_f64, device=dev) for _ in range(2))
    ghp, ghf = (torch.empty(B, T, n, dtype=_f64, device=dev) for _ in range(2))
    J11, J12, _ = it.pairs
    p = _lib.ptr
    rc = _lib.load().svae_lds_sample_vjp_f64(B, T, n, S, int(it.inhomog), int(it.pair_batched), p(J11), p(J12),
                                             p(it.msgs[2]), p(it.msgs[3]), p(it.eps), p(it.samples), p(gs),
                                             p(gJp), p(ghp), p(gJf), p(ghf), None, _stream(dev))
    _lib.check(rc, "svae_lds_sample_vjp_f64")
    return _message_grads(it, gJp, ghp, gJf, ghf)


# ---------------------------------------------------------------------------------------------------------- torch autograd
class _Filter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, node_J, node_h, node_logZ, init_params, pair_params):
        nodes = (node_J.detach(), node_h.detach()) + ((node_logZ.detach(),) if node_logZ is not None else ())
        (((Jp, hp), (Jf, hf)), lognorm), inter = natural_filter_forward_general(init_params, pair_params, nodes)
        ctx.inter = inter
        ctx.has_logZ = node_logZ is not None
        return Jp, hp, Jf, hf, lognorm.clone()

    @staticmethod
    def backward(ctx, gJp, ghp, gJf, ghf, glog):
        gJ, gh, gz = natural_filter_grad(((((gJp, ghp), (gJf, ghf)), glog)), ctx.inter)
        return gJ, gh, (gz if ctx.has_logZ else None), None, None


class _Smoother(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Jp, hp, Jf, hf, pair_params):
        (Ei, Ep, En), inter = natural_smoother_general(((Jp.detach(), hp.detach()), (Jf.detach(), hf.detach())),
                                                       pair_params)
        ctx.inter = inter
        ctx.set_materialize_grads(False)
        return Ei[0].clone(), Ei[1].clone(), Ep[0].clone(), Ep[1].clone(), Ep[2].clone(), En[0].clone(), En[1].clone()

    @staticmethod
    def backward(ctx, gxx0, gx0, gp0, gp1, gp2, gdxx, gx):
        (gJp, ghp), (gJf, ghf) = natural_smoother_general_grad(
            ((gxx0, gx0), (gp0, gp1, gp2, None), (gdxx, gx, None)), ctx.inter)
        return gJp, ghp, gJf, ghf, None


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Jp, hp, Jf, hf, pair_params, num_samples, eps):
        samples, inter = natural_sample_backward(((Jp.detach(), hp.detach()), (Jf.detach(), hf.detach())),
                                                 pair_params, num_samples, eps=eps)
        ctx.inter = inter
        return samples.clone()

    @staticmethod
    def backward(ctx, gs):
        (gJp, ghp), (gJf, ghf) = natural_sample_backward_grad(gs, ctx.inter)
        return gJp, ghp, gJf, ghf, None, None, None


def filter_forward_differentiable(init_params, pair_params, node_params):
    """((J_pred, h_pred), (J_filt, h_filt)), lognorm -- differentiable w.r.t. the node potentials (J, h[, logZ]) (device
    tensors; diagonal J (T,n) / (B,T,n)); backward is natural_filter_grad."""
    node_logZ = node_params[2] if len(node_params) == 3 else None
    Jp, hp, Jf, hf, lognorm = _Filter.apply(node_params[0], node_params[1], node_logZ, init_params, pair_params)
    return ((Jp, hp), (Jf, hf)), lognorm


def smoother_differentiable(forward_messages, pair_params):
    """(E_init, E_pair, E_node) as natural_smoother_general, differentiable w.r.t. the four messages (backward:
    natural_smoother_general_grad).  The scalar "ones" entries are plain constants."""
    (Jp, hp), (Jf, hf) = forward_messages
    xx0, x0, p0, p1, p2, dxx, x = _Smoother.apply(Jp, hp, Jf, hf, pair_params)
    lead = x0.shape[:-1]
    one = lambda *s: torch.ones(lead + s, dtype=_f64, device=x.device)
    T = x.shape[-2]
    ones_pair = one(T - 1) if p0.dim() == x.dim() + 1 else one()
    return (xx0, x0, one(), one()), (p0, p1, p2, ones_pair), (dxx, x, one(T))


def sample_backward_differentiable(forward_messages, pair_params, num_samples, eps=None):
    """samples as natural_sample_backward, differentiable w.r.t. the messages (backward: natural_sample_backward_grad)."""
    (Jp, hp), (Jf, hf) = forward_messages
    return _Sample.apply(Jp, hp, Jf, hf, pair_params, num_samples, eps)
