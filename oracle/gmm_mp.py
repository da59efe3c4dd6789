"""TEST INFRASTRUCTURE: the GMM local step in 50 digits (mpmath) -- the arbiter of the mean-field kernels
(csrc/gmm_meanfield.hip, csrc/gmm_wide.hip), the per-point sampler and the derived adjoint (csrc/gmm_train.hip).  Only
tests/ and tools/ import this (oracle/lds_mp.py and oracle/expfam_mp.py are the precedents; the linear algebra is lds_mp's).

The operation is oracle/gmm_numpy.py's, statement by statement:

  local_meanfield_mp     svae/models/gmm.py:62-88 with :90-110 inside (label_init an argument, as in gmm_numpy)
  sample_mp              svae/distributions/gaussian.py:27-33  x = J^-1 h + chol(J)^-T eps
  local_tail_jvp_mp      the directional derivative of (samples, local_kl) of the ONE pass the reference keeps on the
                         autograd tape (gmm.py:74-86 + the sampler; tests/_gmm_torch.py states it in torch)

Every function takes float64 inputs exactly.  Per point: Cholesky, inverse and mean in `dps` digits, the log-normaliser
as a SUM of logs of the Cholesky diagonal (never a determinant product), the softmax with the maximum subtracted.  With
tol = 0.0 the stopping test |kl - kl_prev| < tol is never true, so the result is max_iter sweeps + the final pass: a
smooth map of the inputs.  Results are float64 (as_float=True) or object arrays / scalars of mpf."""
import numpy as np

from .lds_mp import _chol, _digits, _f64, _lsolve, _ltsolve, _mpa

DPS = 50

KEYS = ("label_stats", "label_fixed", "label_natparam", "gaussian_stats", "gaussian_natparam", "dirichlet_stats",
        "niw_stats", "kl", "iters", "kl_hist", "kl_scale")


def _zeros(shape):
    import mpmath as mp
    z = np.zeros(shape, dtype=object)
    z[...] = mp.mpf(0)
    return z


def _eye(n):
    import mpmath as mp
    I = _zeros((n, n))
    for i in range(n):
        I[i, i] = mp.mpf(1)
    return I


def _dot(a, b):
    import mpmath as mp
    return sum((x * y for x, y in zip(a.reshape(-1), b.reshape(-1))), mp.mpf(0))


def _gauss_point(eta):
    """one dense-packed (N+2, N+2) natural parameter -> (expected statistics dense-packed, log Z, the absolute values of
    log Z's terms summed): gaussian.py:11-25"""
    import mpmath as mp
    N = eta.shape[0] - 2
    J, h = -2 * eta[:N, :N], eta[:N, N]
    L = _chol((J + J.T) / 2)
    Sigma = _ltsolve(L, _lsolve(L, _eye(N)))
    Sigma = (Sigma + Sigma.T) / 2
    Ex = _ltsolve(L, _lsolve(L, h))
    stats = _zeros(eta.shape)
    stats[:N, :N], stats[:N, N] = Sigma + np.outer(Ex, Ex), Ex
    stats[N, N] = stats[N + 1, N + 1] = mp.mpf(1)
    quad, logdiag = np.dot(h, Ex) / 2, sum(mp.log(L[i, i]) for i in range(N))
    logZ = quad - logdiag + eta[N, N] + eta[N + 1, N + 1]
    return stats, logZ, abs(quad) + abs(logdiag) + abs(eta[N, N]) + abs(eta[N + 1, N + 1])


def _softmax(x):
    """-> (softmax, logsumexp) of one row, the maximum subtracted"""
    import mpmath as mp
    mx = max(x)
    e = np.array([mp.exp(v - mx) for v in x], dtype=object)
    se = sum(e)
    return e / se, mx + mp.log(se)


def _pass(lg, gg, node, r):
    """gaussian_meanfield + label_meanfield (gmm.py:112-124) from the responsibilities r (T, K).  -> per-point arrays
    and the three per-batch KL pieces: the KL of gmm.py:82-86, the linear-correction term of gmm.py:99-102 (new
    responsibilities against the ones eta was built from) and the absolute values of the KL's terms summed."""
    import mpmath as mp
    T, K = r.shape
    D = gg.shape[-1]
    N = D - 2
    gflat = gg.reshape(K, D * D)
    gn, gs, ln, ls = _zeros((T, D, D)), _zeros((T, D, D)), _zeros((T, K)), _zeros((T, K))
    kl, lin, scale = mp.mpf(0), mp.mpf(0), mp.mpf(0)
    for t in range(T):
        eta = node[t] + np.dot(r[t], gflat).reshape(D, D)
        stats, logZ, zscale = _gauss_point(eta)
        nodedot = [node[t][i, i] * stats[i, i] for i in range(N)] + [node[t][i, N] * stats[i, N] for i in range(N)]
        sflat = stats.reshape(-1)
        l = np.array([_dot(sflat, gflat[k]) for k in range(K)], dtype=object)
        natparam = l + lg
        rnew, lse = _softmax(natparam)
        lab = [rnew[k] * l[k] for k in range(K)]
        kl += sum(nodedot) - logZ + sum(lab) - lse
        lin += sum((r[t][k] - rnew[k]) * l[k] for k in range(K))
        scale += sum(abs(v) for v in nodedot) + zscale + sum(abs(v) for v in lab) + abs(lse)
        gn[t], gs[t], ln[t], ls[t] = eta, stats, natparam, rnew
    return gn, gs, ln, ls, kl, lin, scale


def _pack_node(node_J, node_h):
    nJ, nh = _mpa(node_J), _mpa(node_h)
    T, N = nh.shape
    node = _zeros((T, N + 2, N + 2))
    for i in range(N):
        node[:, i, i], node[:, i, N] = nJ[:, i], nh[:, i]
    return node


def local_meanfield_mp(label_global, gaussian_globals, node_potentials, label_init, tol=1e-3, max_iter=100,
                       dps=DPS, as_float=True):
    """oracle/gmm_numpy.local_meanfield in `dps` digits.  node_potentials = (J diag (T, N), h (T, N)).  -> dict:
    label_stats, label_fixed (the responsibilities entering the final pass), label_natparam, gaussian_stats,
    gaussian_natparam, dirichlet_stats, niw_stats, kl, iters, kl_hist (the batch-total KL after every sweep, with the
    linear-correction term of gmm.py:99-105) and kl_scale (the absolute values of the terms of `kl` summed: what it
    cancels from)."""
    import mpmath as mp
    with _digits(dps):
        lg, gg = _mpa(label_global), _mpa(gaussian_globals)
        node = _pack_node(*node_potentials)
        r = _mpa(label_init)
        prev, hist, iters = mp.inf, [], 0
        for i in range(int(max_iter)):
            iters = i + 1
            _, _, _, rnew, kl, lin, _ = _pass(lg, gg, node, r)
            r = rnew
            hist.append(kl + lin)
            stop = abs(hist[-1] - prev) < mp.mpf(float(tol))
            prev = hist[-1]
            if stop:
                break
        gn, gs, ln, ls, kl, _, scale = _pass(lg, gg, node, r)
        K, D = ls.shape[1], gs.shape[-1]
        out = dict(label_stats=ls, label_fixed=r, label_natparam=ln, gaussian_stats=gs, gaussian_natparam=gn,
                   dirichlet_stats=ls.sum(0) if ls.shape[0] else _zeros((K,)),
                   niw_stats=np.dot(ls.T, gs.reshape(gs.shape[0], D * D)).reshape(K, D, D),
                   kl=kl, iters=iters, kl_hist=np.array(hist, dtype=object), kl_scale=scale)
        if as_float:
            out = {k: (v if k == "iters" else float(v) if k in ("kl", "kl_scale") else _f64(v)) for k, v in out.items()}
        return out


def _sample(gn, eps):
    T, S, N = eps.shape
    out = _zeros((T, S, N))
    for t in range(T):
        J = -2 * gn[t][:N, :N]
        L = _chol((J + J.T) / 2)
        mean = _ltsolve(L, _lsolve(L, gn[t][:N, N]))
        out[t] = (_ltsolve(L, eps[t].T)).T + mean
    return out


def sample_mp(gaussian_natparam, eps, dps=DPS, as_float=True):
    """gaussian.py:27-33 per point: dense-packed natural parameters (T, N+2, N+2), eps (T, S, N) -> samples (T, S, N)"""
    with _digits(dps):
        out = _sample(_mpa(gaussian_natparam), _mpa(eps))
        return _f64(out) if as_float else out


def local_tail_mp(label_global, gaussian_globals, node_potentials, label_fixed, eps, dps=DPS, as_float=True):
    """the taped function: (samples (T, S, N), local_kl) of the one pass from `label_fixed` (tests/_gmm_torch.py)"""
    with _digits(dps):
        gn, _, _, _, kl, _, _ = _pass(_mpa(label_global), _mpa(gaussian_globals), _pack_node(*node_potentials),
                                      _mpa(label_fixed))
        x = _sample(gn, _mpa(eps))
        return (_f64(x), float(kl)) if as_float else (x, kl)


def local_tail_jvp_mp(label_global, gaussian_globals, node_potentials, label_fixed, eps, direction, dps=60, step=1e-20):
    """d/ds (samples, local_kl)(node_J + s dJ, node_h + s dh) at s = 0, direction = (dJ, dh): a central difference inside
    mp (oracle/lds_mp.jvp_mp's scheme: truncation O(step^2) relative, log10(1/step) of the `dps` digits lost).  The
    responsibilities entering the pass are constants; the label update of the pass itself is differentiated, as on the
    reference's tape.  -> (d samples (T, S, N) float64, d kl float)"""
    import mpmath as mp
    with _digits(dps):
        s = mp.mpf(step)
        nJ, nh, dJ, dh = (_mpa(x) for x in tuple(node_potentials) + tuple(direction))
        up = local_tail_mp(label_global, gaussian_globals, (nJ + s * dJ, nh + s * dh), label_fixed, eps, dps, False)
        dn = local_tail_mp(label_global, gaussian_globals, (nJ - s * dJ, nh - s * dh), label_fixed, eps, dps, False)
        return _f64((up[0] - dn[0]) / (2 * s)), float((up[1] - dn[1]) / (2 * s))
