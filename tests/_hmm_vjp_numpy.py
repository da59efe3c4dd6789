"""NumPy restatement, in log space, of the reverse-mode derivative of the HMM E-step (svae_hmm_estep_vjp_f64,
include/svae_hip.h; the arithmetic is stated in svae_amd/csrc/hmm_estep_vjp.hip), independent of the kernels' scaling.

The statistics (E_init, E_trans, E_states) are the gradient of log Z, so their Jacobian is the Hessian of log Z: the
posterior covariance of the sufficient statistics.  For cotangents g (of logZ), u0 (of E_init), V (of E_trans) and W (of
E_states) put  phi(z) = u0[z_0] + sum_t V[z_t, z_{t+1}] + sum_t W[t, z_t];  then

    g_node[t,k] = gamma_t[k] (g + E[phi | z_t = k] - E[phi]),     g_init = g_node[0],
    g_pair[i,j] = sum_t xi_t[i,j] (g + E[phi | z_t = i, z_{t+1} = j] - E[phi]).

Every weight is a softmax of log quantities; a state without incoming mass has r = W[t, j], one without outgoing mass
s = 0 (both are multiplied by a marginal of exactly 0)."""
import numpy as np

NEG = -np.inf


def _lse(x, axis):
    """log-sum-exp that returns -inf (not NaN) where every term is -inf; also the softmax weights (0 there)"""
    m = np.max(x, axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(x - ms)
    s = e.sum(axis=axis, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.squeeze(ms + np.log(s), axis=axis)
        w = np.where(s > 0, e / np.where(s > 0, s, 1.0), 0.0)
    return out, w


def estep_vjp(init, pair, node, g=0.0, u0=None, V=None, W=None):
    """One sequence: init (K), pair (K,K), node (T,K) log-potentials (entries may be -inf); cotangents g (scalar),
    u0 (K), V (K,K), W (T,K), None = 0.  -> (g_init (K), g_pair (K,K), g_node (T,K))."""
    init, pair, node = (np.asarray(x, float) for x in (init, pair, node))
    T, K = node.shape
    u0 = np.zeros(K) if u0 is None else np.asarray(u0, float)
    V = np.zeros((K, K)) if V is None else np.asarray(V, float)
    W = np.zeros((T, K)) if W is None else np.asarray(W, float)
    with np.errstate(all="ignore"):
        la = np.empty((T, K))               # log a_t, normalised
        r = np.empty((T, K))
        x = init + node[0]
        la[0] = x - _lse(x, 0)[0]
        r[0] = u0 + W[0]
        for t in range(1, T):
            lp, w = _lse(la[t - 1][:, None] + pair, 0)              # w[i, j]: softmax over i
            r[t] = (w * (r[t - 1][:, None] + V)).sum(0) + W[t]
            x = lp + node[t]
            la[t] = x - _lse(x, 0)[0]
        a_last = np.exp(la[T - 1])
        a_last /= a_last.sum()
        Ephi = float(a_last @ r[T - 1])
        g_node = np.zeros((T, K))
        g_pair = np.zeros((K, K))
        lb = np.zeros(K)
        s = np.zeros(K)
        g_node[T - 1] = a_last * (g + r[T - 1] - Ephi)
        for t in range(T - 2, -1, -1):
            lu = node[t + 1] + lb                                   # log (e o b)_{t+1}
            x = pair + lu[None, :]
            lbr, q = _lse(x, 1)                                     # q[i, j]: softmax over j
            yv = W[t + 1] + s
            s_new = (q * (V + yv[None, :])).sum(1)
            lg = la[t] + lbr
            lZ, gam = _lse(lg, 0)
            xi = np.exp(la[t][:, None] + x - lZ)
            xi = np.where(np.isfinite(la[t][:, None] + x), xi, 0.0)
            g_pair += xi * (g - Ephi + r[t][:, None] + V + yv[None, :])
            lb = lbr - lZ
            s = s_new
            g_node[t] = gam * (g + r[t] + s - Ephi)
    return g_node[0].copy(), g_pair, g_node


def estep_vjp_batch(init, pair, node, lengths=None, g=None, u0=None, V=None, W=None):
    """A batch, sequence by sequence (each cut to its length): init (K), pair (K,K) or (B,K,K), node (B,T,K); cotangents
    g (B), u0 (B,K), V (B,K,K), W (B,T,K) or None.  -> per-sequence g_init (B,K), g_pair (B,K,K), g_node (B,T,K) with
    g_node[b, L:] = 0."""
    node = np.asarray(node, float)
    B, T, K = node.shape
    pair = np.asarray(pair, float)
    gi, gp, gn = np.zeros((B, K)), np.zeros((B, K, K)), np.zeros((B, T, K))
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        gi[b], gp[b], gn[b, :L] = estep_vjp(init, pair[b] if pair.ndim == 3 else pair, node[b, :L],
                                            0.0 if g is None else float(g[b]),
                                            None if u0 is None else u0[b], None if V is None else V[b],
                                            None if W is None else W[b, :L])
    return gi, gp, gn


def scale(g, u0, V, W, L):
    """|g| + L max|cotangent|: the size of phi, to which the tolerances of the tests are relative"""
    mx = max([0.0] + [float(np.max(np.abs(x))) for x in (u0, V, W) if x is not None and np.size(x)])
    return abs(0.0 if g is None else float(g)) + L * mx
