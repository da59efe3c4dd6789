"""NumPy restatement, in log space, of the reverse-mode derivative of the HMM E-step with PER-STEP transition potentials
(svae_hmm_perstep_estep_vjp_f64, include/svae_hip.h; the arithmetic is stated in svae_amd/csrc/hmm_estep_perstep_vjp.hip).
TEST INFRASTRUCTURE.

The statistics (E_init, the per-step E_trans, E_states) are the gradient of log Z, so their Jacobian is the Hessian of
log Z: the posterior covariance of the sufficient statistics.  For cotangents g (of logZ), u0 (of E_init), V_t (of
E_trans[t]) and W (of E_states) put  phi(z) = u0[z_0] + sum_t V_t[z_t, z_{t+1}] + sum_t W[t, z_t];  then

    d_node[t,k]   = gamma_t[k] (g + E[phi | z_t = k] - E[phi]),     d_init = d_node[0],
    d_pair[t,j,k] = xi_t[j,k] (g + E[phi | z_t = j, z_{t+1} = k] - E[phi]).

Every weight is a softmax of log quantities; a state without incoming mass has r = W[t, k], one without outgoing mass
s = 0 (both are multiplied by a marginal of exactly 0).  Pinned to torch double-backward, to the covariance over all
paths and to tests/_hmm_vjp_numpy.py by tests/test_hmm_perstep_vjp_cpu.py."""
import numpy as np


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


def estep_perstep_vjp(init, pair, node, g=0.0, u0=None, V=None, W=None):
    """One sequence: init (K), pair (T-1,K,K), node (T,K) log-potentials (entries may be -inf); cotangents g (scalar),
    u0 (K), V (T-1,K,K), W (T,K), None = 0.  -> (d_init (K), d_pair (T-1,K,K), d_node (T,K))."""
    init, pair, node = (np.asarray(x, float) for x in (init, pair, node))
    T, K = node.shape
    pair = pair.reshape(T - 1, K, K)
    g = 0.0 if g is None else float(g)
    u0 = np.zeros(K) if u0 is None else np.asarray(u0, float)
    V = np.zeros((T - 1, K, K)) if V is None else np.asarray(V, float).reshape(T - 1, K, K)
    W = np.zeros((T, K)) if W is None else np.asarray(W, float)
    with np.errstate(all="ignore"):
        la = np.empty((T, K))
        r = np.empty((T, K))
        la[0] = init + node[0]
        r[0] = u0 + W[0]
        for t in range(T - 1):
            lp, w = _lse(la[t][:, None] + pair[t], 0)                  # w[j, k]: softmax over j
            la[t + 1] = node[t + 1] + lp
            r[t + 1] = (w * (r[t][:, None] + V[t])).sum(0) + W[t + 1]
        logZ, gam = _lse(la[T - 1], 0)
        c = g - float(gam @ r[T - 1])
        d_node = np.zeros((T, K))
        d_pair = np.zeros((T - 1, K, K))
        d_node[T - 1] = gam * (c + r[T - 1])
        lb = np.zeros(K)
        s = np.zeros(K)
        for t in range(T - 2, -1, -1):
            y = W[t + 1] + s
            lb, q = _lse(pair[t] + (node[t + 1] + lb)[None, :], 1)     # q[j, k]: softmax over k
            s = (q * (V[t] + y[None, :])).sum(1)
            lg = la[t] + lb - logZ
            gam = np.where(np.isfinite(lg), np.exp(lg), 0.0)
            d_pair[t] = gam[:, None] * q * (c + r[t][:, None] + V[t] + y[None, :])
            d_node[t] = gam * (c + r[t] + s)
    return d_node[0].copy(), d_pair, d_node


def estep_perstep_vjp_batch(init, pair, node, lengths=None, g=None, u0=None, V=None, W=None):
    """A batch, sequence by sequence (each cut to its length): init (K), pair (T-1,K,K) or (B,T-1,K,K), node (B,T,K);
    cotangents g (B), u0 (B,K), V (B,T-1,K,K), W (B,T,K) or None.  -> per-sequence d_init (B,K), d_pair (B,T-1,K,K),
    d_node (B,T,K), with d_node[b, L:] = 0 and d_pair[b, L-1:] = 0.  Nothing behind a sequence's length is read."""
    node = np.asarray(node, float)
    B, T, K = node.shape
    pair = np.asarray(pair, float)
    di, dp, dn = np.zeros((B, K)), np.zeros((B, T - 1, K, K)), np.zeros((B, T, K))
    for b in range(B):
        L = T if lengths is None else int(lengths[b])
        pb = pair[b] if pair.ndim == 4 else pair
        di[b], dp[b, :L - 1], dn[b, :L] = estep_perstep_vjp(
            init, pb[:L - 1], node[b, :L], 0.0 if g is None else float(g[b]), None if u0 is None else u0[b],
            None if V is None else V[b, :L - 1], None if W is None else W[b, :L])
    return di, dp, dn


def scale(g, u0, V, W, L):
    """|g| + L max|cotangent|: the size of phi, to which the tolerances of the tests are relative"""
    mx = max([0.0] + [float(np.max(np.abs(x))) for x in (u0, V, W) if x is not None and np.size(x)])
    return abs(0.0 if g is None else float(g)) + L * mx
