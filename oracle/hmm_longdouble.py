"""Extended-precision (x87 80-bit long double, eps ~1e-19) HMM log-normaliser and E-step.  TEST INFRASTRUCTURE.

The truth for LONG sequences.  oracle/hmm_numpy.hmm_estep is an fp64 log-space recursion: its log-messages grow like
|log Z| ~ 2.5 T, so every step rounds at |log alpha| 2^-53 absolute -- about 1e-11 by T = 25 000, which the posteriors
inherit as a RELATIVE error (3e-9 at T = 22 785).  The scaled fp64 kernels are three orders of magnitude more
accurate than that there, and only arithmetic with more digits can referee them.

Two independent algorithms at the same precision, which pin each other without a 60-digit run at T = 22 785:

  hmm_estep / hmm_logZ                the log-space forward-backward of oracle/hmm_numpy in np.longdouble, with a
                                      max-shifted log-sum-exp of its own (-inf entries are zero terms; an empty maximum
                                      shifts by 0, so there is never inf - inf); the log-messages are shifted to
                                      log-sum-exp 0 at every step and log Z is the sum of the shifts; E_trans summed in
                                      long double
  hmm_estep_scaled / hmm_logZ_scaled  the scaled recursion: probability-space messages normalised at every step, log Z
                                      from the normalisers (long double's exponent range, 1e-4932, is what lets a
                                      per-step scaled recursion stand where the fp64 one leaves its range)

Signatures and return shapes are oracle/hmm_numpy's -- natparam = (init (K), pair (K,K), node (T,K)) of ONE sequence ->
logZ, (E_init, E_trans, E_states) -- and every result is long double: callers round.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
assert EPS < 2e-19, ("oracle/hmm_longdouble.py needs an 80-bit (or wider) long double: np.longdouble has eps = %.3g on "
                     "this platform, no more digits than the arithmetic it is meant to judge" % EPS)

_BLOCK = 2048      # steps of E_trans terms held at once


def _leaves(natparam):
    init, pair, node = (np.asarray(x, dtype=LD) for x in natparam)
    T, K = node.shape
    assert init.shape == (K,) and pair.shape == (K, K), "one sequence: init (K), pair (K,K), node (T,K)"
    return init, pair, node


def logsumexp(x, axis=None):
    """log sum exp over `axis` in long double: shifted by the maximum where that is finite, by 0 where it is not (all
    terms -inf -> -inf, no inf - inf)"""
    x = np.asarray(x, dtype=LD)
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, LD(0))
    with np.errstate(divide="ignore"):
        out = m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def _finite_or_zero(z):
    return np.where(np.isfinite(z), z, LD(0))


def _forward(init, pair, node):
    """-> (la (T,K), logZ): la[t] = log of the filtered message, shifted to log-sum-exp 0 at every step, the shifts summed
    into logZ.  (A recursion that carries the unshifted log alpha_t, as oracle/hmm_numpy does, rounds every step at
    |log alpha_t| eps with |log alpha_t| ~ 2.5 t: in long double that is still 8e-13 on the posteriors at T = 22 785, no
    better than the fp64 arithmetic it is to judge.  Shifted, every entry stays O(10) and a step rounds at 1e-18.)"""
    T, K = node.shape
    la = np.empty((T, K), LD)
    logZ = LD(0)
    x = init + node[0]
    for t in range(T):
        if t:
            x = logsumexp(la[t - 1][:, None] + pair, axis=0) + node[t]
        z = logsumexp(x)
        la[t] = x - _finite_or_zero(z)
        logZ = logZ + z
    return la, logZ


def hmm_logZ(natparam):
    return _forward(*_leaves(natparam))[1]


def hmm_estep(natparam):
    init, pair, node = _leaves(natparam)
    T, K = node.shape
    la, logZ = _forward(init, pair, node)
    lb = np.zeros((T, K), LD)                # log backward messages, shifted to maximum 0 at every step
    for t in range(T - 2, -1, -1):
        x = logsumexp(pair + (node[t + 1] + lb[t + 1])[None, :], axis=1)
        lb[t] = x - _finite_or_zero(np.max(x))
    # the shifts cancel in every posterior: each is normalised by its own log-sum-exp
    g = la + lb
    E_states = np.exp(g - _finite_or_zero(logsumexp(g, axis=-1))[:, None])
    E_trans = np.zeros((K, K), LD)
    for t0 in range(0, T - 1, _BLOCK):
        t1 = min(t0 + _BLOCK, T - 1)
        x = (la[t0:t1, :, None] + pair[None] + (node[t0 + 1:t1 + 1] + lb[t0 + 1:t1 + 1])[:, None, :]).reshape(t1 - t0, K * K)
        E_trans += np.exp(x - _finite_or_zero(logsumexp(x, axis=-1))[:, None]).sum(axis=0).reshape(K, K)
    return logZ, (E_states[0].copy(), E_trans, E_states)


# ---- the second algorithm: scaled messages, normalised every step --------------------------------------------------------------
def _shifted_exp(x):
    """(exp(x - m), m) along the last axis, m the row maximum where finite, else 0"""
    m = np.max(x, axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, LD(0))
    return np.exp(x - m), m[..., 0]


def _scaled_forward(init, pair, node):
    T, K = node.shape
    pm = np.max(pair)
    pm = pm if np.isfinite(pm) else LD(0)
    P = np.exp(pair - pm)
    e0, m0 = _shifted_exp(init + node[0])
    e, m = _shifted_exp(node)
    e[0], m[0] = e0, m0
    alpha, c = np.empty((T, K), LD), np.empty(T, LD)
    a = e[0]
    for t in range(T):
        if t:
            a = (alpha[t - 1] @ P) * e[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
    with np.errstate(divide="ignore"):
        logZ = np.log(c).sum() + m.sum() + (T - 1) * pm
    return P, e, c, alpha, logZ


def hmm_logZ_scaled(natparam):
    return _scaled_forward(*_leaves(natparam))[-1]


def hmm_estep_scaled(natparam):
    init, pair, node = _leaves(natparam)
    T, K = node.shape
    P, e, c, alpha, logZ = _scaled_forward(init, pair, node)
    w = np.zeros((T, K), LD)                 # w[t] = e_t o beta_t / c_t: what step t hands back to step t - 1
    beta = np.ones(K, LD)
    E_states = np.empty((T, K), LD)
    E_states[T - 1] = alpha[T - 1]
    for t in range(T - 1, 0, -1):
        w[t] = e[t] * beta / c[t]
        beta = P @ w[t]
        E_states[t - 1] = alpha[t - 1] * beta
    E_trans = np.zeros((K, K), LD)
    for t0 in range(0, T - 1, _BLOCK):
        t1 = min(t0 + _BLOCK, T - 1)
        E_trans += (alpha[t0:t1, :, None] * w[t0 + 1:t1 + 1, None, :]).sum(axis=0)
    E_trans *= P
    return logZ, (E_states[0].copy(), E_trans, E_states)
