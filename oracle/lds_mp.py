"""TEST INFRASTRUCTURE: the LDS E-step, its message-level parts and their directional derivatives in 40-60 digits (mpmath).

Not a restatement of the reference's algorithm (that is oracle/lds_numpy.py, svae/lds/lds_inference.py:127-178) but the
arbiter between implementations of it where fp64 conditioning makes them disagree: the joint precision of x_0 .. x_{T-1}
under svae/lds/gaussian.py:52-66's conventions (precision blocks -2 J11, -J12, -2 J22 of a pair potential; node and init
potentials on the diagonal) is block tridiagonal; block LDL' forward, back substitution backward, everything in `dps`
digits.  Only tests/ and tools/ import this."""
import numpy as np


def smoothed_means_mp(init, pair, node_J, node_h, dps=60):
    """init = (J (n,n), h (n,)[, ..]), pair = (J11, J12, J22[, ..]) homogeneous, node_J / node_h (T, n) diagonal node
    potentials: E[x_t] (T, n) as float64 of the `dps`-digit solution"""
    import mpmath as mp
    old = mp.mp.dps
    mp.mp.dps = dps
    try:
        M = lambda a: mp.matrix(np.asarray(a, float).tolist())
        iJ, ih = np.asarray(init[0], float), np.asarray(init[1], float)
        J11, J12, J22 = [np.asarray(x, float) for x in pair[:3]]
        node_J, node_h = np.asarray(node_J, float), np.asarray(node_h, float)
        T, n = node_h.shape
        A, h = [], []
        for s in range(T):
            a = np.diag(node_J[s]) + (iJ if s == 0 else 0) + (J11 if s < T - 1 else 0) + (J22 if s > 0 else 0)
            A.append(M(-2 * a))
            h.append(M((node_h[s] + (ih if s == 0 else 0)).reshape(-1, 1)))
        Bm = M(-J12)                                           # block (t, t + 1) of the joint precision
        D, y = [A[0]], [h[0]]
        for s in range(1, T):
            Di = mp.inverse(D[s - 1])
            D.append(A[s] - Bm.T * Di * Bm)
            y.append(h[s] - Bm.T * Di * y[s - 1])
        x = [None] * T
        x[T - 1] = mp.lu_solve(D[T - 1], y[T - 1])
        for s in range(T - 2, -1, -1):
            x[s] = mp.lu_solve(D[s], y[s] - Bm * x[s + 1])
        return np.array([[float(x[s][i]) for i in range(n)] for s in range(T)])
    finally:
        mp.mp.dps = old


# --- the whole E-step, the message-level functions and directional derivatives, all in `dps` digits ----------------------
#
# Arrays in extended precision are NumPy object arrays of mpmath numbers; every function below takes float64 or such
# arrays and returns float64 (as_float=True) or mp arrays.  Conventions are oracle/lds_numpy.py's: natural parameters
# (J = -1/2 precision), homogeneous (n,n) or per-step (T-1,n,n) pair blocks, diagonal (T,n) node potentials, lognorm
# without the (n/2) log 2pi term.

DPS = 50


def _mpa(x):
    """float data (or mp data) -> object array of mpf (exact conversion)"""
    import mpmath as mp
    a = np.asarray(x, dtype=object)
    return np.vectorize(lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v)), otypes=[object])(a) \
        if a.size else np.zeros(a.shape, dtype=object)


def _f64(x):
    if isinstance(x, (tuple, list)):
        return type(x)(_f64(y) for y in x)
    if isinstance(x, (int, float)):
        return x
    return np.asarray(np.vectorize(float, otypes=[float])(x) if np.size(x) else np.zeros(np.shape(x)), dtype=float)


def _chol(A):
    """lower Cholesky factor of an SPD object matrix"""
    import mpmath as mp
    n = A.shape[0]
    L = np.zeros((n, n), dtype=object)
    L[:] = mp.mpf(0)
    for j in range(n):
        L[j, j] = mp.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def _lsolve(L, B):
    """L X = B, L lower; B (n,) or (n,k)"""
    X = np.array(B, dtype=object, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - np.dot(L[i, :i], X[:i])) / L[i, i]
    return X


def _ltsolve(L, B):
    """L' X = B, L lower"""
    X = np.array(B, dtype=object, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - np.dot(L[i + 1:, i], X[i + 1:])) / L[i, i]
    return X


def _inv_logdet(A):
    import mpmath as mp
    L = _chol(A)
    n = A.shape[0]
    I = np.zeros((n, n), dtype=object)
    I[:] = mp.mpf(0)
    for i in range(n):
        I[i, i] = mp.mpf(1)
    Ai = _ltsolve(L, _lsolve(L, I))
    return (Ai + Ai.T) / 2, 2 * sum(mp.log(L[i, i]) for i in range(n))


def _diag(v):
    import mpmath as mp
    D = np.zeros((len(v), len(v)), dtype=object)
    D[:] = mp.mpf(0)
    for i in range(len(v)):
        D[i, i] = v[i]
    return D


def _outer(a, b):
    return np.outer(a, b).astype(object)


def _pair_mp(pair, t):
    J11, J12, J22 = pair[:3]
    return (J11, J12, J22) if J11.ndim == 2 else (J11[t], J12[t], J22[t])


def _logZ_sum(z, steps=1):
    """sum of a log-normaliser entry: a scalar counted `steps` times, or an array summed"""
    z = _mpa(z)
    return z.sum() if z.ndim else steps * z[()]


class _digits(object):
    def __init__(self, dps):
        self.dps = dps

    def __enter__(self):
        import mpmath as mp
        self.old, mp.mp.dps = mp.mp.dps, self.dps

    def __exit__(self, *exc):
        import mpmath as mp
        mp.mp.dps = self.old


def estep_mp(natparam, node_params, dps=DPS, as_float=True):
    """(lognorm, (E_init, E_pair, E_node)) shaped as oracle/lds_numpy.natural_lds_estep_general's, from the block-tridiagonal
    joint precision: forward block elimination (pivots D_t, log det = sum of log det D_t), back substitution for E[x], and
    the diagonal / first off-diagonal blocks of the inverse by the backward recursion
        S_{T-1} = D_{T-1}^-1,   G_t = -D_t^-1 B_t,   S_{t,t+1} = G_t S_{t+1},   S_t = D_t^-1 + G_t S_{t+1} G_t'
    where B_t = -J12_t is block (t, t+1).  E_pair[1] is E[x_t x_{t+1}'] (lds_numpy's order)."""
    with _digits(dps):
        (init, pair) = natparam
        iJ, ih = _mpa(init[0]), _mpa(init[1])
        lz = sum((_logZ_sum(z) for z in init[2:]), 0)
        pair = tuple(_mpa(x) for x in pair[:3]) + ((pair[3] if len(pair) > 3 else 0.),)
        nJ, nh = _mpa(node_params[0]), _mpa(node_params[1])
        T, n = nh.shape
        inhomog = pair[0].ndim == 3
        if len(node_params) > 2:
            lz = lz + _mpa(node_params[2]).sum()
        if T > 1:
            lz = lz + _logZ_sum(pair[3], 1 if inhomog else T - 1)
        D, y, Di = [], [], []
        for t in range(T):
            a = _diag(nJ[t]) + (iJ if t == 0 else 0)
            if t < T - 1:
                a = a + _pair_mp(pair, t)[0]
            if t > 0:
                a = a + _pair_mp(pair, t - 1)[2]
            A = -2 * a
            h = nh[t] + (ih if t == 0 else 0)
            if t > 0:
                Bp = -_pair_mp(pair, t - 1)[1]
                A = A - np.dot(Bp.T, np.dot(Di[t - 1], Bp))
                h = h - np.dot(Bp.T, np.dot(Di[t - 1], y[t - 1]))
            Dinv, logdet = _inv_logdet(A)
            D.append(logdet), y.append(h), Di.append(Dinv)
        lognorm = lz - sum(D) / 2
        mu, S, C = [None] * T, [None] * T, [None] * T
        mu[T - 1], S[T - 1] = np.dot(Di[T - 1], y[T - 1]), Di[T - 1]
        for t in range(T - 2, -1, -1):
            G = -np.dot(Di[t], -_pair_mp(pair, t)[1])
            mu[t] = np.dot(Di[t], y[t]) + np.dot(G, mu[t + 1])
            C[t] = np.dot(G, S[t + 1])                                  # Cov(x_t, x_{t+1})
            S[t] = Di[t] + np.dot(C[t], G.T)
            S[t] = (S[t] + S[t].T) / 2
        # 1/2 h' P^-1 h = 1/2 sum_t y_t' D_t^-1 y_t  (the forward-eliminated right-hand sides)
        lognorm = lognorm + sum(np.dot(y[t], np.dot(Di[t], y[t])) for t in range(T)) / 2
        ExxT = [S[t] + _outer(mu[t], mu[t]) for t in range(T)]
        Exxn = [C[t] + _outer(mu[t], mu[t + 1]) for t in range(T - 1)]
        E_init = (ExxT[0], mu[0], 1., 1.)
        if inhomog:
            st = lambda xs: np.stack(xs) if xs else np.zeros((0, n, n), dtype=object)
            E_pair = (st(ExxT[:-1]), st(Exxn), st(ExxT[1:]), np.ones(T - 1))
        else:
            z = _mpa(np.zeros((n, n)))
            E_pair = (sum(ExxT[:-1], z), sum(Exxn, z), sum(ExxT[1:], z), float(T - 1))
        E_node = (np.stack([np.diag(x) for x in ExxT]), np.stack(mu), np.ones(T))
        out = (lognorm, (E_init, E_pair, E_node))
        return _f64(out) if as_float else out


def filter_mp(init_params, pair_params, node_params, dps=DPS, as_float=True):
    """oracle/lds_numpy.natural_filter_forward_general in `dps` digits -> (((J_pred, h_pred), (J_filt, h_filt)), lognorm)"""
    import mpmath as mp
    with _digits(dps):
        J, h = _mpa(init_params[0]), _mpa(init_params[1])
        lognorm = sum((_logZ_sum(z) for z in init_params[2:]), mp.mpf(0))
        nJ, nh = _mpa(node_params[0]), _mpa(node_params[1])
        nz = _mpa(node_params[2]) if len(node_params) > 2 else _mpa(np.zeros(nh.shape[0]))
        pair = tuple(_mpa(x) for x in pair_params[:3])
        pz = _mpa(pair_params[3]) if len(pair_params) > 3 else _mpa(0.)
        T, n = nh.shape
        Jp, hp, Jf, hf = [], [], [], []
        for t in range(T):
            Jp.append(J), hp.append(h)
            J, h = J + _diag(nJ[t]), h + nh[t]
            lognorm = lognorm + nz[t]
            Jf.append(J), hf.append(h)
            if t < T - 1:                                                # natural_predict
                J11, J12, J22 = _pair_mp(pair, t)
                L = _chol(-2 * J - 2 * J11)
                v = _lsolve(L, h)
                lognorm = lognorm + np.dot(v, v) / 2 - sum(mp.log(L[i, i]) for i in range(n))
                lognorm = lognorm + (pz[t] if pz.ndim else pz[()])
                h = np.dot(J12.T, _ltsolve(L, v))                        # -(-J12)' L^-T v
                tmp = _lsolve(L, -J12)
                J = -(-2 * J22 - np.dot(tmp.T, tmp)) / 2
        L = _chol(-2 * Jf[-1])                                           # natural_lognorm
        v = _lsolve(L, hf[-1])
        lognorm = lognorm + np.dot(v, v) / 2 - sum(mp.log(L[i, i]) for i in range(n))
        out = (((np.stack(Jp), np.stack(hp)), (np.stack(Jf), np.stack(hf))), lognorm)
        return _f64(out) if as_float else out


def smoother_on_messages_mp(forward_messages, pair_params, dps=DPS, as_float=True):
    """oracle/lds_numpy.natural_smoother_general (diagonal node statistics) in `dps` digits, the messages taken as given
    -> (E_init, E_pair, E_node)"""
    with _digits(dps):
        (Jp, hp), (Jf, hf) = ((_mpa(a), _mpa(b)) for a, b in forward_messages)
        pair = tuple(_mpa(x) for x in pair_params[:3])
        inhomog = pair[0].ndim == 3
        T, n = hf.shape
        Sig, _ = _inv_logdet(-2 * Jf[-1])
        mu = np.dot(Sig, hf[-1])
        stats = [(mu, Sig + _outer(mu, mu), None)]
        Jns, hns, mun = Jf[-1], hf[-1], mu
        for t in range(T - 2, -1, -1):                                   # natural_rts_backward_step
            J11, J12, J22 = _pair_mp(pair, t)
            A11 = -2 * Jf[t] - 2 * J11
            A12 = -J12
            A22 = -2 * Jns + 2 * Jp[t + 1] - 2 * J22
            L = _chol(A22)
            temp = _lsolve(L, A12.T)
            Js = A11 - np.dot(temp.T, temp)
            hs = hf[t] - np.dot(temp.T, _lsolve(L, hns - hp[t + 1]))
            sigma, _ = _inv_logdet(Js)
            mu = np.dot(sigma, hs)
            ExnxT = -_ltsolve(L, _lsolve(L, np.dot(A12.T, sigma))) + _outer(mun, mu)
            stats.insert(0, (mu, sigma + _outer(mu, mu), ExnxT))
            Jns, hns, mun = -Js / 2, hs, mu
        E_init = (stats[0][1], stats[0][0], 1., 1.)
        pairs = [(a[1], a[2].T, b[1]) for a, b in zip(stats[:-1], stats[1:])]
        if inhomog:
            st = lambda xs: np.stack(xs) if xs else np.zeros((0, n, n), dtype=object)
            E_pair = tuple(st([p[i] for p in pairs]) for i in range(3)) + (np.ones(T - 1),)
        else:
            z = _mpa(np.zeros((n, n)))
            E_pair = tuple(sum((p[i] for p in pairs), z) for i in range(3)) + (float(T - 1),)
        E_node = (np.stack([np.diag(s[1]) for s in stats]), np.stack([s[0] for s in stats]), np.ones(T))
        out = (E_init, E_pair, E_node)
        return _f64(out) if as_float else out


def sample_on_messages_mp(forward_messages, pair_params, eps, dps=DPS, as_float=True):
    """oracle/lds_numpy.natural_sample_backward_general in `dps` digits (eps[t] (S,n) the noise of x_t) -> (T,S,n)"""
    with _digits(dps):
        _, (Jf, hf) = ((_mpa(a), _mpa(b)) for a, b in forward_messages)
        pair = tuple(_mpa(x) for x in pair_params[:2]) + (None,)
        eps = _mpa(eps)
        T, n = hf.shape
        S = eps.shape[1]
        out = np.zeros((T, S, n), dtype=object)

        def sample(J, h, e):                  # h (S,n), e (S,n)
            L = _chol(-2 * J)
            return (_ltsolve(L, _lsolve(L, h.T)) + _ltsolve(L, e.T)).T

        out[T - 1] = sample(Jf[T - 1], np.stack([hf[T - 1]] * S), eps[T - 1])
        for t in range(T - 2, -1, -1):
            J11, J12 = (pair[0], pair[1]) if pair[0].ndim == 2 else (pair[0][t], pair[1][t])
            out[t] = sample(Jf[t] + J11, hf[t] + np.dot(J12, out[t + 1].T).T, eps[t])
        return _f64(out) if as_float else out


def inference_mp(natparam, node_params, eps, dps=DPS, as_float=True):
    """the training forward (E-step + sampler on the filter's messages) in `dps` digits ->
    (lognorm, (diag E[xx'] (T,n), E[x] (T,n)), samples (T,S,n)): estep_mp, and sample_on_messages_mp on filter_mp's
    messages with the noise eps (T,S,n).  jvp_mp accepts it: the directional derivative of
        L = g_l lognorm + <g_d, diag E[xx']> + <g_x, E[x]> + <g_s, samples>
    is that combination of jvp_mp(inference_mp, (natparam, node_params, eps), direction)'s leaves."""
    with _digits(dps):
        init, pair = natparam
        lognorm, (_, _, E_node) = estep_mp(natparam, node_params, dps=dps, as_float=False)
        messages, _ = filter_mp(init, pair, node_params, dps=dps, as_float=False)
        samples = sample_on_messages_mp(messages, pair, eps, dps=dps, as_float=False)
        out = (lognorm, (E_node[0], E_node[1]), samples)
        return _f64(out) if as_float else out


def _axpy(x, v, s):
    """x + s v over matching nested structures (v None / 0 = no perturbation of that leaf); x's leaves become mp arrays"""
    if isinstance(x, (tuple, list)):
        vs = v if isinstance(v, (tuple, list)) else [None] * len(x)
        return type(x)(_axpy(a, b, s) for a, b in zip(x, vs))
    xm = _mpa(x)
    return xm if v is None else xm + s * _mpa(v)


def _diff(a, b, h2):
    if isinstance(a, (tuple, list)):
        return type(a)(_diff(x, y, h2) for x, y in zip(a, b))
    if isinstance(a, (int, float)) and isinstance(b, (int, float)):
        return 0.
    return _f64((a - b) / h2)


def jvp_mp(f, args, direction, dps=60, step=1e-20):
    """d/ds f(*(args + s direction)) at s = 0 for f one of estep_mp / filter_mp / smoother_on_messages_mp /
    sample_on_messages_mp, by a central difference evaluated in `dps` digits: the truncation error is O(step^2) relative
    (1e-40 at the default step) and the difference loses log10(1/step) of the `dps` digits, so the float64 result is the
    exact derivative rounded.  `direction` has the structure of `args`, with None for leaves that are not perturbed."""
    import mpmath as mp
    with _digits(dps):
        s = mp.mpf(step)
        up = f(*_axpy(tuple(args), tuple(direction), s), dps=dps, as_float=False)
        dn = f(*_axpy(tuple(args), tuple(direction), -s), dps=dps, as_float=False)
        return _diff(up, dn, 2 * s)
