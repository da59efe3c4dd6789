"""TEST INFRASTRUCTURE: the global -> local maps and the prior KLs in 50 digits (mpmath) -- the arbiter of the global-step
kernels.  Only tests/ and tools/ import this (oracle/lds_mp.py is the precedent and lends its linear algebra).

Every function takes the float64 NATURAL parameter exactly (no rounding on the way in) and evaluates the map the
reference spells, in `dps` digits:

  dirichlet_expectedstats / dirichlet_logZ     svae/distributions/dirichlet.py:5-11
  niw_expectedstats (fudge 1e-8) / niw_logZ    svae/distributions/niw.py:15-25, 27-31 (natural_to_standard :33-37)
  mniw_expectedstats / mniw_logZ               svae/distributions/mniw.py:33-55, 13-17
  gmm_prior_kl                                 svae/models/gmm.py:54-58
  lds_prior_kl                                 svae/models/lds.py:16-20

so the error of an fp64 evaluation -- a kernel's, or oracle/expfam_numpy.py's -- against these values is that
evaluation's own: the formulas cancel (S = A - b b'/kappa, log-normaliser differences), and no two fp64 evaluations of
them need agree.  The matrix blocks (NIW A; MNIW A, C) are taken as symmetric: the factorisation reads their lower
triangle.  Results are float64 (as_float=True) or object arrays / scalars of mpf."""
from collections import namedtuple

import numpy as np

from .lds_mp import _digits, _f64, _inv_logdet, _mpa

DPS = 50
FUDGE = 1e-8      # niw.py:15, mniw.py:42 (the float64 the reference adds, taken exactly)

# full: the contraction the code spells; shipped: the value the reference AS SHIPPED returns (gmm.py:55-56 flattens with
# util.py:39 `flat`, which after util.py:166 keeps the FIRST scalar only; lds.py:19 uses `contract`, so there shipped ==
# full); scale: |<d eta, E t>| + |log Z(q)| + |log Z(p)|, what the value cancels from; *_mp: the mpf values
KL = namedtuple("KL", "full shipped scale full_mp shipped_mp scale_mp")


def _out(x, as_float):
    return _f64(x) if as_float else x


def _eye(n, v):
    import mpmath as mp
    I = np.zeros((n, n), dtype=object)
    I[:] = mp.mpf(0)
    for i in range(n):
        I[i, i] = v
    return I


def _sym(X):
    return (X + X.T) / 2


def _psi(x):
    import mpmath as mp
    return mp.digamma(x)


def _multigammaln(a, d):
    """scipy.special.multigammaln: d (d-1)/4 log pi + sum_{j<d} loggamma(a - j/2)"""
    import mpmath as mp
    return mp.mpf(d * (d - 1)) / 4 * mp.log(mp.pi) + sum(mp.loggamma(a - mp.mpf(j) / 2) for j in range(d))


# --- Dirichlet -------------------------------------------------------------------------------------------------------

def _dirichlet_es(nat):
    alpha = _mpa(nat) + 1
    rows = alpha.reshape(-1, alpha.shape[-1])
    out = np.array([[_psi(a) - _psi(sum(r)) for a in r] for r in rows], dtype=object)
    return out.reshape(alpha.shape)


def _dirichlet_logZ(nat):
    import mpmath as mp
    alpha = _mpa(nat) + 1
    rows = alpha.reshape(-1, alpha.shape[-1])
    return sum(sum(mp.loggamma(a) for a in r) - mp.loggamma(sum(r)) for r in rows)


def dirichlet_expectedstats(natparam, dps=DPS, as_float=True):
    """dirichlet.py:5-7, rows along the last axis"""
    with _digits(dps):
        return _out(_dirichlet_es(natparam), as_float)


def dirichlet_logZ(natparam, dps=DPS, as_float=True):
    """dirichlet.py:9-11, summed over the rows"""
    with _digits(dps):
        z = _dirichlet_logZ(natparam)
        return float(z) if as_float else z


# --- NIW (dense-packed (d+2, d+2)) -----------------------------------------------------------------------------------

def _niw_standard(nat):
    """niw.py:33-37 on one dense-packed parameter"""
    nat = _mpa(nat)
    d = nat.shape[-1] - 2
    A, b, kappa, nu = nat[:d, :d], nat[:d, d], nat[d, d], nat[d + 1, d + 1]
    m = b / kappa
    return A - np.outer(b, m), m, kappa, nu


def _niw_one(nat):
    """(expected statistics dense-packed, log Z) of one parameter, from one factorisation of S"""
    import mpmath as mp
    S, m, kappa, nu = _niw_standard(nat)
    d = m.shape[0]
    Sinv, logdetS = _inv_logdet(S)
    E_J = nu * Sinv + _eye(d, mp.mpf(FUDGE))
    E_h = np.dot(E_J, m)
    E_hTJinvh = d / kappa + np.dot(m, E_h)
    E_logdetJ = sum(_psi((nu - i) / 2) for i in range(d)) + d * mp.log(2) - logdetS
    out = np.zeros((d + 2, d + 2), dtype=object)
    out[:] = mp.mpf(0)
    out[:d, :d], out[:d, d], out[d, d], out[d + 1, d + 1] = -E_J / 2, E_h, -E_hTJinvh / 2, E_logdetJ / 2
    logZ = d * nu / 2 * mp.log(2) + _multigammaln(nu / 2, d) - nu / 2 * logdetS - mp.mpf(d) / 2 * mp.log(kappa)
    return out, logZ


def _each(natparam):
    a = np.asarray(natparam)
    return a.reshape((-1,) + a.shape[-2:]), a.shape


def niw_expectedstats(natparam, dps=DPS, as_float=True):
    """niw.py:15-25 (fudge 1e-8 included); (d+2, d+2) or (K, d+2, d+2)"""
    with _digits(dps):
        each, shape = _each(natparam)
        return _out(np.array([_niw_one(x)[0] for x in each], dtype=object).reshape(shape), as_float)


def niw_logZ(natparam, dps=DPS, as_float=True):
    """niw.py:27-31, summed over the leading axis"""
    with _digits(dps):
        z = sum(_niw_one(x)[1] for x in _each(natparam)[0])
        return float(z) if as_float else z


# --- MNIW (tuple (A, B, C, d)) ---------------------------------------------------------------------------------------

def _mniw_one(nat):
    """(expected statistics 4-tuple, log Z): mniw.py:33-40 (natural_to_standard), :42-55, :13-17"""
    import mpmath as mp
    A, B, C, nu = _mpa(nat[0]), _mpa(nat[1]), _mpa(nat[2]), _mpa(nat[3]).reshape(-1)[0]
    K, logdetA = _inv_logdet(A)
    M = np.dot(K, B).T
    S = C - np.dot(M, B)
    m = M.shape[0]
    Sinv, logdetS = _inv_logdet(S)
    fI = _eye(m, mp.mpf(FUDGE))
    SinvM = np.dot(Sinv, M)
    E_Sigmainv = nu * Sinv + fI
    E_Sigmainv_A = nu * SinvM
    E_AT_Sigmainv_A = m * K + nu * _sym(np.dot(M.T, SinvM)) + fI
    E_logdet = sum(_psi((nu - i) / 2) for i in range(m)) + m * mp.log(2) - logdetS
    logZ = m * nu / 2 * mp.log(2) + _multigammaln(nu / 2, m) - nu / 2 * logdetS - mp.mpf(m) / 2 * logdetA   # log|K| = -log|A|
    return (-E_AT_Sigmainv_A / 2, E_Sigmainv_A.T, -E_Sigmainv / 2, E_logdet / 2), logZ


def mniw_expectedstats(natparam, dps=DPS, as_float=True):
    """mniw.py:19-20, 42-55 -> (-1/2 E[A' Sinv A], E[Sinv A]', -1/2 E[Sinv], 1/2 E[log|Sinv|])"""
    with _digits(dps):
        es = _mniw_one(natparam)[0]
        return tuple(_f64(x) for x in es[:3]) + (float(es[3]),) if as_float else es


def mniw_logZ(natparam, dps=DPS, as_float=True):
    """mniw.py:13-17"""
    with _digits(dps):
        z = _mniw_one(natparam)[1]
        return float(z) if as_float else z


# --- prior KLs -------------------------------------------------------------------------------------------------------

def _dot(a, b):
    return sum(x * y for x, y in zip(np.asarray(a, dtype=object).reshape(-1), np.asarray(b, dtype=object).reshape(-1)))


def _kl(contraction, first_term, logZ_q, logZ_p):
    scale = abs(contraction) + abs(logZ_q) + abs(logZ_p)
    full, shipped = contraction - (logZ_q - logZ_p), first_term - (logZ_q - logZ_p)
    return KL(float(full), float(shipped), float(scale), full, shipped, scale)


def gmm_global_step(global_natparam, prior_natparam, dps=DPS):
    """Everything the GMM global-step kernels write, from one factorisation per component:
    (dirichlet.expectedstats (K), niw.expectedstats (K, N+2, N+2), KL of gmm.py:54-58)"""
    with _digits(dps):
        (gd, gn), (pd, pn) = global_natparam, prior_natparam
        es_d = _dirichlet_es(gd)
        q = [_niw_one(x) for x in _each(gn)[0]]
        es_n = np.array([x[0] for x in q], dtype=object)
        dd = _mpa(gd) - _mpa(pd)
        contraction = _dot(dd, es_d) + _dot(_mpa(gn) - _mpa(pn), es_n)
        logZ_q = _dirichlet_logZ(gd) + sum(x[1] for x in q)
        logZ_p = _dirichlet_logZ(pd) + sum(_niw_one(x)[1] for x in _each(pn)[0])
        return _f64(es_d), _f64(es_n), _kl(contraction, dd.reshape(-1)[0] * es_d.reshape(-1)[0], logZ_q, logZ_p)


def gmm_prior_kl(global_natparam, prior_natparam, dps=DPS):
    """gmm.py:54-58: <eta_q - eta_p, E_q t> - (log Z(q) - log Z(p)) over (Dirichlet (K), NIW (K, N+2, N+2)) -> KL"""
    return gmm_global_step(global_natparam, prior_natparam, dps)[2]


def lds_global_step(global_natparam, prior_natparam=None, dps=DPS, prior_logZ=None):
    """Everything the LDS global-step kernel writes: (niw.expectedstats (n+2, n+2), mniw.expectedstats 4-tuple,
    log Z of the global factor, KL of lds.py:16-20 or None without a prior).  `prior_logZ`: the prior's log Z as an mpf
    of the same `dps`, where the caller has it already (it takes two factorisations)"""
    with _digits(dps):
        gn, gm = global_natparam
        (es_n, lz_n), (es_m, lz_m) = _niw_one(gn), _mniw_one(gm)
        kl = None
        if prior_natparam is not None:
            pn, pm = prior_natparam
            contraction = _dot(_mpa(gn) - _mpa(pn), es_n)
            for i in range(3):
                contraction += _dot(_mpa(gm[i]) - _mpa(pm[i]), es_m[i])
            contraction += (_mpa(gm[3]).reshape(-1)[0] - _mpa(pm[3]).reshape(-1)[0]) * es_m[3]
            lz_p = prior_logZ if prior_logZ is not None else _niw_one(pn)[1] + _mniw_one(pm)[1]
            kl = _kl(contraction, contraction, lz_n + lz_m, lz_p)
        return _f64(es_n), tuple(_f64(x) for x in es_m[:3]) + (float(es_m[3]),), float(lz_n + lz_m), kl


def lds_prior_kl(global_natparam, prior_natparam, dps=DPS):
    """lds.py:16-20 over (NIW dense (n+2, n+2), MNIW (A, B, C, d)) -> KL (`contract`, not `flat`: shipped == full)"""
    return lds_global_step(global_natparam, prior_natparam, dps)[3]
