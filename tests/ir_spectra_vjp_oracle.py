"""The yardstick of radtran_ir_spectra_batch_vjp: the contraction
    grad_x(j, c) = sum over d, a, l of (gs_d(l, a, c) + gn_d(a, c) dfreq(l)) W_d(l, a, j) dB/dT(avg_freq(l), x_c(j))
with dB/dT from the closed formula at 40 digits (mpmath, the constants of closed_forms: clima_const.f90), rounded once, and
the sum by math.fsum (exact, rounded once).  It shares nothing with the library: neither its dB/dT nor its order of
summation.  Errors are stated over the sum of |terms| of that (j, c)."""
import math

import mpmath
import numpy as np

import closed_forms as CF


def dplanck_dT(nu, T):
    """d/dT of clima_eqns.f90's planck_fcn, mW sr^-1 m^-2 Hz^-1 K^-1, at CF.DPS digits:
    K x e^x / (T (e^x - 1)^2) = K x e^-x / (T expm1(-x)^2), x = h nu / (k T), K = 1000 * 2 h nu^3 / c^2"""
    with mpmath.workdps(CF.DPS):
        h, c, kb = mpmath.mpf(CF.PLANK), mpmath.mpf(CF.C_LIGHT), mpmath.mpf(CF.K_BOLTZ_SI)
        nu, T = mpmath.mpf(float(nu)), mpmath.mpf(float(T))
        x = h * nu / (kb * T)
        return 1000 * (2 * h * nu ** 3 / c ** 2) * x * mpmath.exp(-x) / (T * mpmath.expm1(-x) ** 2)


def dplanck_table(avg_freq, x):
    """float64 [l, j] of dplanck_dT(avg_freq[l], x[j]) (an underflow rounds to 0.0, as it must)"""
    return np.array([[float(dplanck_dT(nu, t)) for t in x] for nu in avg_freq])


def vjp(avg_freq, dfreq, Ts, T, weights, grads):
    """(grad_T_surface (ncol), grad_T (nz, ncol), sum_abs (nz+1, ncol)): the contraction by math.fsum and the sum of |terms|
    of every (j, c).  weights: "w_up" / "w_dn" (nw_ir, nsel, nz+1); grads: "fup" / "fdn" (nw_ir, nsel, ncol), "fup_n" /
    "fdn_n" (nsel, ncol); T (nz, ncol), Ts (ncol)."""
    nz, n = T.shape
    nl = nz + 1
    out, sa = np.zeros((nl, n)), np.zeros((nl, n))
    for c in range(n):
        x = np.concatenate([[Ts[c]], T[:, c]])
        dB = dplanck_table(avg_freq, x)                               # [l, j]
        for j in range(nl):
            terms = []
            for name in ("up", "dn"):
                w = weights.get("w_" + name)
                if w is None:
                    continue
                gs, gn = grads.get("f" + name), grads.get("f%s_n" % name)
                if gs is None and gn is None:
                    continue
                G = np.zeros(w.shape[:2])
                if gs is not None:
                    G = G + gs[:, :, c]
                if gn is not None:
                    G = G + gn[None, :, c] * dfreq[:, None]
                terms.append((G * w[:, :, j] * dB[:, j, None]).ravel())
            terms = np.concatenate(terms)
            out[j, c] = math.fsum(terms)
            sa[j, c] = math.fsum(np.abs(terms))
    return out[0].copy(), out[1:].copy(), sa
