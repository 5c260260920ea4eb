#!/usr/bin/env python3
"""Generate tests/golden/exact_sol_opr_sens_0.npz: the exact derivatives of two_stream_solar's level values (fup, fdn,
amean, summed over the zenith angles with their weights) in a layer's tau, w0 and g and in the surface reflectance
(tests/exact_sol_opr_sens.py: mpmath, 80 digits, central differences with h = 1e-30, rounded once) on the columns that
clima_test_sol_opr_sens is held to, and the reference ALGORITHM's own error on each of them (its float64 restatement
differentiated by autograd against exact).  Needs mpmath and torch (CPU); neither the reference, nor the oracle, nor a
GPU.  Data only: inputs, exact outputs, the reference's error.

Columns sNN (`n` of them), TOA-first: tau, w0, g (nz), zen_u, zen_w (nzen), rsfc (1), levels (the top, two interior ones,
the surface), the twelve arrays up_tau ... am_rsfc ((nrow, nz), (nrow) for rsfc) and e_ref (12, in NAMES' order): the
largest |restatement - exact| of each array.  CASES lists what each column is there for.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import exact_sol_opr_sens as X  # noqa: E402

THICK, W0_CAP = 3.0e4, 0.99999
ZEN4_U, ZEN4_W = [0.93, 0.61, 0.34, 0.11], [0.17, 0.38, 0.31, 0.14]

# (nz, what, Rsfc, zenith angles, weights)
CASES = [
    (1, "plain", 0.3, [0.6], [1.0]),
    (1, "cap", 1.0, [0.8], [1.0]),                      # w0 at the cap with negative g, over a perfect reflector
    (2, "w0zero", 0.0, [0.5], [1.0]),                   # w0 = 0 throughout over a black surface: fup = 0
    (4, "zero_thick", 0.5, [0.7], [1.0]),               # a layer with tau = 0 over one with tau = 3e4, a lit layer on
                                                        # either side (under tau = 3e4 alone every derivative underflows and
                                                        # the 80-digit solve's residual, 1e-51 and less, is all an array holds)
    (3, "plain", 0.25, ZEN4_U, ZEN4_W),                 # four angles with unequal weights, negative g
    (5, "plain", 0.4, [0.05], [1.0]),                   # a grazing angle
    (7, "near", 0.3, None, [1.0]),                      # |lambda u0 - 1| about 1e-3 in layer 3
    (12, "plain", 0.0, ZEN4_U, ZEN4_W),
    (20, "mixed", 0.6, [0.05, 0.45], [0.3, 0.7]),       # grazing and thick together
    (33, "w0zero", 0.7, [0.65], [1.0]),
    (63, "plain", 0.2, [0.55], [1.0]),
    (64, "mixed", 0.35, ZEN4_U, ZEN4_W),
    (65, "plain", 1.0, [0.75], [1.0]),
    (129, "mixed", 0.15, [0.9, 0.3], [0.45, 0.55]),
]


def levels_of(nz):
    return sorted(set([0, nz // 3, (2 * nz + 1) // 3, nz]))


def lam_of(w0, g):
    """lambda of two_stream_solar for one layer, in float64"""
    w = w0 * (1.0 - g * g) / (1.0 - w0 * g * g)
    gt = g / (1.0 + g)
    gam1 = np.sqrt(3.0) * (2.0 - w * (1.0 + gt)) / 2.0
    gam2 = np.sqrt(3.0) * w * (1.0 - gt) / 2.0
    return np.sqrt(gam1 * gam1 - gam2 * gam2)


def column(n):
    """-> tau, w0, g, zen_u, zen_w, rsfc of stored column n"""
    nz, what, rsfc, zu, zw = CASES[n]
    rng = np.random.default_rng(7000 + 100 * n + nz)
    tau = 10.0 ** rng.uniform(-3.0, 0.5, nz)
    w0 = rng.uniform(0.05, 0.98, nz)
    g = rng.uniform(-0.6, 0.9, nz)
    if nz >= 40:
        tau = tau * 0.1          # (so that light reaches the lower half of a long column)
    if what == "cap":
        w0[0], g[0] = W0_CAP, -0.4
    elif what == "w0zero":
        w0[:] = 0.0
    elif what == "zero_thick":
        tau[1], tau[2] = 0.0, THICK
    elif what == "near":
        zu = [float((1.0 + 1.0e-3) / lam_of(w0[3], g[3]))]
    elif what == "mixed":
        w0[2] = 0.0
        tau[5] = 0.0
        w0[nz // 2], g[nz // 2] = W0_CAP, -0.35
        tau[nz - 3] = THICK
    return tau, w0, g, np.array(zu, dtype=np.float64), np.array(zw, dtype=np.float64), float(rsfc)


def case(n, with_ref=True):
    tau, w0, g, zu, zw, rsfc = column(n)
    lv = levels_of(len(tau))
    ex = X.exact_sol_opr_sens(tau, w0, g, zu, zw, rsfc, lv)
    out = dict(tau=tau, w0=w0, g=g, zen_u=zu, zen_w=zw, rsfc=np.array([rsfc]), levels=np.array(lv, dtype=np.int32))
    out.update(ex)
    if with_ref:
        rs = X.restated_sol_opr_sens(tau, w0, g, zu, zw, rsfc, lv)
        assert all(np.all(np.isfinite(rs[k])) for k in X.NAMES), "the restatement is not finite: no yardstick"
        out["e_ref"] = np.array([np.max(np.abs(rs[k] - ex[k])) for k in X.NAMES])
    return out


def main():
    out = {}
    for n in range(len(CASES)):
        c = case(n)
        for k, v in c.items():
            out["s%02d_%s" % (n, k)] = v
        sc = [np.max(np.abs(c[k])) for k in X.NAMES]
        print("s%02d nz %d %s: e_ref / scale %s" % (n, CASES[n][0], CASES[n][1], " ".join(
            "%s %.1e" % (k, e / s if s else 0.0) for k, e, s in zip(X.NAMES, c["e_ref"], sc))), flush=True)
    out["n"] = np.array([len(CASES)])
    path = os.path.join(HERE, "exact_sol_opr_sens_0.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d columns, %d bytes" % (path, len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
