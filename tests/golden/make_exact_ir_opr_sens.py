#!/usr/bin/env python3
"""Generate tests/golden/exact_ir_opr_sens_0.npz: the exact derivatives of two_stream_ir's level fluxes in a layer's tau,
w0 and g (tests/exact_ir_opr_sens.py: mpmath, 80 digits, central differences with h = 1e-30, rounded once) on the columns
that clima_test_ir_opr_sens is held to, and the reference ALGORITHM's own error on each of them (its float64 restatement
differentiated by autograd against exact).  Needs mpmath and torch (CPU); neither the reference, nor the oracle, nor a
GPU.  Data only: inputs, exact outputs, the reference's error.

Columns sNN (`n` of them), TOA-first: tau, w0, g (nz), bplanck (nz+1, smooth, rising towards the surface), ir_par
(emissivity, has_hard_surface, ir_tau_min), levels (the top, mid-column, the surface), the six arrays up_tau ... dn_g
(nrow, nz), and e_ref (6, in NAMES' order): the largest |restatement - exact| of each array.
  nz = 1 (rows 0 and 2nz-1 only): a layer at w0 = 0.99999 with negative g; a thin layer (tau <= ir_tau_min); tau = 3e4, w0 = 0.
  nz = 3: (w0 = 0 exactly | w0 = 0.99999, negative g | tau = 3e4) and (thin | just above ir_tau_min | negative g).
  nz = 33 (two row segments) and 65 (three, and a second block of layers): all of these in one column -- layer 2 at w0 = 0,
    layer 5 thin next to layer 6 just above ir_tau_min, the middle layer at w0 = 0.99999 with negative g, layer nz-3 at
    tau = 3e4.
Each with a hard surface (emissivity 0.8) and without one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import exact_ir_opr_sens as X  # noqa: E402

TAU_MIN = 1.0e-6
THIN, ABOVE, THICK, W0_CAP = 3.0e-7, 1.5e-6, 3.0e4, 0.99999
EMISSIVITY = 0.8


def levels_of(nz):
    return sorted(set([0, (nz + 1) // 2, nz]))        # exact_two_stream_cases.adjoint_levels


def column(nz, variant):
    """-> tau, w0, g, bplanck"""
    rng = np.random.default_rng(1000 * nz + variant)
    tau = 10.0 ** rng.uniform(-3.0, 0.7, nz)
    w0 = rng.uniform(0.05, 0.98, nz)
    g = rng.uniform(-0.6, 0.9, nz)
    if nz == 1:
        if variant == 0:
            w0[0], g[0] = W0_CAP, -0.4
        elif variant == 1:
            tau[0] = THIN
        else:
            tau[0], w0[0] = THICK, 0.0
    elif nz == 3:
        if variant == 0:
            w0[0] = 0.0
            w0[1], g[1] = W0_CAP, -0.4
            tau[2] = THICK
        else:
            tau[0], tau[1] = THIN, ABOVE
            g[2] = -0.5
    else:
        w0[2] = 0.0
        tau[5], tau[6] = THIN, ABOVE
        w0[nz // 2], g[nz // 2] = W0_CAP, -0.35
        tau[nz - 3] = THICK
    k = np.arange(nz + 1) / nz
    bp = 1.0 + 3.0 * k ** 1.5 + 0.02 * rng.uniform(-1.0, 1.0, nz + 1)
    return tau, w0, g, bp


CASES = [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (33, 0), (65, 0)]      # (nz, variant), each at both surface forms


def case(nz, variant, hard, with_ref=True):
    tau, w0, g, bp = column(nz, variant)
    lv = levels_of(nz)
    ex = X.exact_opr_sens(tau, w0, g, EMISSIVITY, hard, TAU_MIN, bp, lv)
    out = dict(tau=tau, w0=w0, g=g, bplanck=bp, ir_par=np.array([EMISSIVITY, 1.0 if hard else 0.0, TAU_MIN]),
               levels=np.array(lv, dtype=np.int32))
    out.update(ex)
    if with_ref:
        rs = X.restated_opr_sens(tau, w0, g, EMISSIVITY, hard, TAU_MIN, bp, lv)
        assert all(np.all(np.isfinite(rs[k])) for k in X.NAMES), "the restatement is not finite: no yardstick"
        out["e_ref"] = np.array([np.max(np.abs(rs[k] - ex[k])) for k in X.NAMES])
    return out


def main():
    out, n = {}, 0
    for nz, variant in CASES:
        for hard in (True, False):
            c = case(nz, variant, hard)
            for k, v in c.items():
                out["s%02d_%s" % (n, k)] = v
            sc = [np.max(np.abs(c[k])) for k in X.NAMES]
            print("s%02d nz %d variant %d hard %d: e_ref / scale %s" % (n, nz, variant, hard, " ".join(
                "%s %.1e" % (k, e / s if s else 0.0) for k, e, s in zip(X.NAMES, c["e_ref"], sc))), flush=True)
            n += 1
    out["n"] = np.array([n])
    path = os.path.join(HERE, "exact_ir_opr_sens_0.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d columns, %d bytes" % (path, n, os.path.getsize(path)))


if __name__ == "__main__":
    main()
