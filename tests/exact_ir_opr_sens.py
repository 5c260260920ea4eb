"""Exact derivatives of two_stream_ir's level fluxes in a layer's tau, w0 and g, and the reference ALGORITHM's own error on
them.  A helper of the tests, not a test.  It shares nothing with oracle/ and nothing with the kernel's formulas.

  exact_opr_sens(tau, w0, g, emissivity, hard, tau_min, bplanck, levels) -> {"up_tau", "up_w0", "up_g", "dn_tau", "dn_w0",
      "dn_g"}: (nrow, nz) each, [a, n] = d fup (fdn) (levels[a]) / d tau(n) ..., levels and layers TOA-first

`IrColumn` (exact_two_stream.py) rounds its inputs to float64 through `_x`, so it cannot be stepped by 1e-30;
`IrColumnMp` takes mpmath numbers as they are (the thin branch of a layer is decided by the caller: a step of 1e-30 must
not move a layer across `tau_min`).  The derivative is the central difference with h = 1e-30 at 80 digits -- truncation
h^2 f''' / 6 is 1e-60 times the third derivative, far below one rounding even next to w0 = 1 -- rounded once.
`opr_sens_mp` returns the mpmath numbers themselves for sums that are made before rounding (the whole-call test).

  restated_opr_sens(...same arguments...) -> the same dict from the float64 RESTATEMENT of two_stream_ir
      (src/radtran/clima_radtran_twostream.f90:156-295, its formulas in its order, torch on the CPU, a dense solve of the
      2nz-row system) differentiated by autograd: what the reference algorithm's derivative is in float64.  Its distance
      from exact is e_ref of the criterion  kernel error <= max(FLOOR x scale, 10 x e_ref)  (exact_two_stream_cases.py).
"""
import mpmath
import numpy as np

from exact_two_stream import IrColumn

DPS = 80
H = "1e-30"
NAMES = ("up_tau", "up_w0", "up_g", "dn_tau", "dn_w0", "dn_g")


class IrColumnMp(IrColumn):
    """IrColumn on mpmath inputs; `thin[i]`: layer i takes the tau <= tau_min branch.  Use inside `mpmath.workdps`."""

    def __init__(self, tau, w0, g, emissivity, hard, thin):
        nz = len(tau)
        self.tau = [mpmath.mpf(t) for t in tau]
        # (solve_mp decides the branch as tau_f <= tau_min: 0 <= 1 for a thin layer, 2 <= 1 for the others)
        self.tau_f = [0.0 if t else 2.0 for t in thin]
        self.hard, self.tau_min = bool(hard), 1.0
        self.em = mpmath.mpf(emissivity)
        self.Rsfc = 1 - self.em if self.hard else mpmath.mpf(0)
        w, gt = [mpmath.mpf(v) for v in w0], [mpmath.mpf(v) for v in g]
        gam1 = [2 - w[i] * (1 + gt[i]) for i in range(nz)]
        gam2 = [w[i] * (1 - gt[i]) for i in range(nz)]
        lam = [mpmath.sqrt(gam1[i] * gam1[i] - gam2[i] * gam2[i]) for i in range(nz)]
        cap = [gam2[i] / (gam1[i] + lam[i]) for i in range(nz)]
        self.rq = [1 / (gam1[i] + gam2[i]) for i in range(nz)]
        self._matrix(lam, cap, self.tau)


def opr_sens_mp(tau, w0, g, emissivity, hard, tau_min, bplanck, levels):
    """-> {name: [[mpf] * nz] * nrow}; float64 inputs taken as the exact numbers they are.  Use inside `mpmath.workdps`."""
    nz = len(tau)
    x = [[mpmath.mpf(float(v)) for v in a] for a in (tau, w0, g)]
    thin = [float(t) <= float(tau_min) for t in tau]
    bp = [b if isinstance(b, mpmath.mpf) else mpmath.mpf(float(b)) for b in bplanck]      # (mpmath Planck values as they are)
    em, h = mpmath.mpf(float(emissivity)), mpmath.mpf(H)
    out = {name: [[None] * nz for _ in levels] for name in NAMES}
    for p, pname in enumerate(("tau", "w0", "g")):
        for n in range(nz):
            f = []
            for s in (1, -1):
                y = [list(a) for a in x]
                y[p][n] = y[p][n] + s * h
                f.append(IrColumnMp(y[0], y[1], y[2], em, hard, thin).solve_mp(bp))
            for a, lv in enumerate(levels):
                out["up_" + pname][a][n] = (f[0][0][lv] - f[1][0][lv]) / (2 * h)
                out["dn_" + pname][a][n] = (f[0][1][lv] - f[1][1][lv]) / (2 * h)
    return out


def exact_opr_sens(tau, w0, g, emissivity, hard, tau_min, bplanck, levels, dps=DPS):
    with mpmath.workdps(dps):
        d = opr_sens_mp(tau, w0, g, emissivity, hard, tau_min, bplanck, levels)
        return {k: np.array([[float(v) for v in row] for row in rows], dtype=np.float64) for k, rows in d.items()}


def restated_opr_sens(tau, w0, g, emissivity, hard, tau_min, bplanck, levels):
    """two_stream_ir restated in float64 (torch, CPU), in the reference's order, a dense solve; autograd per (level, direction)"""
    import torch
    nz = len(tau)
    f64 = torch.float64
    t = torch.tensor(np.asarray(tau, dtype=np.float64), dtype=f64, requires_grad=True)
    w = torch.tensor(np.asarray(w0, dtype=np.float64), dtype=f64, requires_grad=True)
    gt = torch.tensor(np.asarray(g, dtype=np.float64), dtype=f64, requires_grad=True)
    bp = torch.tensor(np.asarray(bplanck, dtype=np.float64), dtype=f64)
    pi = float(np.pi)
    u1 = 0.5
    norm = 2.0 * pi * u1
    Rsfc = 1.0 - float(emissivity) if hard else 0.0
    gam1 = 2.0 - w * (1.0 + gt)                                                           # :195-201
    gam2 = w * (1.0 - gt)
    lam = torch.sqrt(gam1 ** 2.0 - gam2 ** 2.0)
    cap = gam2 / (gam1 + lam)
    wrk = torch.exp(-lam * t)                                                             # :205-211
    e1, e2, e3, e4 = 1.0 + cap * wrk, 1.0 - cap * wrk, cap + wrk, cap - wrk
    thin = torch.tensor([float(v) <= float(tau_min) for v in tau])
    tsafe = torch.where(thin, torch.ones_like(t), t)
    b0n = torch.where(thin, 0.5 * (bp[:-1] + bp[1:]), bp[:-1])                            # :215-227
    b1n = torch.where(thin, torch.zeros_like(t), (bp[1:] - bp[:-1]) / tsafe)
    rq = 1.0 / (gam1 + gam2)
    cp0 = norm * (b0n + b1n * rq)                                                         # :229-232
    cpb = norm * (b0n + b1n * (t + rq))
    cm0 = norm * (b0n + b1n * (-rq))
    cmb = norm * (b0n + b1n * (t - rq))
    if hard:                                                                              # :236-247
        Ssfc = float(emissivity) * pi * bp[nz]
    else:
        b1_bot = torch.zeros((), dtype=f64) if bool(thin[nz - 1]) else (bp[nz] - bp[nz - 1]) / t[nz - 1]
        Ssfc = pi * (bp[nz] + u1 * b1_bot)
    N = 2 * nz
    rows = [[None] * 3 for _ in range(N)]      # (A, B, D) and E per row, 0-based l - 1 of :251-275
    E = [None] * N
    zero = torch.zeros((), dtype=f64)
    rows[0] = [zero, e1[0], -e2[0]]
    E[0] = 0.0 - cm0[0]
    for i in range(nz - 1):
        l = 2 * i + 2
        rows[l] = [e2[i] * e3[i] - e4[i] * e1[i], e1[i] * e1[i + 1] - e3[i] * e3[i + 1], e3[i] * e4[i + 1] - e1[i] * e2[i + 1]]
        E[l] = e3[i] * (cp0[i + 1] - cpb[i]) + e1[i] * (cmb[i] - cm0[i + 1])
        l = 2 * i + 1
        rows[l] = [e2[i + 1] * e1[i] - e3[i] * e4[i + 1], e2[i] * e2[i + 1] - e4[i] * e4[i + 1], e1[i + 1] * e4[i + 1] - e2[i + 1] * e3[i + 1]]
        E[l] = e2[i + 1] * (cp0[i + 1] - cpb[i]) - e4[i + 1] * (cm0[i + 1] - cmb[i])
    rows[N - 1] = [e1[nz - 1] - Rsfc * e3[nz - 1], e2[nz - 1] - Rsfc * e4[nz - 1], zero]
    E[N - 1] = Ssfc - cpb[nz - 1] + Rsfc * cmb[nz - 1]
    M = torch.zeros((N, N), dtype=f64)
    idx_r, idx_c, vals = [], [], []
    for r in range(N):
        for d, v in zip((-1, 0, 1), rows[r]):
            if 0 <= r + d < N:
                idx_r.append(r); idx_c.append(r + d); vals.append(v)
    M = M.index_put((torch.tensor(idx_r), torch.tensor(idx_c)), torch.stack(vals))
    Y = torch.linalg.solve(M, torch.stack(E))
    y1, y2 = Y[0::2], Y[1::2]
    fup = torch.cat([(y1[0] * e3[0] - y2[0] * e4[0] + cp0[0]).reshape(1), y1 * e1 + y2 * e2 + cpb])    # :288-293
    fdn = torch.cat([torch.zeros(1, dtype=f64), y1 * e3 + y2 * e4 + cmb])
    out = {name: np.zeros((len(levels), nz)) for name in NAMES}
    for a, lv in enumerate(levels):
        for d, f in (("up", fup), ("dn", fdn)):
            gr = torch.autograd.grad(f[lv], (t, w, gt), retain_graph=True, allow_unused=True)
            for pname, v in zip(("tau", "w0", "g"), gr):
                if v is not None:
                    out["%s_%s" % (d, pname)][a] = v.numpy()
    return out
