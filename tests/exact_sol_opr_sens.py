"""Exact derivatives of two_stream_solar's level values (fup, fdn, amean, summed over the zenith angles with their weights)
in a layer's tau, w0 and g and in the surface reflectance, and the reference ALGORITHM's own error on them.  A helper of
the tests, not a test.  It shares nothing with oracle/ and nothing with the kernel's formulas.

  exact_sol_opr_sens(tau, w0, g, zen_u, zen_w, Rsfc, levels) -> {"up_tau", "up_w0", "up_g", "up_rsfc", "dn_...", "am_..."}:
      (nrow, nz) each, [a, n] = d fup (fdn, amean) (levels[a]) / d tau(n) ..., and (nrow,) for rsfc; levels and layers
      TOA-first

`SolarColumn` (exact_two_stream.py) rounds its inputs to float64 through `_x`, so it cannot be stepped by 1e-30;
`SolarColumnMp` takes mpmath numbers as they are.  The derivative is the central difference with h = 1e-30 at 80 digits --
truncation h^2 f''' / 6 is 1e-60 times the third derivative, far below one rounding even next to w0 = 1 or lambda u0 = 1
-- of the sum over the zenith angles, rounded once.  `sol_opr_sens_mp` returns the mpmath numbers themselves for sums that
are made before rounding (the whole-call test).

  restated_sol_opr_sens(...same arguments...) -> the same dict from the float64 RESTATEMENT of two_stream_solar
      (src/radtran/clima_radtran_twostream.f90:10-154, its formulas in its order, torch on the CPU, a dense solve of the
      2nz-row system per zenith angle) differentiated by autograd: what the reference algorithm's derivative is in float64.
      Its distance from exact is e_ref of the criterion  kernel error <= max(FLOOR x scale, 10 x e_ref)
      (exact_two_stream_cases.py).
"""
import mpmath
import numpy as np

from exact_two_stream import SolarColumn

DPS = 80
H = "1e-30"
QUANTITIES = ("up", "dn", "am")
PARAMS = ("tau", "w0", "g", "rsfc")
NAMES = tuple("%s_%s" % (q, p) for q in QUANTITIES for p in PARAMS)


class SolarColumnMp(SolarColumn):
    """SolarColumn on mpmath inputs (u0 and Rsfc of `solve_mp` too).  Use inside `mpmath.workdps`."""

    def __init__(self, tau, w0, g):
        nz = len(tau)
        s3 = self.s3 = mpmath.sqrt(3)
        ti, wi, gi = [mpmath.mpf(v) for v in tau], [mpmath.mpf(v) for v in w0], [mpmath.mpf(v) for v in g]
        self.tau = [ti[i] * (1 - wi[i] * gi[i] * gi[i]) for i in range(nz)]              # :38-40
        self.w0 = [wi[i] * (1 - gi[i] * gi[i]) / (1 - wi[i] * gi[i] * gi[i]) for i in range(nz)]
        self.gt = [gi[i] / (1 + gi[i]) for i in range(nz)]
        self.gam1 = [s3 * (2 - self.w0[i] * (1 + self.gt[i])) / 2 for i in range(nz)]
        self.gam2 = [s3 * self.w0[i] * (1 - self.gt[i]) / 2 for i in range(nz)]
        self.lam = [mpmath.sqrt(self.gam1[i] ** 2 - self.gam2[i] ** 2) for i in range(nz)]
        cap = [self.gam2[i] / (self.gam1[i] + self.lam[i]) for i in range(nz)]
        self.tauc = [mpmath.mpf(0)]
        for i in range(nz):
            self.tauc.append(self.tauc[i] + self.tau[i])
        self._matrix(self.lam, cap, self.tau)

    def solve_mp(self, u0, Rsfc):
        """-> amean, fup, fdn (mpmath); u0 and Rsfc are mpmath numbers, taken as they are"""
        nz, s3 = self.nz, self.s3
        iu = 1 / u0
        direct = [u0 * mpmath.exp(-t * iu) for t in self.tauc]
        cp0, cpb, cm0, cmb = [], [], [], []
        for i in range(nz):                                                              # :73-87
            gam1, gam2, w = self.gam1[i], self.gam2[i], self.w0[i]
            gam3 = (1 - s3 * self.gt[i] * u0) / 2
            gam4 = 1 - gam3
            facp = w * ((gam1 - iu) * gam3 + gam4 * gam2)
            facm = w * ((gam1 + iu) * gam4 + gam2 * gam3)
            denom = self.lam[i] ** 2 - iu * iu
            et0, etb = direct[i] * iu, direct[i + 1] * iu
            cp0.append(et0 * facp / denom)
            cpb.append(etb * facp / denom)
            cm0.append(et0 * facm / denom)
            cmb.append(etb * facm / denom)
        Ssfc = Rsfc * direct[nz]                                                         # :89
        y1, y2 = self._solve(cp0, cpb, cm0, cmb, Rsfc, Ssfc)
        fup, fdn = self._fluxes(y1, y2, cp0, cpb, cmb, Rsfc, Ssfc)
        amean = [s3 * fup[0] + direct[0] * iu]                                           # :135-148
        for i in range(nz):
            amean.append(s3 * (fup[i + 1] + fdn[i + 1]) + direct[i + 1] * iu)
        fdn = [fdn[i] + direct[i] for i in range(nz + 1)]
        return amean, fup, fdn


def solar_sum_mp(tau, w0, g, zen_u, zen_w, Rsfc):
    """sum_z w_z two_stream_solar(u0_z) on mpmath inputs -> (fup, fdn, amean), lists of mpmath numbers"""
    col = SolarColumnMp(tau, w0, g)
    acc = None
    for u, w in zip(zen_u, zen_w):
        am, fu, fd = col.solve_mp(u, Rsfc)
        one = (fu, fd, am)
        acc = [[w * v for v in a] for a in one] if acc is None else [[s + w * v for s, v in zip(sa, a)] for sa, a in zip(acc, one)]
    return acc


def sol_opr_sens_mp(tau, w0, g, zen_u, zen_w, Rsfc, levels):
    """-> {name: [[mpf] * nz] * nrow, or [mpf] * nrow for rsfc}; float64 inputs taken as the exact numbers they are.  Use
    inside `mpmath.workdps`."""
    nz = len(tau)
    x = [[mpmath.mpf(float(v)) for v in a] for a in (tau, w0, g)]
    zu, zw = [mpmath.mpf(float(v)) for v in zen_u], [mpmath.mpf(float(v)) for v in zen_w]
    R, h = mpmath.mpf(float(Rsfc)), mpmath.mpf(H)
    out = {}
    for q in QUANTITIES:
        for p in ("tau", "w0", "g"):
            out["%s_%s" % (q, p)] = [[None] * nz for _ in levels]
        out[q + "_rsfc"] = [None] * len(levels)
    for p, pname in enumerate(("tau", "w0", "g")):
        for n in range(nz):
            f = []
            for s in (1, -1):
                y = [list(a) for a in x]
                y[p][n] = y[p][n] + s * h
                f.append(solar_sum_mp(y[0], y[1], y[2], zu, zw, R))
            for a, lv in enumerate(levels):
                for k, q in enumerate(QUANTITIES):
                    out["%s_%s" % (q, pname)][a][n] = (f[0][k][lv] - f[1][k][lv]) / (2 * h)
    f = [solar_sum_mp(x[0], x[1], x[2], zu, zw, R + s * h) for s in (1, -1)]
    for a, lv in enumerate(levels):
        for k, q in enumerate(QUANTITIES):
            out[q + "_rsfc"][a] = (f[0][k][lv] - f[1][k][lv]) / (2 * h)
    return out


def _to_float(v):
    if isinstance(v, list):
        return [_to_float(a) for a in v]
    return float(v)


def exact_sol_opr_sens(tau, w0, g, zen_u, zen_w, Rsfc, levels, dps=DPS):
    with mpmath.workdps(dps):
        d = sol_opr_sens_mp(tau, w0, g, zen_u, zen_w, Rsfc, levels)
        return {k: np.array(_to_float(v), dtype=np.float64) for k, v in d.items()}


def restated_solar(tau, w0, g, zen_u, zen_w, Rsfc):
    """two_stream_solar restated in float64 (torch, CPU), in the reference's order, a dense solve per zenith angle, the
    angles summed with their weights -> (fup, fdn, amean) torch vectors (nz+1, TOA-first) and the leaves (tau, w0, g, Rsfc)"""
    import torch
    nz = len(tau)
    f64 = torch.float64
    t_in = torch.tensor(np.asarray(tau, dtype=np.float64), dtype=f64, requires_grad=True)
    w_in = torch.tensor(np.asarray(w0, dtype=np.float64), dtype=f64, requires_grad=True)
    g_in = torch.tensor(np.asarray(g, dtype=np.float64), dtype=f64, requires_grad=True)
    R = torch.tensor(float(Rsfc), dtype=f64, requires_grad=True)
    s3 = float(np.sqrt(3.0))
    u1 = 1.0 / s3
    t = t_in * (1.0 - w_in * g_in * g_in)                                                # :38-40
    w = w_in * (1.0 - g_in * g_in) / (1.0 - w_in * g_in * g_in)
    gt = g_in / (1.0 + g_in)
    gam1 = s3 * (2.0 - w * (1 + gt)) / 2.0                                               # :43-44
    gam2 = s3 * w * (1.0 - gt) / 2.0
    lam = torch.sqrt(gam1 ** 2.0 - gam2 ** 2.0)                                          # :50-51
    cap = gam2 / (gam1 + lam)
    wrk = torch.exp(-lam * t)                                                            # :55-61
    e1, e2, e3, e4 = 1.0 + cap * wrk, 1.0 - cap * wrk, cap + wrk, cap - wrk
    tauc = torch.cat([torch.zeros(1, dtype=f64), torch.cumsum(t, 0)])                    # :64-67
    N = 2 * nz
    zero = torch.zeros((), dtype=f64)
    rows = [None] * N
    rows[0] = [zero, e1[0], -e2[0]]
    for i in range(nz - 1):
        l = 2 * i + 2
        rows[l] = [e2[i] * e3[i] - e4[i] * e1[i], e1[i] * e1[i + 1] - e3[i] * e3[i + 1], e3[i] * e4[i + 1] - e1[i] * e2[i + 1]]
        l = 2 * i + 1
        rows[l] = [e2[i + 1] * e1[i] - e3[i] * e4[i + 1], e2[i] * e2[i + 1] - e4[i] * e4[i + 1], e1[i + 1] * e4[i + 1] - e2[i + 1] * e3[i + 1]]
    rows[N - 1] = [e1[nz - 1] - R * e3[nz - 1], e2[nz - 1] - R * e4[nz - 1], zero]
    idx_r, idx_c, vals = [], [], []
    for r in range(N):
        for d, v in zip((-1, 0, 1), rows[r]):
            if 0 <= r + d < N:
                idx_r.append(r); idx_c.append(r + d); vals.append(v)
    M = torch.zeros((N, N), dtype=f64).index_put((torch.tensor(idx_r), torch.tensor(idx_c)), torch.stack(vals))
    fup_s = fdn_s = am_s = None
    for u0, wz in zip(zen_u, zen_w):
        u0, wz = float(u0), float(wz)
        gam3 = (1.0 - s3 * gt * u0) / 2.0                                                # :45-46
        gam4 = 1.0 - gam3
        facp = w * ((gam1 - 1.0 / u0) * gam3 + gam4 * gam2)                              # :76-80
        facm = w * ((gam1 + 1.0 / u0) * gam4 + gam2 * gam3)
        et0 = torch.exp(-tauc[:-1] / u0)
        etb = et0 * torch.exp(-t / u0)
        denom = lam ** 2.0 - 1.0 / (u0 ** 2.0)
        direct = torch.cat([torch.full((1,), u0, dtype=f64), u0 * etb])                  # :73, :82
        cp0, cpb, cm0, cmb = et0 * facp / denom, etb * facp / denom, et0 * facm / denom, etb * facm / denom
        Ssfc = R * direct[nz]                                                            # :89
        E = [None] * N
        E[0] = 0.0 - cm0[0]
        for i in range(nz - 1):
            E[2 * i + 2] = e3[i] * (cp0[i + 1] - cpb[i]) + e1[i] * (cmb[i] - cm0[i + 1])
            E[2 * i + 1] = e2[i + 1] * (cp0[i + 1] - cpb[i]) - e4[i + 1] * (cm0[i + 1] - cmb[i])
        E[N - 1] = Ssfc - cpb[nz - 1] + R * cmb[nz - 1]
        Y = torch.linalg.solve(M, torch.stack(E))
        y1, y2 = Y[0::2], Y[1::2]
        top = y1[0] * e3[0] - y2[0] * e4[0] + cp0[0]
        fup = torch.cat([top.reshape(1), y1 * e1 + y2 * e2 + cpb])                       # :143-148
        fdn = torch.cat([direct[0].reshape(1), (y1 * e3 + y2 * e4 + cmb) + direct[1:]])
        am = torch.cat([((1.0 / u1) * top + direct[0] / u0).reshape(1),                  # :135-140
                        (1.0 / u1) * (y1 * (e1 + e3) + y2 * (e2 + e4) + cpb + cmb) + direct[1:] / u0])
        fup_s = wz * fup if fup_s is None else fup_s + wz * fup
        fdn_s = wz * fdn if fdn_s is None else fdn_s + wz * fdn
        am_s = wz * am if am_s is None else am_s + wz * am
    return (fup_s, fdn_s, am_s), (t_in, w_in, g_in, R)


def restated_sol_opr_sens(tau, w0, g, zen_u, zen_w, Rsfc, levels):
    """the restatement's derivatives by autograd, per (level, quantity) -> the dict of exact_sol_opr_sens"""
    import torch
    nz = len(tau)
    fs, leaves = restated_solar(tau, w0, g, zen_u, zen_w, Rsfc)
    out = {}
    for q in QUANTITIES:
        for p in ("tau", "w0", "g"):
            out["%s_%s" % (q, p)] = np.zeros((len(levels), nz))
        out[q + "_rsfc"] = np.zeros(len(levels))
    for a, lv in enumerate(levels):
        for q, f in zip(QUANTITIES, fs):
            if not f[lv].requires_grad:
                continue
            gr = torch.autograd.grad(f[lv], leaves, retain_graph=True, allow_unused=True)
            for pname, v in zip(PARAMS, gr):
                if v is not None:
                    out["%s_%s" % (q, pname)][a] = v.numpy()
    return out
