"""The two-stream solvers in `mpmath` arithmetic: the solution of the SYSTEM, not another double rounding of it.
A helper of the tests, not a test.  It shares nothing with oracle/ (no import of it, no call into its libraries).

What is restated is the system that oracle/clima_oracle.c:247-416 states (clima_radtran_twostream.f90:10-316):
the delta scaling of the solar call (:38-40), gam1 / gam2 / gam3 / gam4, lambda and Gamma, e1...e4, the IR source with
its `tau <= tau_min` branch, the solar source terms over lambda^2 - 1/u0^2, both surface terms, the 2nz-row
tridiagonal system of `assemble` and the elimination of `tridiag` (in exact arithmetic its order does not matter).
Float64 inputs are taken as the exact numbers they are, `exp` and `sqrt` are mpmath's at `dps` digits (50 by default),
and every output is rounded once, to the nearest float64.  (An output that the mathematics makes 0, or 1e-30 of its
neighbours and less, carries the residual of the solve instead: 1e-50 of the largest output, not its own last bit.)

  exact_ir(tau, w0, g, emissivity, hard, tau_min, bplanck)   -> fup, fdn            (nz+1 each, TOA-first)
  exact_solar(tau, w0, g, u0, Rsfc)                          -> amean, fup, fdn
  exact_unit_responses(tau, w0, g, emissivity, hard, tau_min) -> up, dn [level, k] = d f(level) / d bplanck(k)
  exact_ir_response(..., devs)                               -> up, dn [dev, level]: the change for each (k, dB)
  exact_solar_sum(tau, w0, g, zen_u, zen_w, Rsfc)            -> sum_z w_z exact_solar(u0_z)

The IR fluxes are linear in the Planck values, so the nz+1 unit-vector solves give the derivative exactly; one
factorisation of the matrix serves every right-hand side (`IrColumn`), and the solar matrix does not depend on u0
(`SolarColumn`).  The `_mp` methods return mpmath numbers for the checks that are made before rounding.

`mpmath` is used in two ways.  The column-by-column GPU tests (test_gpu_exact_two_stream.py) read what the generator
tests/golden/make_exact_two_stream.py stored.  The whole-call tests run it live: `closed_forms.radiate_exact` builds one
`IrColumn` / `SolarColumn` per (bin, g-point) of a small case and keeps every sum over g-points, zenith angles and bins in
mpmath (test_closed_forms_host.py without a GPU, test_gpu_closed_forms.py with one; 0.2-2.5 s per case).
"""
import mpmath
import numpy as np

DPS = 50


def _x(v):
    """a float64 as the exact number it is"""
    return mpmath.mpf(float(v))


def _round(v):
    return np.array([float(a) for a in v], dtype=np.float64)


class _Tridiag:
    """tridiag (:297-316) with the forward elimination of the matrix kept, for any number of right-hand sides.  The last
    row (the surface's) may be replaced per solve: it is the only one that holds Rsfc."""

    def __init__(self, A, B, D):
        n = len(B)
        self.n, self.A = n, A
        self.inv, self.c = [None] * n, [None] * n
        self.inv[0] = 1 / B[0]
        self.c[0] = D[0] * self.inv[0]
        for i in range(1, n - 1):
            self.inv[i] = 1 / (B[i] - A[i] * self.c[i - 1])
            self.c[i] = D[i] * self.inv[i]

    def solve(self, E, a_last, b_last):
        n, A, inv, c = self.n, self.A, self.inv, self.c
        d = [None] * n
        d[0] = E[0] * inv[0]
        for i in range(1, n - 1):
            d[i] = (E[i] - A[i] * d[i - 1]) * inv[i]
        d[n - 1] = (E[n - 1] - a_last * d[n - 2]) / (b_last - a_last * c[n - 2])
        for i in range(n - 2, -1, -1):
            d[i] = d[i] - c[i] * d[i + 1]
        return d


class _Column:
    """What the two solvers share once lambda, Gamma and the layer's optical depth are known: e1...e4, the matrix of
    `assemble` and the fluxes from the solution."""

    def _matrix(self, lam, cap, tau):
        nz = self.nz = len(tau)
        one = mpmath.mpf(1)
        wrk = [mpmath.exp(-lam[i] * tau[i]) for i in range(nz)]
        e1 = self.e1 = [one + cap[i] * wrk[i] for i in range(nz)]
        e2 = self.e2 = [one - cap[i] * wrk[i] for i in range(nz)]
        e3 = self.e3 = [cap[i] + wrk[i] for i in range(nz)]
        e4 = self.e4 = [cap[i] - wrk[i] for i in range(nz)]
        n = 2 * nz
        A, B, D = [mpmath.mpf(0)] * n, [None] * n, [mpmath.mpf(0)] * n
        B[0], D[0] = e1[0], -e2[0]
        for i in range(nz - 1):
            l = 2 * i + 2
            A[l] = e2[i] * e3[i] - e4[i] * e1[i]
            B[l] = e1[i] * e1[i + 1] - e3[i] * e3[i + 1]
            D[l] = e3[i] * e4[i + 1] - e1[i] * e2[i + 1]
            l = 2 * i + 1
            A[l] = e2[i + 1] * e1[i] - e3[i] * e4[i + 1]
            B[l] = e2[i] * e2[i + 1] - e4[i] * e4[i + 1]
            D[l] = e1[i + 1] * e4[i + 1] - e2[i + 1] * e3[i + 1]
        B[n - 1] = one          # replaced per solve
        self.tri = _Tridiag(A, B, D)

    def _solve(self, cp0, cpb, cm0, cmb, Rsfc, Ssfc):
        """-> y1, y2 (nz each)"""
        nz, e1, e2, e3, e4 = self.nz, self.e1, self.e2, self.e3, self.e4
        E = [None] * (2 * nz)
        E[0] = -cm0[0]
        for i in range(nz - 1):
            E[2 * i + 2] = e3[i] * (cp0[i + 1] - cpb[i]) + e1[i] * (cmb[i] - cm0[i + 1])
            E[2 * i + 1] = e2[i + 1] * (cp0[i + 1] - cpb[i]) - e4[i + 1] * (cm0[i + 1] - cmb[i])
        E[2 * nz - 1] = Ssfc - cpb[nz - 1] + Rsfc * cmb[nz - 1]
        y = self.tri.solve(E, e1[nz - 1] - Rsfc * e3[nz - 1], e2[nz - 1] - Rsfc * e4[nz - 1])
        return y[0::2], y[1::2]

    def _fluxes(self, y1, y2, cp0, cpb, cmb, Rsfc, Ssfc):
        """-> the diffuse fup, fdn (nz+1 each; fdn[0] is the caller's).  The upward flux at the surface is taken from the
        surface row of the system, fup = Rsfc fdn + Ssfc, which is what y1 e1 + y2 e2 + C+ equals there: formed this way
        a reflected flux that is exactly 0 (Rsfc = 0) comes out 0, not as the residual of the 50-digit solve."""
        nz, e1, e2, e3, e4 = self.nz, self.e1, self.e2, self.e3, self.e4
        fup = [y1[0] * e3[0] - y2[0] * e4[0] + cp0[0]]
        fdn = [mpmath.mpf(0)]
        for i in range(nz):
            fup.append(y1[i] * e1[i] + y2[i] * e2[i] + cpb[i])
            fdn.append(y1[i] * e3[i] + y2[i] * e4[i] + cmb[i])
        fup[nz] = Rsfc * fdn[nz] + Ssfc
        return fup, fdn


class IrColumn(_Column):
    """two_stream_ir (:156-295) of one column; use inside `mpmath.workdps`."""

    def __init__(self, tau, w0, g, emissivity, hard, tau_min):
        nz = len(tau)
        self.tau_f = [float(t) for t in tau]
        self.tau = [_x(t) for t in tau]
        self.hard, self.tau_min = bool(hard), float(tau_min)
        self.em = _x(emissivity)
        self.Rsfc = 1 - self.em if self.hard else mpmath.mpf(0)                         # :186-190
        w, gt = [_x(v) for v in w0], [_x(v) for v in g]
        gam1 = [2 - w[i] * (1 + gt[i]) for i in range(nz)]                               # :195-201
        gam2 = [w[i] * (1 - gt[i]) for i in range(nz)]
        lam = [mpmath.sqrt(gam1[i] * gam1[i] - gam2[i] * gam2[i]) for i in range(nz)]
        cap = [gam2[i] / (gam1[i] + lam[i]) for i in range(nz)]
        self.rq = [1 / (gam1[i] + gam2[i]) for i in range(nz)]
        self._matrix(lam, cap, self.tau)

    def solve_mp(self, bplanck):
        """bplanck: nz+1 mpmath numbers -> fup, fdn (mpmath)"""
        nz, tau, rq = self.nz, self.tau, self.rq
        pi = mpmath.pi                                                                   # norm = 2 pi u1, u1 = 1/2
        cp0, cpb, cm0, cmb = [], [], [], []
        for i in range(nz):                                                              # :215-234
            if self.tau_f[i] <= self.tau_min:
                b0, b1 = (bplanck[i] + bplanck[i + 1]) / 2, mpmath.mpf(0)
            else:
                b0, b1 = bplanck[i], (bplanck[i + 1] - bplanck[i]) / tau[i]
            cp0.append(pi * (b0 + b1 * rq[i]))
            cpb.append(pi * (b0 + b1 * (tau[i] + rq[i])))
            cm0.append(pi * (b0 - b1 * rq[i]))
            cmb.append(pi * (b0 + b1 * (tau[i] - rq[i])))
        if self.hard:                                                                    # :236-247
            Ssfc = self.em * pi * bplanck[nz]
        else:
            b1_bot = mpmath.mpf(0) if self.tau_f[nz - 1] <= self.tau_min else (bplanck[nz] - bplanck[nz - 1]) / tau[nz - 1]
            Ssfc = pi * (bplanck[nz] + b1_bot / 2)
        y1, y2 = self._solve(cp0, cpb, cm0, cmb, self.Rsfc, Ssfc)
        return self._fluxes(y1, y2, cp0, cpb, cmb, self.Rsfc, Ssfc)

    def unit_mp(self, k):
        e = [mpmath.mpf(0)] * (self.nz + 1)
        e[k] = mpmath.mpf(1)
        return self.solve_mp(e)


class SolarColumn(_Column):
    """two_stream_solar (:10-154) of one column; the matrix serves every u0; use inside `mpmath.workdps`."""

    def __init__(self, tau, w0, g):
        nz = len(tau)
        s3 = self.s3 = mpmath.sqrt(3)
        ti, wi, gi = [_x(v) for v in tau], [_x(v) for v in w0], [_x(v) for v in g]
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
        """-> amean, fup, fdn (mpmath)"""
        nz, s3 = self.nz, self.s3
        u0, Rsfc = _x(u0), _x(Rsfc)
        iu = 1 / u0
        direct = [u0 * mpmath.exp(-t * iu) for t in self.tauc]                           # Fs_pi = 1
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
        y1, y2 = self._solve(cp0, cpb, cm0, cmb, Rsfc, Rsfc * direct[nz])               # :89
        fup, fdn = self._fluxes(y1, y2, cp0, cpb, cmb, Rsfc, Rsfc * direct[nz])
        amean = [s3 * fup[0] + direct[0] * iu]                                           # :135-148, 1/u1 = sqrt(3)
        for i in range(nz):
            amean.append(s3 * (fup[i + 1] + fdn[i + 1]) + direct[i + 1] * iu)
        fdn = [fdn[i] + direct[i] for i in range(nz + 1)]
        return amean, fup, fdn


def exact_ir(tau, w0, g, emissivity, hard, tau_min, bplanck, dps=DPS):
    with mpmath.workdps(dps):
        fup, fdn = IrColumn(tau, w0, g, emissivity, hard, tau_min).solve_mp([_x(b) for b in bplanck])
        return _round(fup), _round(fdn)


def exact_solar(tau, w0, g, u0, Rsfc, dps=DPS):
    with mpmath.workdps(dps):
        return tuple(_round(a) for a in SolarColumn(tau, w0, g).solve_mp(u0, Rsfc))


def exact_unit_responses(tau, w0, g, emissivity, hard, tau_min, dps=DPS, ks=None):
    """up, dn [level, k], TOA-first: d fup(level) / d bplanck(k) and d fdn(level) / d bplanck(k) of one column, from the
    unit-vector solves (all nz+1, or the columns `ks` alone: the others stay 0)."""
    nl = len(tau) + 1
    up, dn = np.zeros((nl, nl)), np.zeros((nl, nl))
    with mpmath.workdps(dps):
        col = IrColumn(tau, w0, g, emissivity, hard, tau_min)
        for k in (range(nl) if ks is None else ks):
            fu, fd = col.unit_mp(k)
            up[:, k], dn[:, k] = _round(fu), _round(fd)
    return up, dn


def exact_ir_response(tau, w0, g, emissivity, hard, tau_min, devs, dps=DPS):
    """devs: [(k, dB)] -> up, dn [dev, level]: the change of the level fluxes when bplanck(k) changes by dB, each
    deviation on its own (dB times the unit response, multiplied before rounding)."""
    nl = len(tau) + 1
    up, dn = np.zeros((len(devs), nl)), np.zeros((len(devs), nl))
    with mpmath.workdps(dps):
        col = IrColumn(tau, w0, g, emissivity, hard, tau_min)
        unit = {}
        for j, (k, db) in enumerate(devs):
            if k not in unit:
                unit[k] = col.unit_mp(int(k))
            d = _x(db)
            up[j], dn[j] = _round([d * v for v in unit[k][0]]), _round([d * v for v in unit[k][1]])
    return up, dn


def exact_solar_sum(tau, w0, g, zen_u, zen_w, Rsfc, dps=DPS):
    """sum_z w_z exact_solar(u0_z) -> amean, fup, fdn: what a solar call with several zenith angles returns."""
    with mpmath.workdps(dps):
        col = SolarColumn(tau, w0, g)
        acc = None
        for u, w in zip(zen_u, zen_w):
            one = col.solve_mp(u, Rsfc)
            w = _x(w)
            if acc is None:
                acc = [[w * v for v in a] for a in one]
            else:
                acc = [[s + w * v for s, v in zip(sa, a)] for sa, a in zip(acc, one)]
        return tuple(_round(a) for a in acc)
