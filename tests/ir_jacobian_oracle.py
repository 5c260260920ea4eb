"""The yardstick of radtran_ir_jacobian: the exact IR temperature Jacobian of the level fluxes, built on the CPU from the
oracle's two-stream solver (two_stream_ir, pinned to the compiled reference by tests/golden/twostream_golden_*.npz).

With the opacities fixed, two_stream_ir is linear in the Planck values of its nz+1 levels, so per (IR bin, g-point)
    dF / dT_k = R[:, k] * dB/dT(nu_bin, T_k),   R[:, k] = two_stream_ir(..., bplanck = unit vector at level k),
and the level fluxes are summed over the g-points (weights w_g), the zenith weights and the bins (width dnu) as
src/radtran/clima_radtran_radiate.f90:52-192 sums them.  Levels and k are TOA-first inside (k = nz: the surface); the
result is ground-first on both axes like the library's: row i = nz - level, column j = nz - k (x(1) = T_surface)."""
import numpy as np

PLANK, C_LIGHT, K_BOLTZ_SI = 6.62607004e-34, 299792458.0, 1.380649e-23


def dplanck_dT(nu, T):
    """d planck_fcn(nu, T) / dT (src/clima_eqns.f90:64-73), in a form without overflow or cancellation."""
    x = PLANK * nu / (K_BOLTZ_SI * T)
    K = 1.0e3 * 2.0 * PLANK * nu ** 3 / C_LIGHT ** 2
    e, em = np.exp(-x), np.expm1(-x)
    return K * (x / em) * (e / em) / T


def exact_jacobian(O, tables, opr, T_surface, T, emissivity, hard, tau_min, zenith_weights=(1.0,), cols=None):
    """(jac_up, jac_dn, jac_total), (nz+1, nz+1) ground-first; only the columns `cols` (indices j) are filled when given.
    opr: (tau, w0, g, ...) as Radtran.opr() / OracleRadtran.opr() return them (TOA-first)."""
    tau, w0, gt = opr[0], opr[1], opr[2]
    nz, ng, _ = tau.shape
    nl = nz + 1
    wavl, ir_wavl = np.asarray(tables.wavl, float), np.asarray(tables.ir_wavl, float)
    ir_start = len(wavl) - len(ir_wavl)
    assert np.allclose(wavl[ir_start:], ir_wavl, rtol=1e-7)
    freq, ir_freq = C_LIGHT / (wavl * 1.0e-9), C_LIGHT / (ir_wavl * 1.0e-9)
    wbin = np.asarray(tables.ktables[0]["weights"], float)
    assert len(wbin) == ng
    zw = float(np.sum(zenith_weights))
    emissivity = np.broadcast_to(np.asarray(emissivity, float), (len(ir_wavl) - 1,))
    T = np.asarray(T, float)
    Tk = np.concatenate([T[::-1], [float(T_surface)]])           # by level k, TOA-first
    ks = range(nl) if cols is None else sorted({nz - j for j in cols})
    up, dn = np.zeros((nl, nl)), np.zeros((nl, nl))              # [level, k], TOA-first
    for ll in range(len(ir_wavl) - 1):
        l = ir_start + ll
        avg = 0.5 * (freq[l] + freq[l + 1])
        amp = dplanck_dT(avg, Tk) * (ir_freq[ll] - ir_freq[ll + 1]) * zw
        for g in range(ng):
            t, w, gg = (np.ascontiguousarray(tau[:, g, l]), np.ascontiguousarray(w0[:, g, l]),
                        np.ascontiguousarray(gt[:, l]))
            for k in ks:
                e = np.zeros(nl)
                e[k] = 1.0
                fu, fd = O.two_stream_ir(t, w, gg, float(emissivity[ll]), hard, tau_min, e)
                up[:, k] += wbin[g] * amp[k] * fu
                dn[:, k] += wbin[g] * amp[k] * fd
    up, dn = up[::-1, ::-1].copy(order="F"), dn[::-1, ::-1].copy(order="F")
    return up, dn, np.asfortranarray(dn - up)


def perturbed(col, j, dT):
    """The column with x(j) moved by dT (j = 0: the surface, j = 1 + m: layer m, ground-first)."""
    from clima_amd import synthetic as S
    w = S.Column(col)
    w["T"] = np.array(col["T"], dtype=float)
    if j == 0:
        w["T_surface"] = float(col["T_surface"]) + dT
    else:
        w["T"][j - 1] += dT
    return w


def column_scaled_error(a, b, j):
    """max |a - b| of column j over the column's largest |b|."""
    return float(np.max(np.abs(a[:, j] - b[:, j])) / max(np.max(np.abs(b[:, j])), 1e-300))
