"""The yardstick of radtran_ir_jacobian_spectral_rows: tests/ir_jacobian_oracle.py's exact Jacobian BEFORE the sum over
the bins, built the same way (the oracle's two_stream_ir on unit Planck vectors, summed over the g-points with their
weights and times the zenith weights' sum), with the amplitude dB/dT(avg_freq(bin), T_k) and without the bin's width:
per Hz.  Levels and k are TOA-first inside; the result is ground-first on both axes like the library's."""
import numpy as np

import ir_jacobian_oracle as J


def channel(tables):
    """(ir_start, freq of the opacity grid, freq of the IR channel) as exact_jacobian takes them"""
    wavl, ir_wavl = np.asarray(tables.wavl, float), np.asarray(tables.ir_wavl, float)
    ir_start = len(wavl) - len(ir_wavl)
    assert np.allclose(wavl[ir_start:], ir_wavl, rtol=1e-7)
    return ir_start, J.C_LIGHT / (wavl * 1.0e-9), J.C_LIGHT / (ir_wavl * 1.0e-9)


def dfreq(tables):
    """the IR bins' widths freq(l) - freq(l+1), in the channel's own order"""
    ir_freq = channel(tables)[2]
    return ir_freq[:-1] - ir_freq[1:]


def unit_responses(O, tau, w0, gt, wbin, emissivity, hard, tau_min, ks=None):
    """(up, dn)[level, k], TOA-first: d fup(level) / d bplanck(k) of one bin's column tau / w0 (nz, ng), gt (nz), summed
    over the g-points with wbin; only the columns `ks` are filled when given."""
    nz, ng = tau.shape
    nl = nz + 1
    up, dn = np.zeros((nl, nl)), np.zeros((nl, nl))
    for g in range(ng):
        t, w, gg = np.ascontiguousarray(tau[:, g]), np.ascontiguousarray(w0[:, g]), np.ascontiguousarray(gt)
        for k in (range(nl) if ks is None else ks):
            e = np.zeros(nl)
            e[k] = 1.0
            fu, fd = O.two_stream_ir(t, w, gg, float(emissivity), hard, tau_min, e)
            up[:, k] += wbin[g] * fu
            dn[:, k] += wbin[g] * fd
    return up, dn


def spectral_jacobian(O, tables, opr, T_surface, T, emissivity, hard, tau_min, zenith_weights=(1.0,), cols=None, bins=None):
    """(up, dn, scale): up, dn (nbins, nz+1, nz+1), [bin, i, j] = d f*_a(level i, bin) / d x(j) ground-first on both axes,
    per Hz; scale (nbins): the largest |entry| of the bin's two matrices.  Only the columns `cols` (indices j) are filled
    when given, only the IR bins `bins` (channel indices) computed when given (the first axis follows `bins`)."""
    tau, w0, gt = opr[0], opr[1], opr[2]
    nz, ng, _ = tau.shape
    nl = nz + 1
    ir_start, freq, ir_freq = channel(tables)
    wbin = np.asarray(tables.ktables[0]["weights"], float)
    assert len(wbin) == ng
    zw = float(np.sum(zenith_weights))
    nw_ir = len(ir_freq) - 1
    emissivity = np.broadcast_to(np.asarray(emissivity, float), (nw_ir,))
    Tk = np.concatenate([np.asarray(T, float)[::-1], [float(T_surface)]])           # by level k, TOA-first
    ks = None if cols is None else sorted({nz - j for j in cols})
    bins = list(range(nw_ir)) if bins is None else list(bins)
    up, dn = np.zeros((len(bins), nl, nl)), np.zeros((len(bins), nl, nl))
    for b, ll in enumerate(bins):
        l = ir_start + ll
        amp = J.dplanck_dT(0.5 * (freq[l] + freq[l + 1]), Tk) * zw
        u, d = unit_responses(O, tau[:, :, l], w0[:, :, l], gt[:, l], wbin, emissivity[ll], hard, tau_min, ks)
        up[b] = (u * amp[None, :])[::-1, ::-1]
        dn[b] = (d * amp[None, :])[::-1, ::-1]
    scale = np.maximum(np.max(np.abs(up), axis=(1, 2)), np.max(np.abs(dn), axis=(1, 2)))
    return up, dn, scale
