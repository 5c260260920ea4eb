"""The yardstick of radtran_ir_spectra_batch: the per-bin IR level fluxes of one temperature profile on given optical
properties, two ways.  `from_weights`: the identity the call rests on -- at fixed opacities two_stream_ir is homogeneously
linear in the Planck values, so a flux is the unit responses (tests/ir_jacobian_spectral_oracle.py:unit_responses, the
oracle's two_stream_ir on unit Planck vectors summed over the g-points) times O.planck_fcn at the levels.  `from_call`:
the oracle's own IR-only call.  Both return (up, dn) as (nw_ir, nz+1), levels ground-first like the library's."""
import numpy as np

import ir_jacobian_spectral_oracle as JS


def level_temperatures(T_surface, T):
    """by level k, TOA-first (radiate.f90:65-69: level k is layer nz-1-k, the last one the surface)"""
    return np.concatenate([np.asarray(T, float)[::-1], [float(T_surface)]])


def weights(O, tables, opr, emissivity, hard, tau_min, bins=None):
    """(w_up, w_dn) (nbins, nz+1 levels, nz+1 j), both axes ground-first: d f(level, bin) / d B(x(j))"""
    tau, w0, gt = opr[0], opr[1], opr[2]
    nz = tau.shape[0]
    ir_start, freq, ir_freq = JS.channel(tables)
    wbin = np.asarray(tables.ktables[0]["weights"], float)
    nw_ir = len(ir_freq) - 1
    emissivity = np.broadcast_to(np.asarray(emissivity, float), (nw_ir,))
    bins = list(range(nw_ir)) if bins is None else list(bins)
    up, dn = np.zeros((len(bins), nz + 1, nz + 1)), np.zeros((len(bins), nz + 1, nz + 1))
    for b, ll in enumerate(bins):
        l = ir_start + ll
        u, d = JS.unit_responses(O, tau[:, :, l], w0[:, :, l], gt[:, l], wbin, emissivity[ll], hard, tau_min)
        up[b], dn[b] = u[::-1, ::-1], d[::-1, ::-1]
    return up, dn


def planck_rows(O, tables, T_surface, T, bins=None):
    """B(avg_freq(bin), x(j)) (nbins, nz+1), j ground-first (x(0) = T_surface)"""
    ir_start, freq, ir_freq = JS.channel(tables)
    bins = list(range(len(ir_freq) - 1)) if bins is None else list(bins)
    x = level_temperatures(T_surface, T)[::-1]
    return np.array([[O.planck_fcn(0.5 * (freq[ir_start + ll] + freq[ir_start + ll + 1]), float(t)) for t in x] for ll in bins])


def from_weights(O, tables, w, T_surface, T, bins=None):
    """(up, dn) (nbins, nz+1) of a profile from `weights`' result"""
    B = planck_rows(O, tables, T_surface, T, bins)
    return np.einsum("bij,bj->bi", w[0], B), np.einsum("bij,bj->bi", w[1], B)


def from_call(o, col, T_surface, T):
    """(up, dn, fup_n, fdn_n) of the oracle's IR-only call on its stored opacities: (nw_ir, nz+1) and (nz+1)"""
    a = col.args()
    o.radiate(float(T_surface), np.asarray(T, float), *a[2:], compute_solar=False, compute_opacity=False)
    w = o.wrk_ir
    return np.array(w.fup_a).T, np.array(w.fdn_a).T, np.array(w.fup_n), np.array(w.fdn_n)


def per_bin_worst(got_up, got_dn, want_up, want_dn):
    """the largest |got - want| over the levels given, every bin on the scale of ITS largest level flux in `want` (both
    directions, all of want's levels): arrays (nbins, levels)"""
    scale = np.maximum(np.max(np.abs(want_up), axis=1), np.max(np.abs(want_dn), axis=1))
    e = np.maximum(np.max(np.abs(got_up - want_up), axis=1), np.max(np.abs(got_dn - want_dn), axis=1)) / scale
    return float(np.max(e))
