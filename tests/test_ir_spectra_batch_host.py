"""The identity radtran_ir_spectra_batch rests on, without a GPU: at fixed opacities the per-bin IR level fluxes of any
temperature profile are the unit responses of two_stream_ir (tests/ir_jacobian_spectral_oracle.py:unit_responses) times
the Planck values of the levels (tests/ir_spectra_batch_oracle.py), against the CPU oracle's own IR-only call.

The worst error is taken per bin and per direction against the largest level flux of that bin.  Measured with the oracle
(modern_earth_tables(nw=40), 24 IR bins; nz: hard surface / none): 1: 1.8e-12 / 1.7e-15, 5: 3.7e-11 / 3.1e-11, 33: 6.4e-10
/ 6.9e-10, 65: 3.4e-10 / 1.6e-10 -- the conditioning floor of the method (the 1 / tau source slope of the thinnest layers
above ir_tau_min).  The bound is five times the worst.  One profile per case, the first draw of default_rng(nz) (T, then
T_surface): later draws of the same generator reach 3.0e-8 at nz = 5 with a hard surface (T = 232, 159, 160, 350, 280 K over
layers of tau = 0.85e-6 .. 3e-6), where the oracle's IR-only call is itself 2.8e-8 from its other compilation (FMA
contraction on) -- the conditioning of the reference call on 200 K steps across layers at ir_tau_min, not of the identity."""
import numpy as np
import pytest

import ir_spectra_batch_oracle as SB

MEASURED = 6.9e-10
TOL = 3.5e-9


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("nz", [1, 5, 33, 65])
def test_unit_responses_times_planck_are_the_ir_only_call(O, small_tables, nz, hard):
    from clima_amd import synthetic as S
    col = S.modern_earth_column(nz)
    o = O.OracleRadtran(small_tables, nz, 2, 0.3)
    o.set_scalars(has_hard_surface=hard)
    assert o.nw_ir == 24
    em = np.linspace(0.65, 1.0, o.nw_ir)
    o.set_surface_emissivity(em)
    o.radiate(*col.args(), compute_solar=True, compute_opacity=True)
    w = SB.weights(O, small_tables, o.opr(), em, hard, o.ir_tau_min)
    assert not np.any(w[1][:, nz, :])                                # fdn at the top of the atmosphere is the constant 0
    rng = np.random.default_rng(nz)
    T, Ts = rng.uniform(150.0, 350.0, nz), float(rng.uniform(150.0, 350.0))
    up, dn = SB.from_weights(O, small_tables, w, Ts, T)
    wu, wd, fun, fdn = SB.from_call(o, col, Ts, T)
    assert up.shape == wu.shape == (o.nw_ir, nz + 1)
    worst = SB.per_bin_worst(up, dn, wu, wd)                         # per bin and per direction
    print("nz %d hard %s: %.2e of the bin's largest level flux [%.1e]" % (nz, hard, worst, TOL))
    assert worst <= TOL
