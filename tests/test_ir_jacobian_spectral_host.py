"""The per-bin yardstick (tests/ir_jacobian_spectral_oracle.py) without a GPU: its bins times their widths, summed in bin
order, are the bin-summed yardstick of radtran_ir_jacobian (tests/ir_jacobian_oracle.py), which is itself held to central
differences of the oracle's full IR calls."""
import numpy as np
import pytest

import ir_jacobian_oracle as J
import ir_jacobian_spectral_oracle as JS


@pytest.mark.parametrize("nz", [5, 30])
@pytest.mark.parametrize("hard", [True, False])
def test_bins_times_widths_sum_to_the_exact_jacobian(O, nz, hard):
    from clima_amd import synthetic as S
    tables = S.modern_earth_tables(nw=24)
    col = S.modern_earth_column(nz)
    o = O.OracleRadtran(tables, nz, 2, 0.3)
    o.set_scalars(has_hard_surface=hard)
    em = np.linspace(0.7, 1.0, o.nw_ir)
    o.set_surface_emissivity(em)
    o.radiate(*col.args(), compute_solar=True, compute_opacity=True)
    args = (O, tables, o.opr(), col["T_surface"], col["T"], em, hard, o.ir_tau_min)
    zw = o.get_zenith()[1]
    exact = J.exact_jacobian(*args, zenith_weights=zw)
    up, dn, scale = JS.spectral_jacobian(*args, zenith_weights=zw)
    assert up.shape == dn.shape == (o.nw_ir, nz + 1, nz + 1) and scale.shape == (o.nw_ir,)
    np.testing.assert_array_equal(scale, np.maximum(np.abs(up).max(axis=(1, 2)), np.abs(dn).max(axis=(1, 2))))
    assert not np.any(dn[:, nz, :])                                  # fdn at the top of the atmosphere is the constant 0
    df = JS.dfreq(tables)
    for a, want in ((up, exact[0]), (dn, exact[1])):
        s = np.zeros((nz + 1, nz + 1))
        for l in range(o.nw_ir):
            s += a[l] * df[l]
        assert np.max(np.abs(s - want)) <= 1e-13 * np.max(np.abs(want))
    # columns and bins picked: the same entries
    cols, bins = [0, 2, nz], [3, 0, o.nw_ir - 1]
    pu, pd, ps = JS.spectral_jacobian(*args, zenith_weights=zw, cols=cols, bins=bins)
    for b, ll in enumerate(bins):
        np.testing.assert_array_equal(pu[b][:, cols], up[ll][:, cols])
        np.testing.assert_array_equal(pd[b][:, cols], dn[ll][:, cols])
