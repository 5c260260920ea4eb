"""radtran_ir_jacobian without a GPU: the ABI is declared and exported, the Fortran binding compiles, and the CPU
yardstick (tests/ir_jacobian_oracle.py) is itself held to central differences of the oracle's full IR calls."""
import os
import re
import subprocess

import numpy as np
import pytest

import build_inspect
import ir_jacobian_oracle as J


def test_ir_jacobian_is_declared_exported_and_in_the_signature_table(hip_lib):
    from clima_amd import lib
    text = build_inspect.header_text()
    assert re.search(r"\bvoid\s+radtran_ir_jacobian\s*\(", text)
    assert hasattr(hip_lib, "radtran_ir_jacobian")
    assert len(lib.SIGNATURES["radtran_ir_jacobian"]) == 10


def test_planck_derivative_is_finite_over_the_whole_range():
    nu = 3.0e13
    T = np.array([1e-3, 1.0, 30.0, 300.0, 1500.0, 1e6, 1e9])
    d = J.dplanck_dT(nu, T)
    assert np.all(np.isfinite(d)) and np.all(d >= 0.0)
    assert d[0] == 0.0                                       # x ~ 1e9: the exponential underflows to 0, no NaN
    h = 1e-4 * T[2:5]                                        # against a central difference of planck_fcn where it is tame
    B = lambda t: 1.0e3 * 2.0 * J.PLANK * nu ** 3 / J.C_LIGHT ** 2 / np.expm1(J.PLANK * nu / (J.K_BOLTZ_SI * t))
    fd = (B(T[2:5] + h) - B(T[2:5] - h)) / (2 * h)
    assert np.allclose(d[2:5], fd, rtol=1e-6)


@pytest.mark.parametrize("nz,hard", [(5, True), (5, False), (30, True), (30, False)])
def test_yardstick_against_central_differences_of_the_oracle(O, nz, hard):
    """Central differences of radiate(..., compute_solar=False, compute_opacity=False) at two steps: the error against
    the yardstick falls as the step squared (truncation), so the yardstick is the derivative they converge to.  (The
    steps are large -- 4 and 2 % of the temperature: a column of a thin top layer is 1e-6 of the fluxes it is the
    difference of, and the oracle's own rounding would swamp the truncation error of smaller steps.)"""
    from clima_amd import synthetic as S
    tables = S.modern_earth_tables(nw=24)
    col = S.modern_earth_column(nz)
    o = O.OracleRadtran(tables, nz, 2, 0.3)
    o.set_scalars(has_hard_surface=hard)
    em = np.linspace(0.7, 1.0, o.nw_ir)
    o.set_surface_emissivity(em)
    o.radiate(*col.args(), compute_solar=True, compute_opacity=True)
    exact = J.exact_jacobian(O, tables, o.opr(), col["T_surface"], col["T"], em, hard, o.ir_tau_min,
                             zenith_weights=o.get_zenith()[1])

    def central(j, h):
        out = []
        for s in (+1, -1):
            o.radiate(*J.perturbed(col, j, s * h).args(), compute_solar=False, compute_opacity=False)
            w = o.wrk_ir
            out.append((np.array(w.fup_n), np.array(w.fdn_n)))
        return (out[0][0] - out[1][0]) / (2 * h), (out[0][1] - out[1][1]) / (2 * h)

    for j in range(nz + 1):
        Tj = col["T_surface"] if j == 0 else col["T"][j - 1]
        errs = []
        for h in (4e-2 * Tj, 2e-2 * Tj):
            fu, fd = central(j, h)
            e_up = np.max(np.abs(fu - exact[0][:, j])) / np.max(np.abs(exact[0][:, j]))
            e_dn = np.max(np.abs(fd - exact[1][:, j])) / max(np.max(np.abs(exact[1][:, j])), 1e-300)
            errs.append(max(e_up, e_dn))
        assert errs[1] < 1e-3, (j, errs)
        assert 3.0 < errs[0] / errs[1] < 5.0, (j, errs)        # second order: half the step, a quarter of the error
    assert np.array_equal(exact[2], exact[1] - exact[0])


def test_fortran_binding_compiles(tmp_path):
    from clima_amd import build as B
    if not os.path.exists(B.FLANG):
        pytest.skip("amdflang not found")
    mod = os.path.join(B.FORTRAN_DIR, "clima_radtran_hip.f90")
    prog = tmp_path / "jac.f90"
    prog.write_text("program jac\n  use clima_radtran_hip\n  implicit none\n  type(Radtran) :: rad\n"
                    "  real(dp) :: T(4), ju(5,5), jd(5,5), jt(5,5)\n  character(:), allocatable :: err\n"
                    "  T = 250.0_dp\n  if (.false.) call rad%ir_jacobian(280.0_dp, T, ju, jd, jt, err)\nend program\n")
    subprocess.check_call([B.FLANG, "-c", "-J", str(tmp_path), mod, "-o", str(tmp_path / "m.o")], cwd=str(tmp_path))
    subprocess.check_call([B.FLANG, "-c", "-I", str(tmp_path), "-J", str(tmp_path), str(prog), "-o", str(tmp_path / "p.o")],
                          cwd=str(tmp_path))
