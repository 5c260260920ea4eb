"""radtran_ir_jacobian_reduced without a GPU: the ABI is declared and exported, the Fortran binding compiles with and
without its optional arguments, atmosphere.rce_jacobian_map is what the reference's loop does (restated here by brute
force), and the reduced yardstick S J C of tests/ir_jacobian_oracle.py is the derivative of the oracle's IR-only calls
with a whole group moved together."""
import os
import re
import subprocess

import numpy as np
import pytest

import build_inspect
import ir_jacobian_oracle as J


def test_ir_jacobian_reduced_is_declared_exported_and_in_the_signature_table(hip_lib):
    from clima_amd import lib
    text = build_inspect.header_text()
    assert re.search(r"\bvoid\s+radtran_ir_jacobian_reduced\s*\(", text)
    assert hasattr(hip_lib, "radtran_ir_jacobian_reduced")
    # the prototype's own count: ptr, T_surface, dim_T, T, dim_x, group_of_x, ngroup, nrow, row_level, dim1, dim2,
    # jac_up, jac_dn, jac_total, err
    assert len(lib.SIGNATURES["radtran_ir_jacobian_reduced"]) == 15
    assert build_inspect.header_arg_counts()["radtran_ir_jacobian_reduced"] == 15


def test_fortran_binding_compiles_with_and_without_the_optional_arguments(tmp_path):
    from clima_amd import build as B
    if not os.path.exists(B.FLANG):
        pytest.skip("amdflang not found")
    mod = os.path.join(B.FORTRAN_DIR, "clima_radtran_hip.f90")
    prog = tmp_path / "jac.f90"
    prog.write_text("program jac\n  use clima_radtran_hip\n  implicit none\n  type(Radtran) :: rad\n"
                    "  real(dp) :: T(4), ju(3,2), jd(3,2), jt(3,2)\n  integer :: grp(5), rows(3)\n"
                    "  character(:), allocatable :: err\n"
                    "  T = 250.0_dp\n  grp = [1, 1, 2, 2, 0]\n  rows = [1, 3, 5]\n"
                    "  if (.false.) call rad%ir_jacobian_reduced(280.0_dp, T, grp, rows, jt, err)\n"
                    "  if (.false.) call rad%ir_jacobian_reduced(280.0_dp, T, grp, rows, jt, err, ju, jd)\n"
                    "  if (.false.) call rad%ir_jacobian_reduced(280.0_dp, T, grp, rows, jt, err, jac_up=ju, jac_dn=jd)\n"
                    "end program\n")
    subprocess.check_call([B.FLANG, "-c", "-J", str(tmp_path), mod, "-o", str(tmp_path / "m.o")], cwd=str(tmp_path))
    subprocess.check_call([B.FLANG, "-c", "-I", str(tmp_path), "-J", str(tmp_path), str(prog), "-o", str(tmp_path / "p.o")],
                          cwd=str(tmp_path))


# ---- rce_jacobian_map against the reference's loop, restated by brute force

def _zones(conv):
    """(lower, upper) of the convecting zones over T_in, 1-based (AdiabatClimate_set_convecting_zones: a zone opens at
    the first i with conv(i) and runs to 1 + the last j of the run), and inds_Tx (1, then i + 1 wherever not conv(i))."""
    nz = len(conv)
    lower, upper = [], []
    i = 1
    while i <= nz:
        if conv[i - 1]:
            j = i
            while j <= nz and conv[j - 1]:
                j += 1
            lower.append(i)
            upper.append(j)              # (k = j_last + 1, j_last = j - 1)
            i = j
            continue
        i += 1
    inds = [1] + [i + 1 for i in range(1, nz + 1) if not conv[i - 1]]
    return lower, upper, inds


def _to_radiative_grid(T_in, doubled):
    """x of the radiative grid (x(1) = the surface) from T_in (copy_atm_to_radiative_grid)."""
    Ts, T = T_in[0], T_in[1:]
    if not doubled:
        return np.concatenate([[Ts], T])
    nz = len(T)
    Tr = np.empty(2 * nz + 2)
    for i in range(nz):
        Tr[2 * i] = T[i]
        Tr[2 * i + 1] = T[i]
    Tr[2 * nz] = Tr[2 * nz - 1]
    Tr[2 * nz + 1] = Tr[2 * nz - 1]
    return np.concatenate([[Ts], Tr])


def _brute_map(nz, conv, doubled):
    """Perturb T_in as the Jacobian's loop does for each unknown, copy to the radiative grid, and see which radiative
    temperatures moved: that is the unknown's group."""
    lower, upper, inds = _zones(conv)
    T_in = 200.0 + np.arange(nz + 1, dtype=float)
    base = _to_radiative_grid(T_in, doubled)
    group = np.zeros(len(base), dtype=int)
    for u, ind in enumerate(inds, start=1):
        Tp = T_in.copy()
        Tp[ind - 1] += 1.0
        if ind in lower:                                           # (ind_conv_lower_x: the unknown whose index opens a zone)
            z = lower.index(ind)
            Tp[lower[z] - 1:upper[z]] = T_in[lower[z] - 1:upper[z]] + 1.0
        moved = _to_radiative_grid(Tp, doubled) != base
        assert not np.any(group[moved]), "two unknowns move the same temperature"
        group[moved] = u
    rows = [2 * i - 1 for i in range(1, nz + 2)] if doubled else list(range(1, nz + 2))
    return group, rows, inds


MAP_CASES = [
    (5, [True, True, False, True, False]),                         # the worked case
    (5, [False] * 5),                                               # no zones
    (5, [True] * 5),                                                # one zone of all layers
    (6, [False, False, False, True, True, True]),                   # a zone touching the top
    (6, [True, False, True, False, False, True]),                   # three zones, one at the ground, one at the top
    (1, [True]), (1, [False]),
    (9, [False, True, True, False, False, True, False, True, True]),
]


@pytest.mark.parametrize("doubled", [True, False])
@pytest.mark.parametrize("nz,conv", MAP_CASES)
def test_rce_jacobian_map_against_the_brute_restatement(nz, conv, doubled):
    from clima_amd.atmosphere import rce_jacobian_map
    group, rows, inds = rce_jacobian_map(nz, conv, double_radiative_grid=doubled)
    bg, br, bi = _brute_map(nz, conv, doubled)
    assert list(group) == list(bg)
    assert list(rows) == br
    assert list(inds) == bi
    assert len(group) == (2 * nz + 3 if doubled else nz + 1)
    assert int(np.min(group)) == 1 and int(np.max(group)) == len(inds)   # every x moves with some unknown


def test_rce_jacobian_map_worked_case_and_defaults():
    from clima_amd.atmosphere import rce_jacobian_map
    from clima_amd.radtran import ClimaException
    g, rows, inds = rce_jacobian_map(5, [True, True, False, True, False], double_radiative_grid=False)
    assert list(g) == [1, 1, 1, 2, 2, 3] and list(inds) == [1, 4, 6] and list(rows) == [1, 2, 3, 4, 5, 6]
    g, rows, inds = rce_jacobian_map(5, [True, True, False, True, False])
    assert list(g) == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3]      # surface | 2 x layers 1..5 | the two ghosts
    assert list(rows) == [1, 3, 5, 7, 9, 11] and list(inds) == [1, 4, 6]
    g, rows, inds = rce_jacobian_map(3)                             # no zones: a pair per layer, the top with its ghosts
    assert list(g) == [1, 2, 2, 3, 3, 4, 4, 4, 4] and list(inds) == [1, 2, 3, 4]
    g, rows, inds = rce_jacobian_map(4, double_radiative_grid=False)
    assert list(g) == [1, 2, 3, 4, 5] and list(rows) == [1, 2, 3, 4, 5]
    for bad in ([True] * 4, [True] * 6, []):
        with pytest.raises(ClimaException, match='^Input "convecting_with_below" has the wrong dimension$'):
            rce_jacobian_map(5, bad)


# ---- the reduced yardstick

def reduce_full(jac, group_of_x, rows):
    """S J C: rows picked, the columns of each group added in ascending j."""
    group_of_x = np.asarray(group_of_x)
    out = np.zeros((len(rows), int(group_of_x.max())), order="F")
    for j, g in enumerate(group_of_x):
        if g > 0:
            out[:, g - 1] = out[:, g - 1] + jac[np.asarray(rows) - 1, j]
    return out


def reduced_yardstick(exact, group_of_x, rows):
    """(up, dn, total) of the reduced call from exact_jacobian's matrices: the total is dn - up OF THE REDUCED ones."""
    up, dn = reduce_full(exact[0], group_of_x, rows), reduce_full(exact[1], group_of_x, rows)
    return up, dn, np.asfortranarray(dn - up)


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("which", ["pairs", "zone"])
def test_reduced_yardstick_against_central_differences_of_the_oracle(O, which, hard):
    """The sizes and steps of test_yardstick_against_central_differences_of_the_oracle at nz = 30 radiative layers, the
    whole group moved together: a doubled-grid pair map (14 physical layers: 28 + 2 ghosts) and the same with zones."""
    from clima_amd import synthetic as S
    from clima_amd.atmosphere import rce_jacobian_map
    nz, nphys = 30, 14
    conv = None if which == "pairs" else [True] * 5 + [False] * 3 + [True] * 2 + [False] * 2 + [True] * 2
    group, rows, _ = rce_jacobian_map(nphys, conv)
    assert len(group) == nz + 1
    tables = S.modern_earth_tables(nw=24)
    col = S.modern_earth_column(nz)
    o = O.OracleRadtran(tables, nz, 2, 0.3)
    o.set_scalars(has_hard_surface=hard)
    em = np.linspace(0.7, 1.0, o.nw_ir)
    o.set_surface_emissivity(em)
    o.radiate(*col.args(), compute_solar=True, compute_opacity=True)
    exact = J.exact_jacobian(O, tables, o.opr(), col["T_surface"], col["T"], em, hard, o.ir_tau_min,
                             zenith_weights=o.get_zenith()[1])
    want = reduced_yardstick(exact, group, rows)
    x = np.concatenate([[col["T_surface"]], col["T"]])
    pick = np.asarray(rows) - 1

    def central(members, h):
        out = []
        for s in (+1, -1):
            w = S.Column(col)
            xp = x.copy()
            xp[members] += s * h                                    # the whole group by the same step (the reference's deltaT)
            w["T_surface"], w["T"] = float(xp[0]), xp[1:].copy()
            o.radiate(*w.args(), compute_solar=False, compute_opacity=False)
            out.append((np.array(o.wrk_ir.fup_n)[pick], np.array(o.wrk_ir.fdn_n)[pick]))
        return (out[0][0] - out[1][0]) / (2 * h), (out[0][1] - out[1][1]) / (2 * h)

    for g in range(1, int(group.max()) + 1):
        members = np.flatnonzero(group == g)
        errs = []
        for rel in (4e-2, 2e-2):
            fu, fd = central(members, rel * x[members[0]])
            e_up = np.max(np.abs(fu - want[0][:, g - 1])) / np.max(np.abs(want[0][:, g - 1]))
            e_dn = np.max(np.abs(fd - want[1][:, g - 1])) / max(np.max(np.abs(want[1][:, g - 1])), 1e-300)
            errs.append(max(e_up, e_dn))
        assert errs[1] < 1e-3, (g, errs)
        assert 3.0 < errs[0] / errs[1] < 5.0, (g, errs)            # second order: half the step, a quarter of the error
