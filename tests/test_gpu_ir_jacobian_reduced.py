"""radtran_ir_jacobian_reduced: the exact IR temperature Jacobian in the caller's unknowns (groups of x summed, rows
picked, on the device).  Held bit for bit to the caller's own loop over the same handle's radtran_ir_jacobian, to the CPU
yardstick S J C (tests/ir_jacobian_oracle.py), to central differences through the library's general batch kernel with a
whole group moved, and to itself (repeatable, the handle's state untouched, communicator handles, refusals, Fortran)."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_ir_jacobian import FORTRAN_PROGRAM as FULL_PROGRAM, _handle, _yardstick, far_forms  # noqa: F401
from test_ir_jacobian_reduced_host import reduce_full, reduced_yardstick

pytestmark = pytest.mark.gpu

# of the reduced matrix's largest |value| (every entry): the bounds tests/test_gpu_ir_jacobian.py holds jac_total to
TOL = 5.0e-10
TOL_THIN = 1.0e-7       # ir_tau_min = 1e-8


def loop_reduce(full, group_of_x, rows):
    """What a caller of ir_jacobian does today: the columns of each group added in ascending j, rows picked; the total
    from the reduced up and down."""
    up, dn = reduce_full(full[0], group_of_x, rows), reduce_full(full[1], group_of_x, rows)
    return up, dn, dn - up


def _maps(nz):
    """(name, group_of_x, rows) over nz radiative layers (nz + 1 x, nz + 1 levels)."""
    from clima_amd.atmosphere import rce_jacobian_map
    nl = nz + 1
    out = [("identity", np.arange(1, nl + 1), None)]
    if nz % 2 == 0:
        nphys = (nz - 2) // 2
        conv = np.zeros(nphys, dtype=bool)
        conv[: max(1, nphys // 3)] = True                           # a zone from the ground
        if nphys >= 6:
            conv[nphys - 2:] = True                                 # and one touching the top (with the ghosts)
        g, rows, _ = rce_jacobian_map(nphys, conv)
        out.append(("doubled grid with zones", g, rows))
    else:
        g, rows, _ = rce_jacobian_map(nz, np.arange(nz) % 3 != 2, double_radiative_grid=False)
        out.append(("plain grid with zones", g, rows))
    fixed = np.zeros(nl, dtype=int)                                 # most x held fixed, groups out of order along x
    fixed[1], fixed[nl - 1], fixed[nl // 2], fixed[0] = 2, 1, 2, 3
    rng = np.random.default_rng(nz)
    rows = np.concatenate([[nl, 1, 1, nl // 2], rng.integers(1, nl + 1, size=5)])    # unordered, repeated
    out.append(("fixed entries, unordered rows", fixed, rows))
    return out


def _worst(got, want, cols, label):
    """Largest error of the columns `cols` (0-based groups), of each matrix's largest |value| over those columns."""
    cols = list(cols)
    worst = max(float(np.max(np.abs(a[:, cols] - b[:, cols]))) / float(np.max(np.abs(b[:, cols]))) for a, b in zip(got, want))
    print("%s: %.1e of the reduced matrix's maximum" % (label, worst))
    return worst


@pytest.mark.parametrize("nz", [4, 5, 30, 102, 402])
@pytest.mark.parametrize("hard", [True, False])
def test_parts_are_bitwise_the_callers_loop(small_tables, far_forms, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    for form in (0, 1):
        far_forms(form)
        full = r.ir_jacobian(col["T_surface"], col["T"])
        for name, group, rows in _maps(nz):
            want = loop_reduce(full, group, np.arange(1, nz + 2) if rows is None else rows)
            got = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)
            for a, b in zip(got, want):
                assert a.shape == b.shape and a.flags.f_contiguous, name
                np.testing.assert_array_equal(a, b, err_msg="%s, far form %d" % (name, form))
            np.testing.assert_array_equal(got[2], got[1] - got[0])
            tot = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows)
            assert tot.shape == want[2].shape and tot.flags.f_contiguous
            # total-only runs two-sided and returns jac_dn - jac_up: bit for bit the parts' (and so within the 1e-12 of
            # the matrix maximum a one-sided accumulation would be held to)
            np.testing.assert_array_equal(tot, got[2], err_msg="%s, far form %d" % (name, form))
    far_forms(0)


@pytest.mark.parametrize("nz", [4, 5, 30, 102])
@pytest.mark.parametrize("hard", [True, False])
def test_total_only_against_the_yardstick(O, small_tables, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    r.surface_emissivity = np.linspace(0.65, 1.0, len(r.surface_emissivity))
    exact = _yardstick(O, small_tables, r, col)
    for name, group, rows in _maps(nz):
        want = reduced_yardstick(exact, group, np.arange(1, nz + 2) if rows is None else rows)
        got = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows)
        ng = int(np.max(group))
        assert _worst([got], [want[2]], range(ng), "nz %d hard %s, %s, total only" % (nz, hard, name)) <= TOL
        parts = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)
        assert _worst(parts, want, range(ng), "nz %d hard %s, %s, parts" % (nz, hard, name)) <= TOL
        assert np.max(np.abs(got - parts[2])) <= 1e-12 * np.max(np.abs(parts[2]))


@pytest.mark.parametrize("hard", [True, False])
def test_total_only_402_layers_against_the_yardstick(O, small_tables, hard):
    """AdiabatClimate nz = 200: the yardstick for the members of a handful of groups only (the surface group, the bottom,
    the middle, the top one with its ghosts, one zone of about 20 layers)."""
    from clima_amd.atmosphere import rce_jacobian_map
    nphys, nz = 200, 402
    conv = np.zeros(nphys, dtype=bool)
    conv[60:70] = True                                              # T_in(62..71) join T_in(61): layers 60..70, 22 radiative layers
    group, rows, inds = rce_jacobian_map(nphys, conv)
    r, col = _handle(small_tables, nz, hard)
    zone = int(group[2 * 60])                                       # the group of physical layer 60's second copy
    assert int(np.sum(group == zone)) == 22
    picks = [1, 2, int(group[nz // 2]), int(group.max()), zone]    # 1-based groups
    members = [int(j) for g in picks for j in np.flatnonzero(group == g)]
    assert int(np.sum(group == group.max())) == 4                   # the top layer's pair and the two ghosts
    exact = _yardstick(O, small_tables, r, col, cols=members)
    want = reduced_yardstick(exact, group, rows)
    got = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows)
    assert got.shape == (nphys + 1, len(inds))
    cols = [g - 1 for g in picks]
    assert _worst([got], [want[2]], cols, "nz 402 hard %s, total only" % hard) <= TOL
    parts = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)
    assert _worst(parts, want, cols, "nz 402 hard %s, parts" % hard) <= TOL
    assert np.max(np.abs(got - parts[2])) <= 1e-12 * np.max(np.abs(parts[2]))


def test_thin_layers(O, small_tables):
    from clima_amd.atmosphere import rce_jacobian_map
    nz = 64
    r, col = _handle(small_tables, nz, True, ir_tau_min=1.0e-8)
    group, rows, _ = rce_jacobian_map(31, np.arange(31) < 6)
    want = reduced_yardstick(_yardstick(O, small_tables, r, col), group, rows)
    got = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows)
    assert _worst([got], [want[2]], range(int(group.max())), "ir_tau_min 1e-8") <= TOL_THIN


def test_against_central_differences_of_the_general_batch_kernel(small_tables):
    """The library's own batch with ir_green = 0 (one general solve per column), a whole group moved by one step of
    1e-4 T (of the group's first member, as the reference's deltaT = epsj |x(i)| moves a zone): the bound of
    tests/test_gpu_ir_jacobian.py's test of the same name -- the step's truncation, 1e-5 of the column's maximum, plus
    the cancellation of two level fluxes, 1e-13 of the fluxes over the step."""
    from clima_amd.atmosphere import rce_jacobian_map
    nphys, nz = 29, 60
    conv = np.zeros(nphys, dtype=bool)
    conv[:4] = True                                                 # the surface and the four layers above
    conv[20:23] = True
    group, rows, _ = rce_jacobian_map(nphys, conv)
    r, col = _handle(small_tables, nz, True)
    got = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)
    x = np.concatenate([[col["T_surface"]], col["T"]])
    ng = int(group.max())
    pick = np.asarray(rows) - 1
    h = np.array([1.0e-4 * x[np.flatnonzero(group == g + 1)[0]] for g in range(ng)])
    X = np.repeat(x[:, None], 2 * ng, axis=1)
    for g in range(ng):
        m = np.flatnonzero(group == g + 1)
        X[m, 2 * g] += h[g]
        X[m, 2 * g + 1] -= h[g]
    r.ir_green = 0
    out = r.radiate_ir_batch(X[0], X[1:])
    assert r.ir_green_batches == 0
    scale = max(np.max(np.abs(out[0])), np.max(np.abs(out[1])))
    for k in range(3):
        for g in range(ng):
            fd = (out[k][pick, 2 * g] - out[k][pick, 2 * g + 1]) / (2 * h[g])
            err = np.max(np.abs(fd - got[k][:, g]))
            assert err <= 1e-5 * np.max(np.abs(got[k][:, g])) + 1e-13 * scale / h[g], (k, g)


def test_repeatable_and_the_handle_untouched(small_tables, far_forms):
    from clima_amd.atmosphere import rce_jacobian_map
    nz = 50
    r, col = _handle(small_tables, nz, True)
    group, rows, _ = rce_jacobian_map(24, np.arange(24) < 5)
    T = np.repeat(np.asarray(col["T"], float)[:, None], 12, axis=1)
    Ts = np.full(12, float(col["T_surface"]))
    for c in range(12):
        T[(4 * c) % nz, c] += 0.3 + 0.05 * c
    before = {}
    for mode in (0, 2):
        r.ir_green = mode
        before[mode] = r.radiate_ir_batch(Ts, T)
    names = ("fup_n", "fdn_n", "fup_a", "fdn_a")
    w_ir = [np.array(getattr(r.wrk_ir, a)) for a in names]
    w_sol = [np.array(getattr(r.wrk_sol, a)) for a in names]
    ft = np.array(r.f_total)
    full = r.ir_jacobian(col["T_surface"], col["T"])
    for parts in (True, False):
        a = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=parts)
        b = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=parts)
        for x, y in zip(a if parts else [a], b if parts else [b]):
            np.testing.assert_array_equal(x, y)
        # the work arrays are shared: the full call after a reduced one is what it was
        for x, y in zip(r.ir_jacobian(col["T_surface"], col["T"]), full):
            np.testing.assert_array_equal(x, y)
    for v, name in zip(w_ir, names):
        np.testing.assert_array_equal(np.array(getattr(r.wrk_ir, name)), v)
    for v, name in zip(w_sol, names):
        np.testing.assert_array_equal(np.array(getattr(r.wrk_sol, name)), v)
    np.testing.assert_array_equal(np.array(r.f_total), ft)
    for mode in (0, 2):
        r.ir_green = mode
        for x, y in zip(r.radiate_ir_batch(Ts, T), before[mode]):
            np.testing.assert_array_equal(x, y)


def test_communicator_handles(small_tables):
    from clima_amd import synthetic as S
    from clima_amd.atmosphere import rce_jacobian_map
    from clima_amd.radtran import ClimaException, Radtran
    nz, W = 60, 3
    col = S.modern_earth_column(nz)
    group, rows, inds = rce_jacobian_map(29, np.arange(29) < 4)
    ref, _ = _handle(small_tables, nz, True, col)
    want = ref.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)

    one = Radtran(small_tables, nz, 2, 0.3)
    one.comm_init_rank(1, 0, Radtran.comm_unique_id())
    one.radiate(*col.args())
    for parts in (True, False):
        n0 = one.comm()[2]
        got = one.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=parts)
        assert one.comm()[2] == n0 + 1                             # one collective per call
        for a, b in zip(got if parts else [got], want if parts else [want[2]]):
            np.testing.assert_array_equal(a, b)

    shards = []
    for k in range(W):
        r = Radtran(small_tables, nz, 2, 0.3)
        r.comm_init_rank(1, 0, Radtran.comm_unique_id())
        r.set_bin_shard(k, W)
        r.radiate(*col.args())
        shards.append(r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True))
    for i in range(3):
        s = sum(p[i] for p in shards)
        np.testing.assert_allclose(s, want[i], rtol=1e-12, atol=1e-12 * np.max(np.abs(want[i])))

    # a shard without IR bins: zeros, no error (and no response-form kernel on an empty grid)
    W2 = 16
    empty = None
    for k in range(W2):
        r = Radtran(small_tables, nz, 2, 0.3)
        r.comm_init_rank(1, 0, Radtran.comm_unique_id())
        r.set_bin_shard(k, W2)
        if r.bin_shard()[3] == 0:
            empty = r
            break
        r.comm_destroy()
    assert empty is not None, "no rehearsed shard without IR bins"
    empty.radiate(*col.args())
    for parts in (True, False):
        z = empty.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=parts)
        for m in (z if parts else [z]):
            assert m.shape == (len(rows), len(inds)) and not np.any(m)

    plain = Radtran(small_tables, nz, 2, 0.3)
    plain.set_bin_shard(0, 2)                                       # a shard without a communicator: nobody would reduce
    plain.radiate(*col.args())
    with pytest.raises(ClimaException, match="^ir_jacobian is not available on a bin-sharded handle$"):
        plain.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows)


def test_refusals(hip_lib, small_tables):
    import ctypes as C
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    nz = 10
    col = S.modern_earth_column(nz)
    L = hip_lib
    err = C.create_string_buffer(1025)
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    nl = nz + 1
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    T = np.ascontiguousarray(col["T"], dtype=float)
    ident = np.arange(1, nl + 1, dtype=np.int32)
    all_rows = np.arange(1, nl + 1, dtype=np.int32)

    def call(handle, group=ident, ngroup=nl, rows=all_rows, nrow=None, dim_T=nz, dim_x=None, d1=None, d2=None, up=True, dn=True,
             Ts=280.0, total=True):
        nrow = len(rows) if nrow is None else nrow
        d1, d2 = nrow if d1 is None else d1, ngroup if d2 is None else d2
        buf = [np.empty((max(nrow, 1), max(ngroup, 1)), order="F") for _ in range(3)]
        group, rows = np.ascontiguousarray(group, dtype=np.int32), np.ascontiguousarray(rows, dtype=np.int32)
        L.radtran_ir_jacobian_reduced(handle, C.byref(C.c_double(Ts)), C.byref(C.c_int(dim_T)), T.ctypes.data_as(dp),
                                      C.byref(C.c_int(len(group) if dim_x is None else dim_x)), group.ctypes.data_as(ip),
                                      C.byref(C.c_int(ngroup)), C.byref(C.c_int(nrow)), rows.ctypes.data_as(ip),
                                      C.byref(C.c_int(d1)), C.byref(C.c_int(d2)),
                                      buf[0].ctypes.data_as(dp) if up else None, buf[1].ctypes.data_as(dp) if dn else None,
                                      buf[2].ctypes.data_as(dp) if total else None, err)
        return err.value.decode()

    assert call(h) == "Radtran is not constructed"
    L.deallocate_radtran(h)
    r = Radtran(small_tables, nz, 2, 0.3)
    with pytest.raises(ClimaException, match="^ir_jacobian needs opacities: call radiate with compute_opacity first$"):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], ident)
    r.radiate(*col.args())
    p = r._ptr
    assert call(p) == ""
    assert call(p, up=False, dn=False) == ""
    assert call(p, dim_T=nz - 1) == '"T" has the wrong input dimension.'
    # the map
    assert call(p, group=ident[:-1], ngroup=nl - 1) == \
        'ir_jacobian_reduced: "group_of_x" has the wrong dimension (dim_x = %d, nz + 1 = %d)' % (nl - 1, nl)
    assert call(p, dim_x=nl + 1) == 'ir_jacobian_reduced: "group_of_x" has the wrong dimension (dim_x = %d, nz + 1 = %d)' % (nl + 1, nl)
    bad = ident.copy()
    bad[3] = nl + 1
    assert call(p, group=bad) == "ir_jacobian_reduced: group_of_x(4) = %d is outside 0..%d" % (nl + 1, nl)
    bad[3] = -1
    assert call(p, group=bad) == "ir_jacobian_reduced: group_of_x(4) = -1 is outside 0..%d" % nl
    gap = ident.copy()
    gap[6] = 0                                                      # group 7 lost its only member
    assert call(p, group=gap) == "ir_jacobian_reduced: group 7 of %d has no member in group_of_x" % nl
    assert call(p, ngroup=nl + 1) == "ir_jacobian_reduced: group %d of %d has no member in group_of_x" % (nl + 1, nl + 1)
    # the rows
    rows = all_rows.copy()
    rows[2] = nl + 1
    assert call(p, rows=rows) == "ir_jacobian_reduced: row_level(3) = %d is outside 1..%d" % (nl + 1, nl)
    rows[2] = 0
    assert call(p, rows=rows) == "ir_jacobian_reduced: row_level(3) = 0 is outside 1..%d" % nl
    assert call(p, nrow=0) == "ir_jacobian_reduced: nrow must be at least 1 (nrow = 0)"
    assert call(p, nrow=-2) == "ir_jacobian_reduced: nrow must be at least 1 (nrow = -2)"
    assert call(p, group=np.zeros(nl), ngroup=0) == "ir_jacobian_reduced: ngroup must be at least 1 (ngroup = 0)"
    # the results
    assert call(p, dn=False) == "ir_jacobian_reduced: jac_up and jac_dn go together: only jac_up was given"
    assert call(p, up=False) == "ir_jacobian_reduced: jac_up and jac_dn go together: only jac_dn was given"
    assert call(p, total=False) == "ir_jacobian_reduced: jac_total is required (only jac_up and jac_dn may be absent)"
    assert call(p, d1=nl - 1) == "jac has the wrong dimension"
    assert call(p, d2=nl + 1) == "jac has the wrong dimension"
    # through Python
    with pytest.raises(ClimaException, match='^"T" has the wrong input dimension.$'):
        r.ir_jacobian_reduced(col["T_surface"], col["T"][:-1], ident)
    with pytest.raises(ClimaException, match="has the wrong dimension"):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], ident[:-1])
    with pytest.raises(ClimaException, match=r'^ir_jacobian_reduced: "group_of_x" has the wrong dimension \(2 axes, one expected\)$'):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], ident.reshape(1, -1))
    with pytest.raises(ClimaException, match=r'^ir_jacobian_reduced: "rows" has the wrong dimension \(2 axes, one expected\)$'):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], ident, rows=all_rows.reshape(1, -1))
    with pytest.raises(ClimaException, match="ngroup must be at least 1"):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], np.zeros(nl, dtype=int))
    with pytest.raises(ClimaException, match=r"row_level\(1\) = 12 is outside 1\.\.11"):
        r.ir_jacobian_reduced(col["T_surface"], col["T"], ident, rows=[12])
    # everything radtran_ir_jacobian refuses, with its texts
    for v in (np.nan, np.inf, 0.0, -5.0):
        with pytest.raises(ClimaException, match="^ir_jacobian: temperatures must be finite and positive$"):
            r.ir_jacobian_reduced(v, col["T"], ident)
        Tb = np.array(col["T"], float)
        Tb[3] = v
        with pytest.raises(ClimaException, match="^ir_jacobian: temperatures must be finite and positive$"):
            r.ir_jacobian_reduced(col["T_surface"], Tb, ident)
    for n in (3, 513):
        c = S.modern_earth_column(n)
        s = Radtran(small_tables, n, 2, 0.3)
        s.radiate(*c.args())
        with pytest.raises(ClimaException, match=r"^ir_jacobian: the response form takes 4 <= nz <= 512 \(nz = %d\)$" % n):
            s.ir_jacobian_reduced(c["T_surface"], c["T"], np.arange(1, n + 2))
    big = S.modern_earth_tables(nw=9000, ng=16, nP=2, nT=2, ir_frac=0.5)
    b = Radtran(big, 4, 2, 0.3)
    nq = (len(big.ir_wavl) - 1) * 16
    assert nq > 65535
    with pytest.raises(ClimaException, match=r"^ir_jacobian: the response form takes at most 65535 \(bin, g-point\) pairs \(%d\)$" % nq):
        b.ir_jacobian_reduced(280.0, np.full(4, 250.0), np.arange(1, 6))


def _reduced_program():
    """tests/test_gpu_ir_jacobian.py's Fortran host up to its radiate call, then the reduced call with and without
    the optional arguments on a map read from the case's side file."""
    head, tail = FULL_PROGRAM.split("  allocate(ju(nz+1,nz+1), jd(nz+1,nz+1), jt(nz+1,nz+1))\n")
    head = head.replace("  real(dp), allocatable :: ju(:,:), jd(:,:), jt(:,:)\n",
                        "  real(dp), allocatable :: ju(:,:), jd(:,:), jt(:,:), jt2(:,:)\n"
                        "  integer, allocatable :: grp(:), rows(:)\n  integer :: ngroup, nrow\n  character(1024) :: fmap\n")
    head = head.replace("  call get_command_argument(2, fout)\n",
                        "  call get_command_argument(2, fout)\n  call get_command_argument(3, fmap)\n")
    body = """  open(newunit=u, file=trim(fmap), access='stream', form='unformatted', status='old')
  read(u) ngroup, nrow
  allocate(grp(nz+1), rows(nrow)); read(u) grp; read(u) rows
  close(u)
  allocate(ju(nrow,ngroup), jd(nrow,ngroup), jt(nrow,ngroup), jt2(nrow,ngroup))
  call rad%ir_jacobian_reduced(T_surface, T, grp, rows, jt, err, ju, jd); call check()
  call rad%ir_jacobian_reduced(T_surface, T, grp, rows, jt2, err); call check()
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) ju; write(u) jd; write(u) jt; write(u) jt2
  close(u)
  deallocate(jt); allocate(jt(nrow,ngroup+1))
  call rad%ir_jacobian_reduced(T_surface, T, grp, rows, jt, err)
  print '(a)', 'expected error: '//err
  call rad%ir_jacobian_reduced(T_surface, T, grp, rows, jt2, err, jac_up=ju)
  print '(a)', 'expected error: '//err
  call rad%destroy()
contains
  subroutine check()
    if (allocated(err)) then
      print '(a)', err
      error stop 1
    endif
  end subroutine
end program
"""
    return head + body


def test_fortran_ir_jacobian_reduced_matches_python(tmp_path):
    from clima_amd import build, synthetic as S
    from clima_amd.atmosphere import rce_jacobian_map
    from clima_amd.fortran_case import write_case
    from clima_amd.radtran import Radtran
    if not os.path.exists(build.FLANG):
        pytest.skip("amdflang is not available on this box")
    build.build()
    tb = S.modern_earth_tables(nw=30)
    nz, nzen, albedo = 40, 4, 0.15
    col = S.modern_earth_column(nz)
    group, rows, inds = rce_jacobian_map(19, np.arange(19) < 5)
    case, res, fmap = str(tmp_path / "case.bin"), str(tmp_path / "jac.bin"), str(tmp_path / "map.bin")
    write_case(case, tb, col, nzen, albedo)
    with open(fmap, "wb") as f:
        np.array([len(inds), len(rows)], dtype=np.int32).tofile(f)
        np.asarray(group, dtype=np.int32).tofile(f)
        np.asarray(rows, dtype=np.int32).tofile(f)
    src, exe = tmp_path / "jac.f90", str(tmp_path / "jac")
    src.write_text(_reduced_program())
    subprocess.check_call([build.FLANG, "-O2", "-J", str(tmp_path), os.path.join(build.FORTRAN_DIR, "clima_radtran_hip.f90"),
                           str(src), "-o", exe, "-L" + build.CSRC, "-lclima_radtran_hip", "-Wl,-rpath," + build.CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"], cwd=str(tmp_path))
    out = subprocess.run([exe, case, res, fmap], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expected error: jac has the wrong dimension" in out.stdout
    assert "expected error: ir_jacobian_reduced: jac_up and jac_dn go together: only jac_up was given" in out.stdout
    m = np.fromfile(res, dtype=np.float64).reshape(4, len(inds), len(rows))
    r = Radtran(tb, nz, nzen, albedo)
    r.radiate(*col.args())
    want = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows, parts=True)
    for i in range(3):
        np.testing.assert_array_equal(m[i].T, want[i])            # (Fortran order on disk: column g is row g here)
    np.testing.assert_array_equal(m[3].T, r.ir_jacobian_reduced(col["T_surface"], col["T"], group, rows))
