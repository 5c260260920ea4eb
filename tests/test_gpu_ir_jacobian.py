"""radtran_ir_jacobian: the exact IR temperature Jacobian of the level fluxes (the response form of ir_green.inc with the
Planck derivatives as amplitudes).  Held to the CPU yardstick built from the oracle's two-stream solver
(tests/ir_jacobian_oracle.py), to central differences through the library's own general batch kernel, and to itself
(repeatable, the handle's state untouched, communicator handles, refusals, the Fortran binding)."""
import os
import subprocess

import numpy as np
import pytest

import ir_jacobian_oracle as J

pytestmark = pytest.mark.gpu

# Tolerances, of the matrix's largest |value| (every entry).  Measured on an MI355X: 7e-12 - 1.9e-10 of the matrix
# maximum at the reference's ir_tau_min (1.2e-10 at 202 layers, 1.9e-10 with one g-point); per column, of the column's
# own maximum, the columns of the thin top layers -- whose largest entries are 1e-3 - 1e-7 of the matrix's -- agree to
# 3e-8 - 2e-5 only (the unit responses of a thin layer carry its source slope 1 / tau, in the response form as in
# two_stream_ir itself).  Both figures are printed.
TOL = 5.0e-10
TOL_THIN = 1.0e-7       # ir_tau_min = 1e-8 (measured: 1.2e-9 of the matrix maximum, 1.6e-5 of the worst column's own)


def _handle(tables, nz, hard=True, col=None, **scalars):
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, 2, 0.3)
    r.has_hard_surface = hard
    for k, v in scalars.items():
        setattr(r, k, v)
    col = col if col is not None else S.modern_earth_column(nz)
    r.radiate(*col.args())
    return r, col


def _yardstick(O, tables, r, col, cols=None):
    return J.exact_jacobian(O, tables, r.opr(), col["T_surface"], col["T"], r.surface_emissivity, r.has_hard_surface,
                            r.ir_tau_min, zenith_weights=r.zenith_weights, cols=cols)


def _worst(got, want, cols, label=""):
    """The largest error of the columns `cols` of the three matrices, of each matrix's largest |value|; the worst column
    of its own maximum is printed beside it."""
    cols = list(cols)
    by_matrix = max(float(np.max(np.abs(a[:, cols] - b[:, cols]))) / float(np.max(np.abs(b))) for a, b in zip(got, want))
    by_column = max(J.column_scaled_error(a, b, j) for a, b in zip(got, want) for j in cols)
    print("%s: %.1e of the matrix maximum, worst column %.1e of its own" % (label, by_matrix, by_column))
    return by_matrix


@pytest.fixture
def far_forms(hip_lib):
    """Both far-accumulation kernels: the matrix-core one (default) and the vector one."""
    import ctypes as C

    def set_form(v):
        hip_lib.clima_test_green_far_form_set(C.byref(C.c_int(v)))
    yield set_form
    set_form(0)


@pytest.mark.parametrize("nz", [4, 5, 30, 64, 102, 202])
@pytest.mark.parametrize("hard", [True, False])
def test_exact_jacobian_against_the_yardstick(O, small_tables, far_forms, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    em = np.linspace(0.65, 1.0, len(r.surface_emissivity))      # per-bin emissivity (read by the hard surface only)
    r.surface_emissivity = em
    want = _yardstick(O, small_tables, r, col)
    got = r.ir_jacobian(col["T_surface"], col["T"])
    for m in got:
        assert m.shape == (nz + 1, nz + 1) and m.flags.f_contiguous
    assert _worst(got, want, range(nz + 1), "nz %d hard %s" % (nz, hard)) <= TOL
    np.testing.assert_array_equal(got[2], got[1] - got[0])
    far_forms(1)
    vec = r.ir_jacobian(col["T_surface"], col["T"])
    far_forms(0)
    for a, b in zip(vec, got):
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


def test_exact_jacobian_402_layers(O, small_tables, far_forms):
    nz = 402
    r, col = _handle(small_tables, nz, True)
    cols = [0, 1, 2, nz // 2, nz // 2 + 1, nz - 1, nz]          # surface, bottom, middle, top, and neighbours
    want = _yardstick(O, small_tables, r, col, cols=cols)
    got = r.ir_jacobian(col["T_surface"], col["T"])
    assert _worst(got, want, cols, "nz 402") <= TOL
    far_forms(1)
    vec = r.ir_jacobian(col["T_surface"], col["T"])
    far_forms(0)
    for a, b in zip(vec, got):
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


@pytest.mark.parametrize("ng", [1, 4, 16])
def test_gauss_points_and_an_extreme_column(O, ng):
    from clima_amd import synthetic as S
    tables = S.modern_earth_tables(nw=30, ng=ng)
    nz = 40
    col = S.modern_earth_column(nz)
    r, col = _handle(tables, nz, True, col)
    hot = S.Column(col)
    hot["T"] = np.linspace(1500.0, 30.0, nz)                     # a 30 K top over a 1500 K surface
    hot["T_surface"] = 1500.0
    for c in (col, hot):
        got = r.ir_jacobian(c["T_surface"], c["T"])
        assert all(np.all(np.isfinite(m)) for m in got)
        want = _yardstick(O, tables, r, c)
        assert _worst(got, want, range(nz + 1), "ng %d" % ng) <= TOL


def test_thin_layers(O, small_tables):
    nz = 64
    r, col = _handle(small_tables, nz, True, ir_tau_min=1.0e-8)
    want = _yardstick(O, small_tables, r, col)
    got = r.ir_jacobian(col["T_surface"], col["T"])
    assert _worst(got, want, range(nz + 1), "ir_tau_min 1e-8") <= TOL_THIN


def test_against_central_differences_of_the_general_batch_kernel(small_tables):
    """The library's own batch with ir_green = 0 (one general solve per column) at dT = 1e-4 T.  Its error is the step's
    truncation (~1e-9) plus the cancellation of two level fluxes (~1e-13 of the fluxes over the step): a column that is
    itself a small part of the fluxes (a thin top layer) is held to the latter."""
    nz = 60
    r, col = _handle(small_tables, nz, True)
    jac = r.ir_jacobian(col["T_surface"], col["T"])
    x = np.concatenate([[col["T_surface"]], col["T"]])
    n = nz + 1
    h = 1.0e-4 * x
    X = np.repeat(x[:, None], 2 * n + 2, axis=1)
    for j in range(n):
        X[j, 2 * j] += h[j]
        X[j, 2 * j + 1] -= h[j]
    zone = [0, 1, 2, 3, 4]                                       # a convective zone: the surface and the four layers above
    d = 1.0e-4 * x[zone]
    X[zone, 2 * n] += d
    X[zone, 2 * n + 1] -= d
    r.ir_green = 0
    out = r.radiate_ir_batch(X[0], X[1:])
    assert r.ir_green_batches == 0
    scale = max(np.max(np.abs(out[0])), np.max(np.abs(out[1])))
    for m in range(3):
        for j in range(n):
            fd = (out[m][:, 2 * j] - out[m][:, 2 * j + 1]) / (2 * h[j])
            err = np.max(np.abs(fd - jac[m][:, j]))
            assert err <= 1e-5 * np.max(np.abs(jac[m][:, j])) + 1e-13 * scale / h[j], (m, j)
        fd = (out[m][:, 2 * n] - out[m][:, 2 * n + 1]) / 2.0       # directional derivative along d
        lin = jac[m][:, zone] @ d
        assert np.max(np.abs(fd - lin)) <= 1e-5 * np.max(np.abs(lin))


def test_repeatable_and_the_handle_untouched(small_tables, far_forms):
    nz = 50
    r, col = _handle(small_tables, nz, True)
    T = np.repeat(np.asarray(col["T"], float)[:, None], 12, axis=1)
    Ts = np.full(12, float(col["T_surface"]))
    for c in range(12):
        T[(4 * c) % nz, c] += 0.3 + 0.05 * c
    before = {}
    for mode in (0, 2):
        r.ir_green = mode
        before[mode] = r.radiate_ir_batch(Ts, T)
    w_ir = [np.array(getattr(r.wrk_ir, a)) for a in ("fup_n", "fdn_n", "fup_a", "fdn_a")]
    w_sol = [np.array(getattr(r.wrk_sol, a)) for a in ("fup_n", "fdn_n", "fup_a", "fdn_a")]
    ft = np.array(r.f_total)
    a = r.ir_jacobian(col["T_surface"], col["T"])
    b = r.ir_jacobian(col["T_surface"], col["T"])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    for v, name in zip(w_ir, ("fup_n", "fdn_n", "fup_a", "fdn_a")):
        np.testing.assert_array_equal(np.array(getattr(r.wrk_ir, name)), v)
    for v, name in zip(w_sol, ("fup_n", "fdn_n", "fup_a", "fdn_a")):
        np.testing.assert_array_equal(np.array(getattr(r.wrk_sol, name)), v)
    np.testing.assert_array_equal(np.array(r.f_total), ft)
    for mode in (0, 2):
        r.ir_green = mode
        for x, y in zip(r.radiate_ir_batch(Ts, T), before[mode]):
            np.testing.assert_array_equal(x, y)


def test_communicator_handles(small_tables):
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    nz, W = 60, 3
    col = S.modern_earth_column(nz)
    ref, _ = _handle(small_tables, nz, True, col)
    want = ref.ir_jacobian(col["T_surface"], col["T"])

    one = Radtran(small_tables, nz, 2, 0.3)
    one.comm_init_rank(1, 0, Radtran.comm_unique_id())
    one.radiate(*col.args())
    n0 = one.comm()[2]
    got = one.ir_jacobian(col["T_surface"], col["T"])
    assert one.comm()[2] == n0 + 1                                 # one collective per call
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)

    parts = []
    for k in range(W):
        r = Radtran(small_tables, nz, 2, 0.3)
        r.comm_init_rank(1, 0, Radtran.comm_unique_id())
        r.set_bin_shard(k, W)
        r.radiate(*col.args())
        parts.append(r.ir_jacobian(col["T_surface"], col["T"]))
    for i in range(3):
        s = sum(p[i] for p in parts)
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
    z = empty.ir_jacobian(col["T_surface"], col["T"])
    for m in z:
        assert m.shape == (nz + 1, nz + 1) and not np.any(m)

    plain = Radtran(small_tables, nz, 2, 0.3)
    plain.set_bin_shard(0, 2)                                       # a shard without a communicator: nobody would reduce
    plain.radiate(*col.args())
    with pytest.raises(ClimaException, match="bin-sharded"):
        plain.ir_jacobian(col["T_surface"], col["T"])


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
    buf = [np.empty((nl, nl), order="F") for _ in range(3)]
    dp = C.POINTER(C.c_double)
    T = np.ascontiguousarray(col["T"], dtype=float)

    def call(handle, Ts, T, dim_T, d1, d2):
        L.radtran_ir_jacobian(handle, C.byref(C.c_double(Ts)), C.byref(C.c_int(dim_T)), T.ctypes.data_as(dp),
                              C.byref(C.c_int(d1)), C.byref(C.c_int(d2)), *[b.ctypes.data_as(dp) for b in buf], err)
        return err.value.decode()

    assert call(h, 280.0, T, nz, nl, nl) == "Radtran is not constructed"
    L.deallocate_radtran(h)
    r = Radtran(small_tables, nz, 2, 0.3)
    with pytest.raises(ClimaException, match="^ir_jacobian needs opacities: call radiate with compute_opacity first$"):
        r.ir_jacobian(col["T_surface"], col["T"])
    r.radiate(*col.args())
    assert call(r._ptr, 280.0, T, nz - 1, nl, nl) == '"T" has the wrong input dimension.'
    assert call(r._ptr, 280.0, T, nz, nl, nl - 1) == "jac has the wrong dimension"
    assert call(r._ptr, 280.0, T, nz, nl + 1, nl) == "jac has the wrong dimension"
    with pytest.raises(ClimaException, match='^"T" has the wrong input dimension.$'):
        r.ir_jacobian(col["T_surface"], col["T"][:-1])
    for bad in (np.nan, np.inf, 0.0, -5.0):
        with pytest.raises(ClimaException, match="finite and positive"):
            r.ir_jacobian(bad, col["T"])
        Tb = np.array(col["T"], float)
        Tb[3] = bad
        with pytest.raises(ClimaException, match="finite and positive"):
            r.ir_jacobian(col["T_surface"], Tb)
    for n in (3, 513):
        c = S.modern_earth_column(n)
        s = Radtran(small_tables, n, 2, 0.3)
        s.radiate(*c.args())
        with pytest.raises(ClimaException, match=r"^ir_jacobian: the response form takes 4 <= nz <= 512 \(nz = %d\)$" % n):
            s.ir_jacobian(c["T_surface"], c["T"])
    # more than 65535 (bin, g-point) pairs: 4 500 IR bins x 16 g-points (the refusal comes before any opacity is needed)
    big = S.modern_earth_tables(nw=9000, ng=16, nP=2, nT=2, ir_frac=0.5)
    b = Radtran(big, 4, 2, 0.3)
    nq = (len(big.ir_wavl) - 1) * 16
    assert nq > 65535
    with pytest.raises(ClimaException, match=r"^ir_jacobian: the response form takes at most 65535 \(bin, g-point\) pairs \(%d\)$" % nq):
        b.ir_jacobian(280.0, np.full(4, 250.0))


FORTRAN_PROGRAM = """program jac
  use clima_radtran_hip, only: Radtran, dp
  implicit none
  type(Radtran) :: rad
  character(:), allocatable :: err
  character(1024) :: fin, fout
  integer :: nz, nsp, np, nw, nzen, nk, nxs, has_cont, npart, n_ir, n_sol
  integer :: sp_ind, ng, npr, nT, xs_type, xdim, sp1, sp2, LH2O, p_ind, nrad, i, u
  real(dp) :: albedo, T_surface
  real(dp), allocatable :: wavl(:), weights(:), log10P(:), temp(:), log10k(:,:,:,:), xs0(:), xs1(:,:)
  real(dp), allocatable :: h2o(:,:), frn(:,:), radii_ax(:), w0(:,:), qext(:,:), gt(:,:)
  real(dp), allocatable :: ir_wavl(:), sol_wavl(:), photons(:)
  real(dp), allocatable :: T(:), P(:), densities(:,:), dz(:), pdensities(:,:), radii(:,:)
  real(dp), allocatable :: ju(:,:), jd(:,:), jt(:,:)
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) nz, nsp, np, nw, nzen
  read(u) albedo
  allocate(wavl(nw+1)); read(u) wavl
  call rad%begin(nz, nsp, np, wavl, err); call check()
  read(u) nk
  do i = 1, nk
    read(u) sp_ind, ng, npr, nT
    allocate(weights(ng), log10P(npr), temp(nT), log10k(ng,npr,nT,nw))
    read(u) weights; read(u) log10P; read(u) temp; read(u) log10k
    call rad%add_ktable(sp_ind, weights, log10P, temp, log10k, err); call check()
    deallocate(weights, log10P, temp, log10k)
  enddo
  read(u) nxs
  do i = 1, nxs
    read(u) xs_type, xdim, sp1, sp2, nT
    if (xdim == 0) then
      allocate(xs0(nw)); read(u) xs0
      call rad%add_xsection(xs_type, [sp1, sp2], xs_0d=xs0, err=err); call check()
      deallocate(xs0)
    else
      allocate(temp(nT), xs1(nT,nw)); read(u) temp; read(u) xs1
      call rad%add_xsection(xs_type, [sp1, sp2], temp=temp, log10_xs_1d=xs1, err=err); call check()
      deallocate(temp, xs1)
    endif
  enddo
  read(u) has_cont
  if (has_cont /= 0) then
    read(u) LH2O, nT
    allocate(temp(nT), h2o(nT,nw), frn(nT,nw)); read(u) temp; read(u) h2o; read(u) frn
    call rad%set_water_continuum(LH2O, temp, h2o, frn, err); call check()
  endif
  read(u) npart
  do i = 1, npart
    read(u) p_ind, nrad
    allocate(radii_ax(nrad), w0(nrad,nw), qext(nrad,nw), gt(nrad,nw))
    read(u) radii_ax; read(u) w0; read(u) qext; read(u) gt
    call rad%add_particle(p_ind, radii_ax, w0, qext, gt, err); call check()
    deallocate(radii_ax, w0, qext, gt)
  enddo
  read(u) n_ir; allocate(ir_wavl(n_ir)); read(u) ir_wavl
  read(u) n_sol; allocate(sol_wavl(n_sol)); read(u) sol_wavl
  call rad%set_channels(ir_wavl, sol_wavl, err); call check()
  allocate(photons(n_sol-1)); read(u) photons
  call rad%set_photons_sol(photons, err); call check()
  call rad%finish(nzen, albedo, err); call check()
  allocate(T(nz), P(nz), densities(nz,nsp), dz(nz), pdensities(nz,np), radii(nz,np))
  read(u) T_surface; read(u) T; read(u) P; read(u) densities; read(u) dz
  if (np > 0) then
    read(u) pdensities; read(u) radii
  endif
  close(u)
  if (np > 0) then
    call rad%radiate(T_surface, T, P, densities, dz, pdensities, radii, err=err)
  else
    call rad%radiate(T_surface, T, P, densities, dz, err=err)
  endif
  call check()
  allocate(ju(nz+1,nz+1), jd(nz+1,nz+1), jt(nz+1,nz+1))
  call rad%ir_jacobian(T_surface, T, ju, jd, jt, err); call check()
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) ju; write(u) jd; write(u) jt
  close(u)
  deallocate(ju); allocate(ju(nz,nz+1))
  call rad%ir_jacobian(T_surface, T, ju, jd, jt, err)
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


def test_fortran_ir_jacobian_matches_python(tmp_path):
    from clima_amd import build, synthetic as S
    from clima_amd.fortran_case import write_case
    from clima_amd.radtran import Radtran
    if not os.path.exists(build.FLANG):
        pytest.skip("amdflang is not available on this box")
    build.build()
    tb = S.modern_earth_tables(nw=30)
    nz, nzen, albedo = 40, 4, 0.15
    col = S.modern_earth_column(nz)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "jac.bin")
    write_case(case, tb, col, nzen, albedo)
    src, exe = tmp_path / "jac.f90", str(tmp_path / "jac")
    src.write_text(FORTRAN_PROGRAM)
    subprocess.check_call([build.FLANG, "-O2", "-J", str(tmp_path), os.path.join(build.FORTRAN_DIR, "clima_radtran_hip.f90"),
                           str(src), "-o", exe, "-L" + build.CSRC, "-lclima_radtran_hip", "-Wl,-rpath," + build.CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"], cwd=str(tmp_path))
    out = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expected error: jac has the wrong dimension" in out.stdout
    m = np.fromfile(res, dtype=np.float64).reshape(3, nz + 1, nz + 1)
    r = Radtran(tb, nz, nzen, albedo)
    r.radiate(*col.args())
    want = r.ir_jacobian(col["T_surface"], col["T"])
    for i in range(3):
        np.testing.assert_array_equal(m[i].T, want[i])            # (Fortran order on disk: column j is row j here)
