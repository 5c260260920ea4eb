"""radtran_ir_jacobian_spectral_rows: rows of the IR temperature Jacobian before the sum over the bins, by one adjoint
two-stream solve per (bin, g-point, row, direction) (clima_amd/csrc/ir_adjoint.inc).  Held to the per-bin CPU yardstick
built from the oracle's two-stream solver (tests/ir_jacobian_spectral_oracle.py), to the library's own bin-summed
Jacobian, to central differences through the library's own IR-only call, to exact closed forms at the hook's level, and
to itself (exact zeros, switches, repeatable, the handle's state untouched, refusals, the Fortran binding)."""
import ctypes as C
import os
import subprocess

import mpmath
import numpy as np
import pytest

import closed_forms as CF
import ir_jacobian_oracle as J
import ir_jacobian_spectral_oracle as JS

pytestmark = pytest.mark.gpu

# Tolerances.  Every bin is compared on ITS scale: the largest |entry| of the bin's two full (nz+1) x (nz+1) matrices
# (never the row's own maximum: rows such as fdn near the top are 1e-4 and less of it, and the source slope 1 / tau of
# thin layers costs both sides digits -- tests/test_gpu_ir_jacobian.py says the same of the response form).
# Measured on an MI355X, test 1 (nz: hard surface / none):  4: 2.4e-10 / 4.1e-11   5: 4.5e-10 / 2.5e-11   31: 1.5e-10 /
# 1.1e-10   32: 1.8e-10 / 1.2e-10   33: 1.4e-10 / 1.1e-10   64: 2.6e-10 / 1.9e-10   65: 2.0e-10 / 1.2e-10   130: 2.5e-10 /
# 1.7e-10; 402 layers (test 9): 7.2e-11; the hook at 1, 12, 16, 32 g-points (test 7): 1.5e-10 / 9.9e-11.  The bound is
# 5 times the worst of test 1.  A CPU restatement of the same algebra (a serial sweep in numpy) sits 0.9e-10 - 5.0e-10
# from the oracle on these columns: the conditioning's floor, and the device's figures lie inside it.  Against the
# library's own bin-summed Jacobian (test 2): 2.1e-11 - 3.8e-11 of the matrix maximum.
MEASURED_YARD = 4.53e-10
TOL_YARD = 5.0 * MEASURED_YARD
TOL_J = 5.0e-10          # tests/test_gpu_ir_jacobian.py's, of the matrix maximum
# The hook against exact closed forms (w0 = 0, test 6): the kernel's own error.  Measured: 1.8e-16 at 3 layers (all of
# them at or below tau_min: no source slope), 4.3e-11 at 33 and 5.8e-11 at 65 layers, whose thinnest layer above tau_min
# has tau = 3e-6 and with it a source slope 1 / tau = 3e5 times an ulp.  The bound is 5 times the worst.
MEASURED_CLOSED = 5.81e-11
TOL_CLOSED = 5.0 * MEASURED_CLOSED

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _handle(tables, nz, hard=True, col=None, **scalars):
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, 2, 0.3)
    r.has_hard_surface = hard
    for k, v in scalars.items():
        setattr(r, k, v)
    r.surface_emissivity = np.linspace(0.65, 1.0, len(r.surface_emissivity))   # per bin (read by the hard surface only)
    col = col if col is not None else S.modern_earth_column(nz)
    r.radiate(*col.args())
    return r, col


def _yardstick(O, tables, r, col, cols=None, bins=None):
    return JS.spectral_jacobian(O, tables, r.opr(), col["T_surface"], col["T"], r.surface_emissivity, r.has_hard_surface,
                                r.ir_tau_min, zenith_weights=r.zenith_weights, cols=cols, bins=bins)


def _rows(nz):
    """top, one below, middle, one above the surface, surface, and a repeat: levels 1..nz+1, ground-first"""
    return [nz + 1, nz, nz // 2 + 1, 2, 1, nz + 1]


def _per_bin_worst(got, yard, rows, cols=None, bins=None):
    """the largest |got - yardstick| of the rows (both directions), every bin on its own scale"""
    up, dn, scale = yard
    cols = slice(None) if cols is None else list(cols)
    bins = list(range(up.shape[0])) if bins is None else list(bins)
    worst = 0.0
    for name, want in (("up", up), ("dn", dn)):
        for b, ll in enumerate(bins):
            for a, v in enumerate(rows):
                e = np.max(np.abs(got[name][ll, a, cols] - want[b, v - 1, cols])) / scale[b]
                worst = max(worst, float(e))
    return worst


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("nz", [4, 5, 31, 32, 33, 64, 65, 130])
@pytest.mark.parametrize("hard", [True, False])
def test_1_against_the_yardstick(O, small_tables, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    rows = _rows(nz)
    got = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[v - 1 for v in rows], parts=("up", "dn"))
    nw_ir = len(r.ir.freq) - 1
    for m in got.values():
        assert m.shape == (nw_ir, len(rows), nz + 1) and m.flags.f_contiguous and np.all(np.isfinite(m))
    worst = _per_bin_worst(got, _yardstick(O, small_tables, r, col), rows)
    print("nz %d hard %s: %.2e of the bin's matrix maximum [%.1e]" % (nz, hard, worst, TOL_YARD))
    assert worst <= TOL_YARD


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("nz", [30, 65])
def test_2_bins_times_widths_sum_to_the_librarys_jacobian(small_tables, nz):
    r, col = _handle(small_tables, nz, True)
    rows = _rows(nz)
    got = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[v - 1 for v in rows], parts=("up", "dn"))
    jac = r.ir_jacobian(col["T_surface"], col["T"])
    df = np.asarray(r.ir.freq, float)
    df = df[:-1] - df[1:]
    for name, full in (("up", jac[0]), ("dn", jac[1])):
        s = np.zeros((len(rows), nz + 1))
        for l in range(len(df)):
            s += got[name][l] * df[l]
        e = np.max(np.abs(s - full[[v - 1 for v in rows], :])) / np.max(np.abs(full))
        print("nz %d %s: %.2e of the matrix maximum [%.1e]" % (nz, name, e, TOL_J + TOL_YARD))
        assert e <= TOL_J + TOL_YARD


# ------------------------------------------------------------------ 3
def test_3_exact_zeros_and_switches(small_tables):
    nz = 33
    r, col = _handle(small_tables, nz, True)
    Ts, T = col["T_surface"], col["T"]
    lv = [v - 1 for v in _rows(nz)]
    both = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    assert np.all(both["dn"][:, 0, :] == 0.0) and np.all(both["dn"][:, 5, :] == 0.0)     # fdn(1) = 0 at the top
    assert np.any(both["dn"][:, 1, :] != 0.0) and np.all(np.any(both["up"] != 0.0, axis=(0, 2)))
    for name in ("up", "dn"):                                                               # a repeated level
        assert both[name][:, 0, :].tobytes() == both[name][:, 5, :].tobytes()
    again = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    for name in ("up", "dn"):
        assert again[name].tobytes() == both[name].tobytes()
    up = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up",))
    dn = r.ir_jacobian_spectral(Ts, T, levels=lv, parts="dn")
    assert list(up) == ["up"] and list(dn) == ["dn"]
    assert up["up"].tobytes() == both["up"].tobytes() and dn["dn"].tobytes() == both["dn"].tobytes()
    assert r.ir_jacobian_spectral(Ts, T)["up"].tobytes() == np.asfortranarray(both["up"][:, :1, :]).tobytes()   # the default: TOA, up
    # without a hard surface the emissivity is not read
    r.has_hard_surface = False
    a = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    r.surface_emissivity = np.linspace(0.2, 0.4, len(r.surface_emissivity))
    b = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    for name in ("up", "dn"):
        assert a[name].tobytes() == b[name].tobytes()
    assert a["up"].tobytes() != both["up"].tobytes()                                        # (the other surface form did run)


# ------------------------------------------------------------------ 4
def test_4_central_differences_through_the_library(small_tables):
    """radiate(compute_solar=False, compute_opacity=False) at x(j) +- 1e-4 x(j): the step's truncation (~1e-9) plus the
    cancellation of two per-bin fluxes (~1e-13 of the fluxes over the step), the form and figures of
    tests/test_gpu_ir_jacobian.py's central differences."""
    nz = 30
    r, col = _handle(small_tables, nz, True)
    r.ir_green = 0
    rows = _rows(nz)[:5]
    got = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[v - 1 for v in rows], parts=("up", "dn"))
    x = np.concatenate([[col["T_surface"]], col["T"]])
    xs = [0, 1, nz // 2, nz // 2 + 1, nz - 1, nz]               # surface, bottom, two middle, the two (thin) top layers
    for j in xs:
        h = 1.0e-4 * x[j]
        spec = []
        for s in (+1, -1):
            r.radiate(*J.perturbed(col, j, s * h).args(), compute_solar=False, compute_opacity=False)
            spec.append((np.array(r.wrk_ir.fup_a), np.array(r.wrk_ir.fdn_a)))
        scale = max(np.max(np.abs(spec[0][0])), np.max(np.abs(spec[0][1])))
        for m, name in enumerate(("up", "dn")):
            for a, v in enumerate(rows):
                fd = (spec[0][m][v - 1, :] - spec[1][m][v - 1, :]) / (2 * h)
                slab = got[name][:, a, j]
                err = np.max(np.abs(fd - slab))
                assert err <= 1e-5 * np.max(np.abs(slab)) + 1e-13 * scale / h, (name, v, j, err)


# ------------------------------------------------------------------ 5
def test_5_the_handle_afterwards(small_tables):
    from test_gpu_batch_bounds import fields_of
    from test_gpu_entry_points import left_state
    nz = 50
    r, col = _handle(small_tables, nz, True)
    Ts, T = col["T_surface"], col["T"]
    r.radiate(*col.args(), compute_opacity=False)
    jac = r.ir_jacobian(Ts, T)
    before, fields, opr = left_state(r), fields_of(r), [np.array(a) for a in r.opr()]
    r.ir_jacobian_spectral(Ts, T, levels=[-1, 0, 7], parts=("up", "dn"))
    r.ir_jacobian_spectral(Ts, T)
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    for k, v in fields_of(r).items():
        assert v.tobytes() == fields[k].tobytes(), k
    for a, b in zip(r.opr(), opr):
        assert np.array(a).tobytes() == b.tobytes()
    r.radiate(*col.args(), compute_opacity=False)
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), ("the call after", k)
    for a, b in zip(r.ir_jacobian(Ts, T), jac):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 6, 7: the hook
def _hook(L, tau, w0, g, wbin, emis, hard, tau_min, levels):
    nz, ng, nr = len(tau), len(wbin), len(levels)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)   # noqa: E731
    tau, w0, g, wbin = c(tau), c(w0), c(g), c(wbin)
    par = c([emis, 1.0 if hard else 0.0, tau_min])
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    up, dn = np.full((nr, nz + 1), np.nan), np.full((nr, nz + 1), np.nan)
    err = C.create_string_buffer(1025)
    d = lambda a: a.ctypes.data_as(DP)   # noqa: E731
    L.clima_test_ir_adjoint(C.byref(C.c_int(nz)), C.byref(C.c_int(ng)), d(tau), d(w0), d(g), d(par), d(wbin), C.byref(C.c_int(nr)),
                            lv.ctypes.data_as(IP), d(up), d(dn), err)
    assert not err.value, err.value.decode()
    return up, dn


def _hook_levels(nz):
    return [0, 1, (nz + 1) // 2, nz - 1, nz, 0]          # TOA-first: top, one below, middle, one above the surface, surface, a repeat


def _wbin(ng):
    w = np.linspace(1.0, 3.0, ng) ** 2
    return w / w.sum()


@pytest.mark.parametrize("ng", [1, 8])
@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("nz", [3, 33, 65])
def test_6_hook_against_the_closed_forms(hip_lib, nz, hard, ng):
    """w0 = 0: two_stream_ir decouples into two sweeps (closed_forms.ir_sweep), linear in bplanck -- its value on unit
    vectors is the exact derivative.  One layer at tau_min exactly, one below it, and without a hard surface the bottom
    layer below it too (the b1_bot branch)."""
    tau_min, emis = 1.0e-6, 0.8
    tau = np.geomspace(3.0e-6, 2.5, nz)
    tau[0] = tau_min
    tau[1] = 0.3 * tau_min
    if not hard:
        tau[nz - 1] = 0.5 * tau_min
    wbin = _wbin(ng)
    levels = _hook_levels(nz)
    up, dn = _hook(hip_lib, tau, np.zeros(nz), np.zeros(nz), wbin, emis, hard, tau_min, levels)
    nl = nz + 1
    with mpmath.workdps(CF.DPS):
        trans = [mpmath.exp(-2 * mpmath.mpf(float(t))) for t in tau]
        wsum = sum(mpmath.mpf(float(w)) for w in wbin)
        ru, rd = np.zeros((nl, nl), dtype=np.longdouble), np.zeros((nl, nl), dtype=np.longdouble)   # [level, k]
        for k in range(nl):
            e = [mpmath.mpf(0)] * nl
            e[k] = mpmath.mpf(1)
            fu, fd = CF.ir_sweep(tau, e, emis, hard, tau_min, trans=trans)
            for lv in range(nl):
                ru[lv, k], rd[lv, k] = CF._ld(fu[lv] * wsum), CF._ld(fd[lv] * wsum)
    scale = max(np.max(np.abs(ru)), np.max(np.abs(rd)))
    worst = max(float(np.max(np.abs(up[a] - ru[lv])) / scale) for a, lv in enumerate(levels))
    worst = max(worst, max(float(np.max(np.abs(dn[a] - rd[lv])) / scale) for a, lv in enumerate(levels)))
    print("nz %d hard %s ng %d: %.2e of the matrices' maximum [%.1e]" % (nz, hard, ng, worst, TOL_CLOSED))
    assert worst <= TOL_CLOSED
    assert not np.any(dn[0]) and up[0].tobytes() == up[5].tobytes()


@pytest.mark.parametrize("ng", [1, 12, 16, 32])
def test_7_hook_other_gauss_point_counts(O, hip_lib, ng):
    nz, tau_min, emis = 33, 1.0e-6, 0.8
    rng = np.random.default_rng(5)
    tau = np.geomspace(2.0e-6, 4.0, nz) * rng.uniform(0.7, 1.3, nz)
    w0, g = rng.uniform(0.0, 0.95, nz), rng.uniform(-0.3, 0.8, nz)
    wbin = _wbin(ng)
    levels = _hook_levels(nz)
    for hard in (True, False):
        up, dn = _hook(hip_lib, tau, w0, g, wbin, emis, hard, tau_min, levels)
        ru, rd = JS.unit_responses(O, np.repeat(tau[:, None], ng, axis=1), np.repeat(w0[:, None], ng, axis=1), g, wbin, emis, hard, tau_min)
        scale = max(np.max(np.abs(ru)), np.max(np.abs(rd)))
        worst = max(max(np.max(np.abs(up[a] - ru[lv])), np.max(np.abs(dn[a] - rd[lv]))) / scale for a, lv in enumerate(levels))
        print("ng %d hard %s: %.2e of the matrices' maximum [%.1e]" % (ng, hard, worst, TOL_YARD))
        assert worst <= TOL_YARD


# ------------------------------------------------------------------ 8
def test_8_refusals(hip_lib, small_tables):
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    from test_gpu_entry_points import configure, left_state
    import launch_forms as LF
    nz = 10
    nl = nz + 1
    col = S.modern_earth_column(nz)
    L = hip_lib
    err = C.create_string_buffer(1025)
    T = np.ascontiguousarray(col["T"], dtype=float)
    nw_ir = len(small_tables.ir_wavl) - 1
    nr = 2
    bufs = [np.full((nw_ir, nr, nl), 7.0, order="F") for _ in range(2)]
    lv = np.array([nl, 1], dtype=np.int32)

    def call(handle, Ts=280.0, T=T, dim_T=nz, nrow=nr, level=lv, d1=nw_ir, d2=nr, d3=nl, up=bufs[0], dn=bufs[1]):
        i = lambda v: C.byref(C.c_int(v))   # noqa: E731
        L.radtran_ir_jacobian_spectral_rows(handle, C.byref(C.c_double(Ts)), i(dim_T), T.ctypes.data_as(DP), i(nrow),
                                            level.ctypes.data_as(IP) if level is not None else None, i(d1), i(d2), i(d3),
                                            up.ctypes.data_as(DP) if up is not None else None,
                                            dn.ctypes.data_as(DP) if dn is not None else None, err)
        return err.value.decode()

    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    assert call(h) == "Radtran is not constructed"
    L.deallocate_radtran(h)
    r = Radtran(small_tables, nz, 2, 0.3)                         # a fresh handle
    with pytest.raises(ClimaException, match="^ir_jacobian_spectral_rows needs opacities: call radiate with compute_opacity first$"):
        r.ir_jacobian_spectral(col["T_surface"], col["T"])
    r.radiate(*col.args())
    before = left_state(r)
    who = "ir_jacobian_spectral_rows: "
    assert call(r._ptr, dim_T=nz - 1) == '"T" has the wrong input dimension.'
    for kw in (dict(d1=nw_ir + 1), dict(d2=nr + 1), dict(d3=nz)):
        assert call(r._ptr, **kw).startswith(who + "jac has the wrong dimension (%d, %d, %d)" % (kw.get("d1", nw_ir), kw.get("d2", nr), kw.get("d3", nl)))
    assert call(r._ptr, nrow=0, d2=0) == who + "nrow must be at least 1 (nrow = 0)"
    assert call(r._ptr, level=None) == who + '"row_level" is a required argument'
    assert call(r._ptr, level=np.array([1, 0], dtype=np.int32)) == who + "row_level(2) = 0 is outside 1..%d" % nl
    assert call(r._ptr, level=np.array([nz + 2, 1], dtype=np.int32)) == who + "row_level(1) = %d is outside 1..%d" % (nz + 2, nl)
    assert call(r._ptr, up=None, dn=None) == who + "neither jac_up_a nor jac_dn_a was given"
    assert call(r._ptr, Ts=float("nan")).startswith(who + "temperatures must be finite and positive (T_surface = nan")
    Tb = T.copy()
    Tb[3] = -5.0
    assert call(r._ptr, T=Tb).startswith(who + "temperatures must be finite and positive (T(4) = -5.0")
    assert all(np.all(b == 7.0) for b in bufs)                   # nothing was written
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert call(r._ptr) == ""                                     # the handle is usable afterwards
    assert call(r._ptr, dn=None) == "" and call(r._ptr, up=None) == ""
    with pytest.raises(ClimaException, match='"total" is not one of up, dn'):   # the Python checks come first
        r.ir_jacobian_spectral(col["T_surface"], col["T"], parts=("total",))
    with pytest.raises(ClimaException, match=r"levels\[0\] = %d is outside" % nl):
        r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[nl])
    # a bin shard, a communicator
    sh = Radtran(small_tables, nz, 2, 0.3)
    sh.radiate(*col.args())
    sh.set_bin_shard(0, 2)
    assert call(sh._ptr) == who + "needs the whole spectrum (a bin shard of 2)"
    cm = Radtran(small_tables, nz, 2, 0.3)
    cm.comm_init_rank(1, 0, Radtran.comm_unique_id())
    cm.radiate(*col.args())
    reduces = cm.comm()[2]
    assert call(cm._ptr) == who + "needs the whole spectrum (a communicator)"
    assert cm.comm()[2] == reduces
    cm.comm_destroy()
    # after a batch of one launch per chunk the handle's own block holds no opacities
    row = LF.BY_NAME["h100"]
    assert row.one_launch
    b = configure(row, row.make(Radtran))
    b.TOA_fluxes_batch(row.columns(4))
    c = row.column()
    with pytest.raises(ClimaException, match="^ir_jacobian_spectral_rows needs opacities"):
        b.ir_jacobian_spectral(c["T_surface"], c["T"])
    b.radiate(*c.args())
    assert np.all(np.isfinite(b.ir_jacobian_spectral(c["T_surface"], c["T"])["up"]))


# ------------------------------------------------------------------ 9
def test_9_402_layers(O, small_tables):
    nz = 402
    r, col = _handle(small_tables, nz, True)
    cols = [0, 1, 2, nz // 2, nz // 2 + 1, nz - 1, nz]          # surface, bottom, middle, top, and neighbours
    nw_ir = len(r.ir.freq) - 1
    bins = [0, nw_ir // 3, (2 * nw_ir) // 3, nw_ir - 1]
    rows = [nz + 1, 1]
    got = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[-1, 0], parts=("up", "dn"))
    worst = _per_bin_worst(got, _yardstick(O, small_tables, r, col, cols=cols, bins=bins), rows, cols=cols, bins=bins)
    print("nz 402: %.2e of the bin's maximum over the seven columns [%.1e]" % (worst, TOL_YARD))
    assert worst <= TOL_YARD


# ------------------------------------------------------------------ 10
FORTRAN_CALLS = """  allocate(ju3(n_ir-1,2,nz+1), jd3(n_ir-1,2,nz+1))
  call rad%ir_jacobian_spectral_rows(T_surface, T, [nz+1, 1], err, jac_up_a=ju3, jac_dn_a=jd3); call check()
  print '(a,2es24.16)', 'checksum ', sum(ju3), sum(jd3)
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) ju3; write(u) jd3
  close(u)
  call rad%ir_jacobian_spectral_rows(T_surface, T, [nz+2, 1], err, jac_up_a=ju3)
  print '(a)', 'expected error: '//err
"""


def test_10_fortran_binding_matches_python(tmp_path):
    from clima_amd import build, synthetic as S
    from clima_amd.fortran_case import write_case
    from clima_amd.radtran import Radtran
    from test_gpu_ir_jacobian import FORTRAN_PROGRAM
    if not os.path.exists(build.FLANG):
        pytest.skip("amdflang is not available on this box")
    build.build()
    head, rest = FORTRAN_PROGRAM.split("  allocate(ju(nz+1,nz+1)")
    tail = rest[rest.index("  call rad%destroy()"):]
    program = head.replace("ju(:,:), jd(:,:), jt(:,:)", "ju3(:,:,:), jd3(:,:,:)") + FORTRAN_CALLS + tail
    tb = S.modern_earth_tables(nw=30)
    nz, nzen, albedo = 40, 4, 0.15
    col = S.modern_earth_column(nz)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "rows.bin")
    write_case(case, tb, col, nzen, albedo)
    src, exe = tmp_path / "rows.f90", str(tmp_path / "rows")
    src.write_text(program)
    subprocess.check_call([build.FLANG, "-O2", "-J", str(tmp_path), os.path.join(build.FORTRAN_DIR, "clima_radtran_hip.f90"),
                           str(src), "-o", exe, "-L" + build.CSRC, "-lclima_radtran_hip", "-Wl,-rpath," + build.CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"], cwd=str(tmp_path))
    out = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expected error: ir_jacobian_spectral_rows: row_level(1) = %d is outside 1..%d" % (nz + 2, nz + 1) in out.stdout
    r = Radtran(tb, nz, nzen, albedo)
    r.radiate(*col.args())
    want = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=[-1, 0], parts=("up", "dn"))
    nw_ir = len(r.ir.freq) - 1
    m = np.fromfile(res, dtype=np.float64).reshape(2, nz + 1, 2, nw_ir)        # (Fortran order on disk)
    for i, name in enumerate(("up", "dn")):
        assert m[i].transpose(2, 1, 0).tobytes(order="F") == want[name].tobytes(order="F")
    sums = [float(v) for v in out.stdout.split("checksum")[1].split()[:2]]
    assert np.allclose(sums, [want["up"].sum(), want["dn"].sum()], rtol=1e-12)
