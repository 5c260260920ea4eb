"""radtran_ir_spectra_batch: per-bin IR spectra of many temperature profiles on one set of opacities, by the adjoint's
unit-amplitude rows (the weights W, clima_amd/csrc/ir_adjoint.inc) times the Planck values of each column
(clima_amd/csrc/ir_rows_apply.inc).  Held to the library's own IR-only call, to the CPU oracle's, to the exact sweeps at
w0 = 0, to a host sum of its own weights times Planck values, to the spectral rows of the Jacobian, and to itself (exact
zeros, independence of the other columns, repeatable, the handle's state untouched, refusals, every launch form, the
Fortran binding).

Error metric of the spectra: |got - want| per bin and column, over that column's largest level flux of that bin (both
directions, all levels); of fup_n / fdn_n: over the channel's largest level flux of the column."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import closed_forms as CF
import ir_jacobian_oracle as J
import ir_jacobian_spectral_oracle as JS
import ir_spectra_batch_oracle as SB

pytestmark = pytest.mark.gpu

# Tolerances.  MEASURED: the worst of test 1 on an MI355X; the bound is 5 x MEASURED, the project's convention (the margin
# covers other columns).  The CPU restatement of the identity (tests/test_ir_spectra_batch_host.py) sits up to 6.9e-10
# from the oracle: the conditioning floor of the method; a MEASURED above ten times that would be a defect, not a
# tolerance.
# Measured, test 1, spectra (nz: hard surface / none):  1: 1.6e-12 / 2.3e-12   4: 4.0e-10 / 2.9e-10   5: 6.1e-10 / 1.4e-9
# 63: 7.4e-10 / 3.8e-10   64: 1.1e-9 / 1.0e-9   65: 1.2e-9 / 6.3e-10   130: 8.5e-10 / 8.0e-10; fup_n / fdn_n: 8.8e-14 - 2.4e-10.
# Test 2 (the oracle): 8.0e-11 - 1.2e-9 where the library's own call is 4.9e-12 - 6.0e-10 from the oracle.  Test 6: 64 bins
# 1.0e-9, 65 bins 9.6e-10, 402 layers 1.0e-9.  Test 10, every launch form: 1.0e-13 - 4.4e-10.
# A random profile on which the REFERENCE call is ill-conditioned (see _columns) gives 1.8e-8 at nz = 5: such draws are
# skipped by a rule of the CPU oracle alone.
MEASURED = 1.44e-9
TOL = 5.0 * MEASURED
assert MEASURED <= 6.9e-9
# The apply kernel alone against math.fsum of w_up * planck on the host (test 4), over sum |terms|: a few ulps.  Measured:
# 2.5e-15 at 5 layers, 2.2e-15 at 65, 3.2e-15 at 130; the bound is 5 x the worst, and anything above 1e-13 is a defect.
# fup_n against fsum of fup times the widths: 3.6e-16, 5.0e-16, 4.7e-16.
MEASURED_APPLY = 3.18e-15
TOL_APPLY = 5.0 * MEASURED_APPLY
assert MEASURED_APPLY <= 1.0e-13
MEASURED_SUM = 5.01e-16
TOL_SUM = 5.0 * MEASURED_SUM

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


def _rows(nz):
    """top, one below, middle, one above the ground, ground, and a repeat: numpy-style indices, ground-first"""
    return [nz, max(nz - 1, 0), nz // 2, min(1, nz), 0, nz]


YARD_MAX = 6.9e-10            # the CPU floor of tests/test_ir_spectra_batch_host.py


def _yardsticks(O, tables, r, col):
    """the oracle in its two compilations (FMA contraction off / on) with the handle's settings and opacities of `col`"""
    out = []
    for variant in ("", "fma"):
        o = O.OracleRadtran(tables, r.nz, 2, 0.3, variant=variant)
        o.set_scalars(has_hard_surface=bool(r.has_hard_surface))
        o.set_surface_emissivity(np.asarray(r.surface_emissivity, dtype=float))
        o.radiate(*col.args())
        out.append(o)
    return out


def _columns(O, tables, r, col):
    """the base profile, two smooth perturbations, two random 150-350 K profiles: T_surface (5), T (nz, 5).

    The reference of tests 1, 2 and 6 is an IR-only CALL, and a call is itself ill-conditioned on some random profiles:
    steps of ~200 K across layers whose tau lies at ir_tau_min meet the source slope 1 / tau, and the oracle's two
    compilations then differ by up to 2.8e-8 of a bin's largest flux (nz = 5, hard surface, T = 232, 159, 160, 350, 280 K:
    the library's spectra and its own call differ by 1.8e-8 there, measured on an MI355X) -- no reference to hold anything
    to 3.5e-9 with.  So a random draw (default_rng(nz): T, then T_surface) is kept only where the reference can be
    trusted: where the oracle's two compilations agree to YARD_MAX per bin, a figure of the CPU alone.  Draws that are
    not are skipped and printed."""
    nz = r.nz
    rng = np.random.default_rng(nz)
    T0, Ts0 = np.asarray(col["T"], dtype=float), float(col["T_surface"])
    z = np.linspace(0.0, 1.0, nz)
    cols = [(Ts0, T0), (Ts0 + 4.0, T0 + 5.0 * np.cos(np.pi * z)), (Ts0 - 6.0, T0 * (1.0 - 0.04 * z) - 3.0)]
    oracles = _yardsticks(O, tables, r, col)
    for _ in range(40):
        T, Ts = rng.uniform(150.0, 350.0, nz), float(rng.uniform(150.0, 350.0))
        a, b = (SB.from_call(o, col, Ts, T) for o in oracles)
        yard = SB.per_bin_worst(b[0], b[1], a[0], a[1])
        if yard <= YARD_MAX:
            cols.append((Ts, T))
        else:
            print("nz %d: a draw skipped, the oracle's two compilations differ by %.2e on it" % (nz, yard))
        if len(cols) == 5:
            break
    assert len(cols) == 5
    return np.array([c[0] for c in cols]), np.asfortranarray(np.stack([c[1] for c in cols], axis=1))


def _ir_only(r, col, Ts, T):
    """the library's own IR-only call on column (Ts, T): fup_a, fdn_a (nw_ir, nz+1), fup_n, fdn_n (nz+1)"""
    from clima_amd import synthetic as S
    r.radiate(*S.Column(col, T=np.array(T, dtype=float), T_surface=float(Ts)).args(), compute_solar=False, compute_opacity=False)
    w = r.wrk_ir
    return np.array(w.fup_a).T.copy(), np.array(w.fdn_a).T.copy(), np.array(w.fup_n), np.array(w.fdn_n)


def _errors(got, want, lv, c):
    """(worst of the spectra, worst of the sums) of column c against `want` = _ir_only's tuple"""
    wu, wd, wun, wdn = want
    scale = np.maximum(np.max(np.abs(wu), axis=1), np.max(np.abs(wd), axis=1))
    e = 0.0
    if "fup" in got:
        e = max(e, float(np.max(np.max(np.abs(got["fup"][:, :, c] - wu[:, lv]), axis=1) / scale)))
    if "fdn" in got:
        e = max(e, float(np.max(np.max(np.abs(got["fdn"][:, :, c] - wd[:, lv]), axis=1) / scale)))
    sn = max(float(np.max(np.abs(wun))), float(np.max(np.abs(wdn))))
    en = 0.0
    if "fup_n" in got:
        en = max(en, float(np.max(np.abs(got["fup_n"][:, c] - wun[lv]))) / sn)
    if "fdn_n" in got:
        en = max(en, float(np.max(np.abs(got["fdn_n"][:, c] - wdn[lv]))) / sn)
    return e, en


def _against_the_single_call(r, col, Ts, T, lv, what):
    got = r.ir_spectra_batch(Ts, T, levels=lv, parts=("up", "dn"), fluxes=True)
    nw_ir, n = len(r.ir.freq) - 1, len(Ts)
    assert got["fup"].shape == got["fdn"].shape == (nw_ir, len(lv), n) and got["fup_n"].shape == got["fdn_n"].shape == (len(lv), n)
    for m in got.values():
        assert m.flags.f_contiguous and np.all(np.isfinite(m))
    worst = [0.0, 0.0]
    for c in range(n):
        e = _errors(got, _ir_only(r, col, Ts[c], T[:, c]), lv, c)
        worst = [max(a, b) for a, b in zip(worst, e)]
    print("%s: spectra %.2e, sums %.2e of the largest level flux [%.1e]" % (what, worst[0], worst[1], TOL))
    return got, worst


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("nz", [1, 4, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("hard", [True, False])
def test_01_against_the_librarys_ir_only_call(O, small_tables, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    Ts, T = _columns(O, small_tables, r, col)
    got, worst = _against_the_single_call(r, col, Ts, T, _rows(nz), "nz %d hard %s" % (nz, hard))
    assert max(worst) <= TOL


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("nz,hard", [(5, True), (64, False), (65, True)])
def test_02_against_the_cpu_oracle(O, small_tables, nz, hard):
    r, col = _handle(small_tables, nz, hard)
    Ts, T = _columns(O, small_tables, r, col)
    lv = _rows(nz)
    got = r.ir_spectra_batch(Ts, T, levels=lv, parts=("up", "dn"), fluxes=True)
    o = O.OracleRadtran(small_tables, nz, 2, 0.3)
    o.set_scalars(has_hard_surface=hard)
    o.set_surface_emissivity(np.asarray(r.surface_emissivity, dtype=float))
    o.radiate(*col.args())
    for c in range(len(Ts)):
        want = SB.from_call(o, col, Ts[c], T[:, c])
        own = _ir_only(r, col, Ts[c], T[:, c])                # the oracle-to-library distance on this column
        dist = max(_errors(dict(fup=own[0][:, lv, None], fdn=own[1][:, lv, None], fup_n=own[2][lv, None], fdn_n=own[3][lv, None]), want, lv, 0))
        e, en = _errors(got, want, lv, c)
        print("nz %d hard %s column %d: spectra %.2e, sums %.2e (library to oracle %.2e) [%.1e]" % (nz, hard, c, e, en, dist, TOL + dist))
        assert e <= TOL + dist and en <= TOL + dist


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["nz12", "nz65-thin"])
def test_03_pure_absorption_against_the_exact_sweep(O, hip_lib, name):
    """the cases, the columns and the tolerance rule of test_gpu_closed_forms.test_ir_batches_against_the_exact_sweep: the
    larger of TOL_LEVEL and 10 times the distance of the oracle's two compilations, per bin here"""
    from clima_amd import synthetic as S
    from test_gpu_closed_forms import _handle as closed_handle
    from test_gpu_parity import TOL_LEVEL
    case = CF.absorption_case(name)
    col, nz, ncol = case["column"], case["nz"], 4
    r = closed_handle(case["tables"], nz, case["nzen"], "coop-fused", case["scalars"], case["albedo"], case["emissivity"])
    r.radiate(*col.args())
    oracles = []
    for variant in ("", "fma"):
        o = O.OracleRadtran(case["tables"], nz, case["nzen"], 0.3, variant=variant)
        o.set_scalars(**case["scalars"])
        o.set_surface_emissivity(case["emissivity"])
        o.radiate(*col.args())
        oracles.append(o)
    tau, w0 = r.opr()[:2]
    assert np.all(w0 == 0.0)
    rng = np.random.default_rng(nz)
    T = np.repeat(np.asarray(col["T"], dtype=float)[:, None], ncol, axis=1)
    Ts = np.full(ncol, float(col["T_surface"]))
    for c in range(1, ncol):                               # column 0 is the profile itself
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(0, nz + 1))
            d = float(rng.choice([1e-3, 0.1, 3.0, 40.0])) * float(rng.choice([-1.0, 1.0]))
            if j == nz:
                Ts[c] += d
            else:
                T[j, c] += d
    lv = list(range(nz + 1))
    got = r.ir_spectra_batch(Ts, T, levels=lv, parts=("up", "dn"), fluxes=True)
    trans = CF.ir_transmissions(case["tables"], tau)
    s = case["scalars"]
    for c in range(ncol):
        ref = CF.ir_channel(case["tables"], tau, Ts[c], T[:, c], case["emissivity"], s["has_hard_surface"], s["ir_tau_min"], trans)
        w = S.Column(col)
        w["T"], w["T_surface"] = T[:, c].copy(), Ts[c]
        spec = []
        for o in oracles:
            o.radiate(*w.args(), compute_solar=False, compute_opacity=False)
            spec.append((np.array(o.wrk_ir.fup_a), np.array(o.wrk_ir.fdn_a), np.array(o.wrk_ir.fup_n), np.array(o.wrk_ir.fdn_n)))
        yard = CF.per_bin(spec[0][0], spec[0][1], spec[1][0], spec[1][1])
        e = CF.per_bin(got["fup"][:, :, c].T, got["fdn"][:, :, c].T, ref.fup_a, ref.fdn_a)
        bound = np.maximum(TOL_LEVEL, 10.0 * yard)
        scale = max(float(np.max(np.abs(ref.fup_n))), float(np.max(np.abs(ref.fdn_n))))
        yn = max(float(np.max(np.abs(spec[0][2] - spec[1][2]))), float(np.max(np.abs(spec[0][3] - spec[1][3])))) / scale
        en = max(float(np.max(np.abs(np.asarray(got["fup_n"][:, c], dtype=CF.LD) - ref.fup_n))),
                 float(np.max(np.abs(np.asarray(got["fdn_n"][:, c], dtype=CF.LD) - ref.fdn_n)))) / scale
        print("%s column %d: per bin %.2e (largest share of its bound %.3f), sums %.2e [%.1e]"
              % (name, c, e.max(), (e / bound).max(), en, max(TOL_LEVEL, 10.0 * yn)))
        assert np.all(e <= bound), (c, e, bound)
        assert en <= max(TOL_LEVEL, 10.0 * yn)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("nz", [5, 65, 130])
def test_04_the_apply_kernel_alone(O, small_tables, nz):
    """fup against math.fsum of w_up(l, a, j) planck(avg_freq(l), x_c(j)) on the host (closed_forms.planck at 50 digits,
    rounded), over the sum of |terms|; fup_n against fsum of fup times the bins' widths, over the sum of |terms|"""
    import mpmath
    r, col = _handle(small_tables, nz, True)
    Ts, T = _columns(O, small_tables, r, col)
    lv = _rows(nz)[:5]
    got = r.ir_spectra_batch(Ts, T, levels=lv, parts=("up",), fluxes=True, weights=True)
    ir_start, freq, ir_freq = JS.channel(small_tables)
    df = JS.dfreq(small_tables)
    nw_ir = len(df)
    worst = worst_n = 0.0
    for c in range(len(Ts)):
        x = np.concatenate([[Ts[c]], T[:, c]])
        with mpmath.workdps(CF.DPS):
            B = np.array([[float(CF.planck(mpmath.mpf(float(0.5 * (freq[ir_start + l] + freq[ir_start + l + 1]))), float(t))) for t in x]
                          for l in range(nw_ir)])
        for a in range(len(lv)):
            for l in range(nw_ir):
                terms = got["w_up"][l, a, :] * B[l]
                worst = max(worst, abs(got["fup"][l, a, c] - math.fsum(terms)) / math.fsum(np.abs(terms)))
            terms = got["fup"][:, a, c] * df
            worst_n = max(worst_n, abs(got["fup_n"][a, c] - math.fsum(terms)) / math.fsum(np.abs(terms)))
    print("nz %d: apply %.2e of sum |terms| [%.1e], sums over the bins %.2e [%.1e]" % (nz, worst, TOL_APPLY, worst_n, TOL_SUM))
    assert worst <= TOL_APPLY and worst_n <= TOL_SUM


# ------------------------------------------------------------------ 5
def test_05_exact_properties(small_tables):
    nz = 33
    r, col = _handle(small_tables, nz, True)
    lv = _rows(nz)
    rng = np.random.default_rng(37)
    n = 37
    T = np.asfortranarray(np.asarray(col["T"], dtype=float)[:, None] + rng.uniform(-20.0, 20.0, (nz, n)))
    Ts = float(col["T_surface"]) + rng.uniform(-20.0, 20.0, n)
    kw = dict(levels=lv, parts=("up", "dn"), fluxes=True, weights=True)
    both = r.ir_spectra_batch(Ts, T, **kw)
    names = ("fup", "fdn", "fup_n", "fdn_n", "w_up", "w_dn")
    assert sorted(both) == sorted(names)
    # fdn at the top of the atmosphere is the constant 0 (level nz+1: rows 0 and 5)
    for a in (0, 5):
        assert np.all(both["fdn"][:, a, :] == 0.0) and np.all(both["fdn_n"][a, :] == 0.0) and np.all(both["w_dn"][:, a, :] == 0.0)
    assert np.all(np.any(both["fdn"][:, 1:5, :] != 0.0, axis=0)) and np.all(both["fup"] > 0.0)
    # a repeated level
    for k in names:
        m = both[k]
        assert (m[0] if m.ndim == 2 else m[:, 0]).tobytes() == (m[5] if m.ndim == 2 else m[:, 5]).tobytes(), k
    # bitwise repeatable
    again = r.ir_spectra_batch(Ts, T, **kw)
    for k in names:
        assert again[k].tobytes() == both[k].tobytes(), k
    # a column does not depend on ncol or on the other columns (37 columns: tiles of 4 and a tail; 3 and 1: tiles of 1)
    for c in (0, 17, 35, 36):
        alone = r.ir_spectra_batch(Ts[c], T[:, c], **kw)
        three = r.ir_spectra_batch(Ts[[c, 1, 2]], T[:, [c, 1, 2]], **kw)
        for k in ("fup", "fdn"):
            want = np.ascontiguousarray(both[k][:, :, c]).tobytes()
            assert np.ascontiguousarray(alone[k][:, :, 0]).tobytes() == want, (k, c)
            assert np.ascontiguousarray(three[k][:, :, 0]).tobytes() == want, (k, c)
        for k in ("fup_n", "fdn_n"):
            want = np.ascontiguousarray(both[k][:, c]).tobytes()
            assert np.ascontiguousarray(alone[k][:, 0]).tobytes() == want and np.ascontiguousarray(three[k][:, 0]).tobytes() == want, (k, c)
        for k in ("w_up", "w_dn"):
            assert alone[k].tobytes() == both[k].tobytes()
    # outputs do not depend on which other outputs were asked for
    for parts, fluxes, weights in ((("up",), False, False), ("dn", False, False), (("up",), True, False), (("dn",), True, True),
                                   (("up", "dn"), False, False), (("up", "dn"), False, True)):
        part = r.ir_spectra_batch(Ts, T, levels=lv, parts=parts, fluxes=fluxes, weights=weights)
        for k, m in part.items():
            assert m.tobytes() == both[k].tobytes(), (parts, fluxes, weights, k)
    assert r.ir_spectra_batch(Ts, T)["fup"].tobytes() == np.asfortranarray(both["fup"][:, :1, :]).tobytes()   # the default: TOA, up
    only_w = r.ir_spectra_batch(None, None, levels=lv, parts=("up", "dn"), weights=True)                      # no columns
    assert sorted(only_w) == ["w_dn", "w_up"] and all(only_w[k].tobytes() == both[k].tobytes() for k in only_w)
    # fewer and more functionals per pass than 8: the same rows
    for levels in (lv[:1], lv[:3], list(range(nz + 1))):       # 2, 6 and 68 functionals: passes of 2; 4 + 2; 8 x 8 + 4
        part = r.ir_spectra_batch(Ts[:5], T[:, :5], levels=levels, parts=("up", "dn"))
        for a, v in enumerate(levels):
            if v in lv:
                for k in ("fup", "fdn"):
                    assert np.ascontiguousarray(part[k][:, a, :]).tobytes() == np.ascontiguousarray(both[k][:, lv.index(v), :5]).tobytes(), (len(levels), k, a)
    # without a hard surface the emissivity is not read
    r.has_hard_surface = False
    a = r.ir_spectra_batch(Ts, T, **kw)
    r.surface_emissivity = np.linspace(0.2, 0.4, len(r.surface_emissivity))
    b = r.ir_spectra_batch(Ts, T, **kw)
    for k in names:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["fup"].tobytes() != both["fup"].tobytes()                                        # (the other surface form did run)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("nw,bins", [(106, 64), (108, 65)])
def test_06_bin_lane_edges(O, nw, bins):
    from clima_amd import synthetic as S
    tables = S.modern_earth_tables(nw=nw)
    assert len(tables.ir_wavl) - 1 == bins
    nz = 33
    r, col = _handle(tables, nz, True)
    Ts, T = _columns(O, tables, r, col)
    got, worst = _against_the_single_call(r, col, Ts[[0, 3, 4]], np.asfortranarray(T[:, [0, 3, 4]]), _rows(nz), "%d IR bins" % bins)
    assert max(worst) <= TOL


def test_06_sixteen_g_points(O):
    from clima_amd import synthetic as S
    tables = S.make_tables(nw=40, ng=16)
    nz = 33
    r, col = _handle(tables, nz, True)
    assert len(tables.ktables[0]["weights"]) == 16
    Ts, T = _columns(O, tables, r, col)
    got, worst = _against_the_single_call(r, col, Ts[[0, 3, 4]], np.asfortranarray(T[:, [0, 3, 4]]), _rows(nz), "16 g-points")
    assert max(worst) <= TOL


def test_06_402_layers(O, small_tables):
    from clima_amd import synthetic as S
    col = S.doubled_column(S.modern_earth_column(201))
    nz = len(col["T"])
    assert nz == 402
    r, col = _handle(small_tables, nz, True, col=col)
    Ts, T = _columns(O, small_tables, r, col)
    got, worst = _against_the_single_call(r, col, Ts[[0, 1, 3]], np.asfortranarray(T[:, [0, 1, 3]]), [nz, nz // 2, 0], "402 layers")
    assert max(worst) <= TOL


# ------------------------------------------------------------------ 7
def test_07_weights_times_dplanck_are_the_spectral_rows(small_tables):
    nz = 40
    r, col = _handle(small_tables, nz, True)
    lv = _rows(nz)
    Ts, T = float(col["T_surface"]), np.asarray(col["T"], dtype=float)
    w = r.ir_spectra_batch(None, None, levels=lv, parts=("up", "dn"), weights=True)
    jac = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    ir_start, freq, ir_freq = JS.channel(small_tables)
    x = np.concatenate([[Ts], T])
    for l in range(len(ir_freq) - 1):
        amp = J.dplanck_dT(0.5 * (freq[ir_start + l] + freq[ir_start + l + 1]), x)
        for name in ("up", "dn"):
            for a in range(len(lv)):
                got, want = w["w_" + name][l, a, :] * amp, jac[name][l, a, :]
                assert np.max(np.abs(got - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300), (l, name, a)


# ------------------------------------------------------------------ 8
def test_08_the_handle_afterwards(small_tables):
    from test_gpu_batch_bounds import fields_of
    from test_gpu_entry_points import ir_batch_columns, left_state
    from test_gpu_merged_integration import _assert_same_state
    nz = 50
    r, col = _handle(small_tables, nz, True)
    Ts, T = ir_batch_columns(col, nz)
    T = np.asfortranarray(T)
    r.radiate(*col.args(), compute_opacity=False)
    before, fields, opr = left_state(r), fields_of(r), [np.array(a) for a in r.opr()]
    first = r.ir_spectra_batch(Ts, T, levels=[-1, 0, 7], parts=("up", "dn"), fluxes=True, weights=True)
    r.ir_spectra_batch(Ts, T)
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    for k, v in fields_of(r).items():
        assert v.tobytes() == fields[k].tobytes(), k
    for a, b in zip(r.opr(), opr):
        assert np.array(a).tobytes() == b.tobytes()
    r.radiate(*col.args(), compute_opacity=False)           # a following single call is unaffected
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), ("the call after", k)
    # a pending deferred integration is settled first, and correctly
    from clima_amd.radtran import Radtran
    pair = []
    for defer in (True, False):
        h = Radtran(small_tables, nz, 2, 0.3)
        h.surface_emissivity = np.asarray(r.surface_emissivity, dtype=float)
        h.defer_integration = defer
        h.upload_column(*col.args())
        h.radiate_resident()
        got = h.ir_spectra_batch(Ts, T, levels=[-1, 0, 7], parts=("up", "dn"), fluxes=True, weights=True)
        for k in first:
            assert got[k].tobytes() == first[k].tobytes(), (defer, k)
        h.synchronize()
        pair.append(h)
    _assert_same_state(pair[0], pair[1], "deferring against not, a spectra batch in between")
    for k, v in left_state(pair[0]).items():
        if k.startswith("sol_") or k == "ir_tau_band":
            assert v.tobytes() == before[k].tobytes(), k


# ------------------------------------------------------------------ 9
def test_09_refusals(hip_lib, small_tables):
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    from test_gpu_entry_points import configure, left_state
    import launch_forms as LF
    nz, n, nsel = 10, 3, 2
    nl = nz + 1
    col = S.modern_earth_column(nz)
    L = hip_lib
    err = C.create_string_buffer(1025)
    T = np.asfortranarray(np.repeat(np.asarray(col["T"], dtype=float)[:, None], n, axis=1))
    Ts = np.full(n, float(col["T_surface"]))
    nw_ir = len(small_tables.ir_wavl) - 1
    bufs = dict(fup=np.full((nw_ir, nsel, n), 7.0, order="F"), fdn=np.full((nw_ir, nsel, n), 7.0, order="F"),
                fup_n=np.full((nsel, n), 7.0, order="F"), fdn_n=np.full((nsel, n), 7.0, order="F"),
                w_up=np.full((nw_ir, nsel, nl), 7.0, order="F"), w_dn=np.full((nw_ir, nsel, nl), 7.0, order="F"))
    lv = np.array([nl, 1], dtype=np.int32)
    ALL = tuple(bufs)

    def call(handle, ncol=n, Ts=Ts, T=T, dim1=nz, dim2=n, nsel=nsel, level=lv, outs=ALL):
        i = lambda v: C.byref(C.c_int(v))   # noqa: E731
        p = lambda a: a.ctypes.data_as(DP) if a is not None else None   # noqa: E731
        L.radtran_ir_spectra_batch(handle, i(ncol), p(Ts), i(dim1), i(dim2), p(T), i(nsel),
                                   level.ctypes.data_as(IP) if level is not None else None,
                                   *[p(bufs[k]) if k in outs else None for k in ALL], err)
        return err.value.decode()

    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    assert call(h) == "Radtran is not constructed"
    L.deallocate_radtran(h)
    r = Radtran(small_tables, nz, 2, 0.3)                         # a fresh handle
    with pytest.raises(ClimaException, match="^ir_spectra_batch needs opacities: call radiate with compute_opacity first$"):
        r.ir_spectra_batch(Ts, T)
    r.radiate(*col.args())
    before = left_state(r)
    who = "ir_spectra_batch: "
    assert call(r._ptr, dim1=nz - 1) == '"T" has the wrong input dimension.'
    assert call(r._ptr, dim2=n + 1) == '"T" has the wrong input dimension.'
    assert call(r._ptr, ncol=-1, dim2=-1) == who + "ncol must not be negative (ncol = -1)"
    assert call(r._ptr, ncol=0, dim2=0) == who + "ncol = 0 gives the weights alone, but ir_fup was asked for"
    assert call(r._ptr, ncol=0, dim2=0, outs=("w_up", "fdn_n")) == who + "ncol = 0 gives the weights alone, but fdn_n was asked for"
    assert call(r._ptr, nsel=0) == who + "nsel must be at least 1 (nsel = 0)"
    assert call(r._ptr, level=None) == who + '"spec_level" is a required argument'
    assert call(r._ptr, level=np.array([1, 0], dtype=np.int32)) == who + "spec_level(2) = 0 is outside 1..%d" % nl
    assert call(r._ptr, level=np.array([nz + 2, 1], dtype=np.int32)) == who + "spec_level(1) = %d is outside 1..%d" % (nz + 2, nl)
    assert call(r._ptr, outs=()) == who + "none of ir_fup, ir_fdn, fup_n, fdn_n, w_up, w_dn was given"
    assert call(r._ptr, T=None) == who + '"T" is a required argument (ncol = 3)'
    assert call(r._ptr, Ts=None) == who + '"T_surface" is a required argument (ncol = 3)'
    Tb = Ts.copy()
    Tb[1] = float("nan")
    assert call(r._ptr, Ts=Tb).startswith(who + "temperatures must be finite and positive (T_surface(2) = nan")
    Tb = T.copy(order="F")
    Tb[3, 2] = -5.0
    assert call(r._ptr, T=Tb).startswith(who + "temperatures must be finite and positive (T(4, 3) = -5.0")
    Tb[3, 2] = float("inf")
    assert call(r._ptr, T=Tb).startswith(who + "temperatures must be finite and positive (T(4, 3) = inf")
    # the adjoint work buffer: 192 (bin, g-point) pairs x (4 + nfun) x 2 nz doubles pass 4 GiB near 90 000 (repeated) levels
    many = np.ones(100000, dtype=np.int32)
    assert call(r._ptr, nsel=len(many), level=many, outs=("fup_n",)).startswith(
        who + "the work buffer of nsel = 100000 levels in 1 direction(s) would take ")
    assert all(np.all(b == 7.0) for b in bufs.values())          # nothing was written
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert call(r._ptr) == ""                                     # the handle is usable afterwards
    assert not any(np.any(b == 7.0) for b in bufs.values())
    for outs in (("fup",), ("fdn_n",), ("w_dn",)):
        assert call(r._ptr, outs=outs) == ""
    assert call(r._ptr, ncol=0, dim2=0, Ts=None, T=None, outs=("w_up", "w_dn")) == ""      # the weights alone: T unread
    with pytest.raises(ClimaException, match='"total" is not one of up, dn'):   # the Python checks come first
        r.ir_spectra_batch(Ts, T, parts=("total",))
    with pytest.raises(ClimaException, match=r"levels\[0\] = %d is outside" % nl):
        r.ir_spectra_batch(Ts, T, levels=[nl])
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
    with pytest.raises(ClimaException, match="^ir_spectra_batch needs opacities"):
        b.ir_spectra_batch(c["T_surface"], c["T"])
    b.radiate(*c.args())
    assert np.all(np.isfinite(b.ir_spectra_batch(c["T_surface"], c["T"])["fup"]))


# ------------------------------------------------------------------ 10
import launch_forms as LF   # noqa: E402


@pytest.mark.parametrize("row", LF.ROWS, ids=repr)
def test_10_every_launch_form(row):
    from clima_amd.radtran import ClimaException, Radtran
    from test_gpu_entry_points import configure, ir_batch_columns
    r = configure(row, row.make(Radtran))
    col, nz = row.column(), row.nz
    r.radiate(*col.args())
    Ts, T = ir_batch_columns(col, nz)
    got, worst = _against_the_single_call(r, col, Ts, np.asfortranarray(T), [nz, nz // 2, 0], row.name)
    assert max(worst) <= TOL
    assert r.fused_fallbacks == 0
    if row.one_launch:
        r.TOA_fluxes_batch(row.columns(2))
        with pytest.raises(ClimaException, match="^ir_spectra_batch needs opacities"):
            r.ir_spectra_batch(Ts, T)


# ------------------------------------------------------------------ 11
FORTRAN_CALLS = """  allocate(Tc(nz,3), Tsc(3), su(n_ir-1,2,3), sd(n_ir-1,2,3), nu(2,3), nd(2,3), wu(n_ir-1,2,nz+1), wd(n_ir-1,2,nz+1))
  do i = 1, 3
    Tc(:,i) = T + 2.0_dp*(i-1); Tsc(i) = T_surface - 1.5_dp*(i-1)
  enddo
  call rad%ir_spectra_batch(Tsc, Tc, [nz+1, 1], err, ir_fup_a=su, ir_fdn_a=sd, fup_n=nu, fdn_n=nd, w_up=wu, w_dn=wd); call check()
  print '(a,2es24.16)', 'checksum ', sum(su), sum(sd)
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) su; write(u) sd; write(u) nu; write(u) nd; write(u) wu; write(u) wd
  close(u)
  call rad%ir_spectra_batch(Tsc, Tc, [nz+2, 1], err, ir_fup_a=su)
  print '(a)', 'expected error: '//err
  call rad%ir_spectra_batch(Tsc, Tc, [nz+1, 1], err, fup_n=wu(:,:,1))
  print '(a)', 'expected error: '//err
"""


def test_11_fortran_binding_matches_python(tmp_path):
    from clima_amd import build, synthetic as S
    from clima_amd.fortran_case import write_case
    from clima_amd.radtran import Radtran
    from test_gpu_ir_jacobian import FORTRAN_PROGRAM
    if not os.path.exists(build.FLANG):
        pytest.skip("amdflang is not available on this box")
    build.build()
    head, rest = FORTRAN_PROGRAM.split("  allocate(ju(nz+1,nz+1)")
    tail = rest[rest.index("  call rad%destroy()"):]
    decl = "Tc(:,:), Tsc(:), su(:,:,:), sd(:,:,:), nu(:,:), nd(:,:), wu(:,:,:), wd(:,:,:)"
    program = head.replace("ju(:,:), jd(:,:), jt(:,:)", decl) + FORTRAN_CALLS + tail
    tb = S.modern_earth_tables(nw=30)
    nz, nzen, albedo = 40, 4, 0.15
    col = S.modern_earth_column(nz)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "spectra.bin")
    write_case(case, tb, col, nzen, albedo)
    src, exe = tmp_path / "spectra.f90", str(tmp_path / "spectra")
    src.write_text(program)
    subprocess.check_call([build.FLANG, "-O2", "-J", str(tmp_path), os.path.join(build.FORTRAN_DIR, "clima_radtran_hip.f90"),
                           str(src), "-o", exe, "-L" + build.CSRC, "-lclima_radtran_hip", "-Wl,-rpath," + build.CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"], cwd=str(tmp_path))
    out = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "expected error: ir_spectra_batch: spec_level(1) = %d is outside 1..%d" % (nz + 2, nz + 1) in out.stdout
    assert 'expected error: ir_spectra_batch: "fup_n" has the wrong dimension' in out.stdout
    r = Radtran(tb, nz, nzen, albedo)
    r.radiate(*col.args())
    T = np.asfortranarray(np.stack([np.asarray(col["T"], dtype=float) + 2.0 * i for i in range(3)], axis=1))
    Ts = np.array([float(col["T_surface"]) - 1.5 * i for i in range(3)])
    want = r.ir_spectra_batch(Ts, T, levels=[-1, 0], parts=("up", "dn"), fluxes=True, weights=True)
    m = np.fromfile(res, dtype=np.float64)
    at = 0
    for name in ("fup", "fdn", "fup_n", "fdn_n", "w_up", "w_dn"):
        size = want[name].size
        assert m[at:at + size].tobytes() == want[name].tobytes(order="F"), name
        at += size
    assert at == m.size
    sums = [float(v) for v in out.stdout.split("checksum")[1].split()[:2]]
    assert np.allclose(sums, [want["fup"].sum(), want["fdn"].sum()], rtol=1e-12)
