"""The CPU oracle (oracle/clima_oracle.c) against tests/closed_forms.py: references that share no code and no reading of
the reference with it.  Runs without a GPU.  What these tests establish is that the reference implementation ALONE
stays inside every bound that tests/test_gpu_closed_forms.py asks of the HIP path -- so a miss there is the HIP path's.

Bounds (none of them comes from what the code under test gives):
  * tau_band, scat, g against `band_mean` ............ 1e-12 relative (the project's RTOL_OPR is 1e-11)
  * per-bin spectra against the exact sweeps, each bin on its own scale ... max(2e-12, 10 x the difference between
    the oracle's two compilations, liborc.so and liborc_fma.so, on that bin): the IR source slope dB/tau in layers just
    above ir_tau_min is what both lose digits to
  * level fluxes, f_total, ISR, OLR .................. TOL_LEVEL / RTOL_TOA = 1e-9, as on the GPU
  * albedo 0: solar fup_a exactly 0; fdn_a and amean element by element to 1e-12 relative down to 1e-30 of the bin's
    maximum ((1.5 + |x|) 2^-52 with |x| <= 70 for one exponential is 1.6e-14; the cumulative optical depth of at most
    130 layers adds 130 x 2^-53 x 70 = 1e-12 at the very worst, every rounding on one side)

  * scattering on (closed_forms.SCATTERING_CASES): a whole call against `radiate_exact`, the 50-digit solves of the
    two-stream system, on the oracle's own tau, w0, g -- per bin TOL_BIN_SOLVE = 2e-10 (test_gpu_golden.TOL, the project's
    bound for one production solve against the reference's solver), both compilations; level fluxes, f_total, ISR, OLR
    1e-9.  Every case first meets `check_scattering_case` on the exact reference alone: at least 40 % of its channel's
    elements have w0 > 0.1, the cap cases reach the cap, and the exact answer at w0 = 0 (at g = 0) is 1e3 bounds away in
    half the bins or more.  custom-nz12 also with tau, w0 from `mixing_split` and g from `band_mean`: nothing of the oracle

Measured here, scattering on (worst over the nine cases and both compilations):
  * IR per bin 1.2e-11 (rayleigh-sky-nz12, ir_tau_min = 1e-6; the two compilations are 1.2e-11 apart there): 0.057 of the
    bound; solar per bin 1.7e-15, amean 1.2e-15; level fluxes 7.1e-12, f_total 4.6e-11, OLR 7.9e-12, ISR 8.0e-16
  * stand-alone custom-nz12: IR 1.6e-15, solar 4.1e-16, amean 5.3e-16
  * the exact answer at w0 = 0 is up to 0.88 of a bin's maximum away, at g = 0 up to 0.33; two bins' albedos swapped 0.60
  * the exact call takes 0.2-2.4 s per case

Measured here (worst over the cases of closed_forms.OPACITY_CASES / ABSORPTION_CASES; pytest -s prints each):
  * tau_band 4.8e-14, g 6.2e-15 (margin to 1e-12: 20x and more)
  * sum_g w_g tau against tau_band 3.6e-16; w0 tau against scat 9.7e-16, spread over the g-points 2.2e-16
  * IR per bin, ir_tau_min = 1e-6: 8.4e-12 where the two compilations differ by 1.1e-11 (bound there 1.1e-10); largest
    share of a bin's bound 0.15.  ir_tau_min = 1e-2: 2.1e-15
  * solar per bin 8.2e-16, amean 1.0e-15 (margin to 2e-12: 2000x)
  * level fluxes 2.5e-12 of the channel's maximum, f_total 3.1e-12, OLR 2.2e-12, ISR 7.1e-16 (margin to 1e-9: 300x)
  * albedo 0, element by element: 1.9e-14 (margin to 1e-12: 50x); elements below 1e-30 of their bin's maximum:
    15-26 % of a case's
  * the IR bin maxima of nz12-cold-T02 span 115 decades
"""
import numpy as np
import pytest

import closed_forms as CF

RTOL_MEAN = 1e-12
TOL_BIN = 2e-12
TOL_LEVEL = RTOL_TOA = 1e-9          # tests/test_gpu_parity.py
RTOL_ELEMENT = 1e-12
TOL_BIN_SOLVE = 2e-10                # tests/test_gpu_golden.py TOL: one production solve against the reference's solver
STANDALONE_CASE = "custom-nz12"


def _rel(a, b, where=None):
    a, b = np.asarray(a, dtype=CF.LD), np.asarray(b, dtype=CF.LD)
    d = np.abs(a - b) / np.maximum(np.abs(b), CF.LD(1e-300))
    return float(np.max(d if where is None else d[where], initial=0.0))


def _oracle(O, tables, nz, nzen, column, custom=None, variant="", albedo=0.3, emissivity=None, scalars=None):
    o = O.OracleRadtran(tables, nz, nzen, 0.3, variant=variant)
    if scalars:
        o.set_scalars(**scalars)
    if custom is not None:
        o.set_custom_optical_properties(*custom)
    o.set_surface_albedo(albedo)
    if emissivity is not None:
        o.set_surface_emissivity(emissivity)
    o.isr, o.olr = o.TOA_fluxes(*column.args())
    return o


def check_opr_identities(tables, opr, scat, rtol):
    """Wherever tau > tau_min and w0 < max_w0: sum_g w_g tau[:, g, l] is tau_band, and w0 tau is the same for every
    g-point and is the scattering depth (clima_radtran_types.f90:869-881).  -> the three measured maxima."""
    tau, w0, _, tau_band = opr
    w = np.asarray(tables.ktables[0]["weights"], dtype=CF.LD)
    mean = np.sum(np.asarray(tau, dtype=CF.LD) * w[None, :, None], axis=1)
    a = _rel(mean, tau_band)
    ok = (tau > CF.TAU_MIN) & (w0 < CF.MAX_W0)
    st = np.asarray(w0, dtype=CF.LD) * np.asarray(tau, dtype=CF.LD)
    want = np.broadcast_to(np.asarray(scat, dtype=CF.LD)[:, None, :], st.shape)
    b = _rel(st, want, ok)
    lo = np.min(np.where(ok, st, np.inf), axis=1)
    hi = np.max(np.where(ok, st, -np.inf), axis=1)
    some = np.any(ok, axis=1)
    c = float(np.max(((hi - lo) / np.maximum(hi, CF.LD(1e-300)))[some], initial=0.0))
    print("    sum_g w_g tau vs tau_band %.2e   w0 tau vs scat %.2e   spread over g %.2e   (%d of %d elements)"
          % (a, b, c, int(ok.sum()), ok.size))
    assert a <= rtol and b <= rtol and c <= rtol
    return a, b, c


@pytest.mark.parametrize("name", list(CF.OPACITY_CASES))
def test_oracle_band_mean_scattering_depth_and_asymmetry(O, name):
    tables, column, custom = CF.opacity_case(name)
    o = _oracle(O, tables, len(column["T"]), 1, column, custom)
    tau, w0, g, tau_band = o.opr()
    tb, scat, gc = CF.band_mean(tables, column, custom)
    assert np.any(scat > 0) and (not tables.particles or np.any(gc > 0))
    has_g = np.asarray(scat > CF.TAU_MIN)
    e = (_rel(tau_band, tb), _rel(g, gc, has_g))
    print("\n    %s: tau_band %.2e   g %.2e" % (name, e[0], e[1]))
    assert e[0] <= RTOL_MEAN and e[1] <= RTOL_MEAN
    assert np.array_equal(np.asarray(o.wrk_ir.tau_band)[::-1], tau_band[:, o.ir_start:o.ir_start + o.nw_ir])
    check_opr_identities(tables, (tau, w0, g, tau_band), scat, RTOL_MEAN)


def oracle_absorption(O, name):
    """One pure-absorption case through both compilations of the oracle and the closed forms on the oracle's own tau.
    -> case, oracle, closed forms, per-bin yardstick (ir, solar, amean)."""
    case = CF.absorption_case(name)
    o, o2 = (_oracle(O, case["tables"], case["nz"], case["nzen"], case["column"], None, v, case["albedo"], case["emissivity"],
                     case["scalars"]) for v in ("", "fma"))
    tau, w0 = o.opr()[:2]
    assert np.all(w0 == 0.0)
    closed = CF.closed_for(case, tau)
    yard = (CF.per_bin(o2.wrk_ir.fup_a, o2.wrk_ir.fdn_a, o.wrk_ir.fup_a, o.wrk_ir.fdn_a),
            CF.per_bin(o2.wrk_sol.fup_a, o2.wrk_sol.fdn_a, o.wrk_sol.fup_a, o.wrk_sol.fdn_a),
            CF.per_bin_one(o2.wrk_sol.amean, o.wrk_sol.amean))
    return case, o, closed, yard


def check_levels(got_ir, got_sol, f_total, isr, olr, closed, tol=TOL_LEVEL, rtol=RTOL_TOA):
    """fup_n / fdn_n on their channel's common scale, f_total on its own, ISR and OLR relative."""
    worst = 0.0
    for got, ref in ((got_ir, closed.ir), (got_sol, closed.sol)):
        scale = max(float(np.max(np.abs(ref.fup_n))), float(np.max(np.abs(ref.fdn_n))), 1e-300)
        for a, b in ((got.fup_n, ref.fup_n), (got.fdn_n, ref.fdn_n)):
            worst = max(worst, float(np.max(np.abs(np.asarray(a, dtype=CF.LD) - b))) / scale)
    ft = float(np.max(np.abs(np.asarray(f_total, dtype=CF.LD) - closed.f_total)) / np.max(np.abs(closed.f_total)))
    e_isr = float(abs(isr - closed.isr) / max(abs(closed.isr), CF.LD(1e-300)))
    e_olr = float(abs(olr - closed.olr) / abs(closed.olr))
    print("    levels %.2e   f_total %.2e   ISR %.2e   OLR %.2e" % (worst, ft, e_isr, e_olr))
    assert worst <= tol and ft <= tol
    assert e_isr <= rtol and e_olr <= rtol


def check_albedo_zero(sol, closed_sol, rtol=RTOL_ELEMENT):
    """Surface albedo 0: nothing comes up, and what goes down is the direct beam alone -- element by element.
    `rtol`: RTOL_ELEMENT where the closed form stands on the same tau as `sol`; a caller whose tau has another source
    adds what the difference is worth."""
    assert np.all(np.asarray(closed_sol.fup_a) == 0.0)
    assert np.all(np.asarray(sol.fup_a) == 0.0) and np.all(np.asarray(sol.fup_n) == 0.0)
    frac = CF.tiny_fraction(closed_sol)
    assert frac <= 0.5, frac                  # a property of the case, asserted on the closed form alone
    worst = 0.0
    for got, ref in ((sol.fdn_a, closed_sol.fdn_a), (sol.amean, closed_sol.amean)):
        held = np.asarray(ref >= CF.LD(1e-30) * np.max(ref, axis=0)[None, :])
        worst = max(worst, _rel(got, ref, held))
    print("    albedo 0: element by element %.2e, %.0f %% of the elements below 1e-30 of their bin" % (worst, 100 * frac))
    assert worst <= rtol


@pytest.mark.parametrize("name", list(CF.ABSORPTION_CASES))
def test_oracle_pure_absorption_against_the_exact_sweeps(O, name):
    case, o, closed, yard = oracle_absorption(O, name)
    ir, sol = o.wrk_ir, o.wrk_sol
    errs = (CF.per_bin(ir.fup_a, ir.fdn_a, closed.ir.fup_a, closed.ir.fdn_a),
            CF.per_bin(sol.fup_a, sol.fdn_a, closed.sol.fup_a, closed.sol.fdn_a),
            CF.per_bin_one(sol.amean, closed.sol.amean))
    print("\n    %s" % name)
    for what, e, y in zip(("IR", "solar", "amean"), errs, yard):
        bound = np.maximum(TOL_BIN, 10.0 * y)
        print("    %-5s per bin: worst %.2e (two compilations %.2e), largest share of the bound %.2f" % (what, e.max(), y.max(), (e / bound).max()))
        assert np.all(e <= bound), (what, e, bound)
    print("    IR bin maxima span %.0f decades" % np.log10(float(np.max(closed.ir.fup_a) / np.min(np.max(closed.ir.fup_a, axis=0)))))
    assert np.all(np.asarray(ir.amean) == 0.0)
    check_levels(ir, sol, o.f_total, o.isr, o.olr, closed)
    if not np.any(case["albedo"]):
        check_albedo_zero(sol, closed.sol)


def oracle_pair(O, case):
    """a scattering case through both compilations of the oracle"""
    return tuple(_oracle(O, case["tables"], case["nz"], case["nzen"], case["column"], case["custom"], v, case["albedo"],
                         case["emissivity"], case["scalars"]) for v in ("", "fma"))


def oracle_scattering(O, name, standalone=False):
    """One scattering case through both compilations of the oracle, and the 50-digit solves (`CF.radiate_exact`) on the
    oracle's own tau, w0, g -- `standalone`: on `CF.standalone_properties`, which take nothing from the oracle either.
    -> case, the two oracles, the properties, the exact call, each oracle's per-bin distances from it (IR, solar, amean)."""
    case = CF.scattering_case(name)
    oracles = oracle_pair(O, case)
    props = CF.standalone_properties(case) if standalone else tuple(np.asarray(a) for a in oracles[0].opr()[:3])
    exact = CF.closed_for(case, *props)
    dist = [CF.scattering_errors(o.wrk_ir, o.wrk_sol, exact) for o in oracles]
    return case, oracles, props, exact, dist


@pytest.mark.parametrize("name", list(CF.SCATTERING_CASES))
def test_oracle_scattering_against_the_exact_solves(O, name):
    """A whole call with scattering on -- the hand-over of w0 and g from the opacities to the solvers, the delta scaling and
    the caps, per-bin albedo and emissivity, the sums over g-points, zenith angles and bins, amean -- against
    `CF.radiate_exact`, which shares nothing with oracle/.  -> the first compilation's per-bin distance from exact, the
    yardstick of tests/test_gpu_closed_forms.py."""
    import time
    t0 = time.perf_counter()
    case, oracles, (tau, w0, g), exact, dist = oracle_scattering(O, name)
    seconds = time.perf_counter() - t0
    print("\n    %s (oracle twice and the exact call: %.1f s)" % (name, seconds))
    measured = CF.check_scattering_case(case, tau, w0, g, exact, TOL_BIN_SOLVE)
    for ch, m in measured.items():
        print("    %-3s w0 > %.1f in %.0f %% of the elements, at the cap %.1f %%, max w0 %.5f, max |g| %.3f; %s" % (
            ch, CF.W0_LEVEL, 100 * m["share"], 100 * m["at_cap"], m["w0_max"], m["g_max"],
            ", ".join("%s: %.0f %% of the bins 1e3 bounds away, worst %.2e" % (k, 100 * m[k][0], m[k][1]) for k in ("w0=0", "g=0") if k in m)))
    for variant, o, errs in zip(("plain", "fma"), oracles, dist):
        for what, e in zip(("IR", "solar", "amean"), errs):
            print("    %-5s %-5s per bin: worst %.2e, share of the bound %.3f" % (variant, what, e.max(), e.max() / TOL_BIN_SOLVE))
            assert np.all(e <= TOL_BIN_SOLVE), (variant, what, e)
        assert np.all(np.asarray(o.wrk_ir.amean) == 0.0)
        check_levels(o.wrk_ir, o.wrk_sol, o.f_total, o.isr, o.olr, exact)
    two = CF.scattering_errors(oracles[1].wrk_ir, oracles[1].wrk_sol, _as_closed(oracles[0]))
    print("    the two compilations apart: IR %.2e  solar %.2e  amean %.2e" % tuple(e.max() for e in two))


def _as_closed(o):
    c = CF.Closed()
    c.ir, c.sol = o.wrk_ir, o.wrk_sol
    return c


def test_oracle_scattering_against_the_stand_alone_reference(O):
    """custom-nz12 with nothing taken from the code under test: tau, w0 from `mixing_split`, g from `band_mean`."""
    case, oracles, props, exact, dist = oracle_scattering(O, STANDALONE_CASE, standalone=True)
    print()
    for variant, o, errs in zip(("plain", "fma"), oracles, dist):
        for what, e in zip(("IR", "solar", "amean"), errs):
            print("    %-5s %-5s per bin: worst %.2e, share of the bound %.3f" % (variant, what, e.max(), e.max() / TOL_BIN_SOLVE))
            assert np.all(e <= TOL_BIN_SOLVE), (variant, what, e)
        check_levels(o.wrk_ir, o.wrk_sol, o.f_total, o.isr, o.olr, exact)


def test_a_wrong_exact_call_is_told_apart():
    """`radiate_exact` with two bins' albedos (emissivities) swapped is another answer by orders of magnitude."""
    case = CF.scattering_case("rayleigh-sky-nz12")
    props = CF.standalone_properties(case)
    exact = CF.closed_for(case, *props)
    wrong = dict(case, albedo=case["albedo"][::-1].copy(), emissivity=case["emissivity"][::-1].copy())
    other = CF.closed_for(wrong, *props)
    e_ir, e_sol, e_am = CF.scattering_errors(other.ir, other.sol, exact)
    mid = len(e_sol) // 2 if len(e_sol) % 2 else None            # the middle bin of an odd count keeps its albedo
    print("\n    albedos and emissivities reversed: IR %s  solar %s" % (e_ir, e_sol))
    assert all(e >= CF.WRONG_FACTOR * TOL_BIN_SOLVE for i, e in enumerate(e_sol) if i != mid)
    assert np.mean(e_ir >= CF.WRONG_FACTOR * TOL_BIN_SOLVE) >= 0.5


def test_the_cold_column_reaches_bins_far_below_the_peak():
    """nz12-cold-T02 is there for the short-wave IR bins that an array-scaled comparison never sees."""
    case = CF.absorption_case("nz12-cold-T02")
    start, nwc = CF._channel_bins(case["tables"], case["tables"].ir_wavl)
    nu = [299792458.0 / (0.5e-9 * (case["tables"].ir_wavl[i] + case["tables"].ir_wavl[i + 1])) for i in range(nwc)]
    B = [float(CF.planck(x, case["column"]["T_surface"])) for x in nu]
    assert max(B) / min(B) > 1e24        # dozens of decades


def test_closed_forms_own_limits():
    """The sweeps against what they must give in cases that need no arithmetic: an isothermal column with a black
    surface radiates pi B at every level upward; without an atmosphere the beam arrives unattenuated."""
    import mpmath
    tau = np.array([0.3, 1e-8, 2.0, 40.0, 0.7])
    fup, fdn = CF.ir_sweep(tau, [mpmath.mpf(3)] * 6, 1.0, True, 1e-6)
    with mpmath.workdps(CF.DPS):
        assert all(abs(x - 3 * mpmath.pi) < mpmath.mpf("1e-35") for x in fup)
        total = sum(mpmath.mpf(float(x)) for x in tau)
        assert fdn[0] == 0 and abs(fdn[5] - 3 * mpmath.pi * (1 - mpmath.exp(-2 * total))) < mpmath.mpf("1e-35")
    fup, fdn, amean = CF.solar_sweep(np.zeros((4, 2)), 0.5, 0.25)
    assert np.all(fdn == 0.5) and np.all(fup == 0.125) and np.allclose(np.asarray(amean, dtype=float), np.sqrt(3) * 0.125 + 1.0, rtol=1e-15)
    i, q = CF._bracket([1.0, 2.0, 4.0, 8.0], [0.0, 1.0, 2.0, 3.0, 8.0, 12.0])
    assert list(i) == [0, 0, 1, 1, 2, 2] and [float(x) for x in q] == [-1.0, 0.0, 0.0, 0.5, 1.0, 2.0]
