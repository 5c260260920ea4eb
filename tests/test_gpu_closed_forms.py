"""The HIP path against tests/closed_forms.py: references of `compute_opacity`'s band mean, scattering depth and asymmetry,
of Planck, of the orchestration of `radiate` and of both two-stream solvers at w0 = 0 that share nothing with oracle/.
Every other GPU test of those parts compares with oracle/clima_oracle.c, written by the same hands from the same reading
of the reference as the kernels: a shared misreading passes all of them and fails here.

Every launch form a call can take is run: the group-of-lanes opacity kernel (`coop_items` at its default) and the
lane-per-item one (`coop_items = 0`), each with the fused grid on and off; the paired form (a doubled column), the
half-wave two-stream launch (16 g-points at 100 layers) and, for batches, the general kernel and the response form.

Bounds -- none of them taken from what the kernels give:
  * tau_band, scat, g against `band_mean` ..... RTOL_OPR = 1e-11 relative (g where its denominator exceeds tau_min),
    and the identities sum_g w_g tau = tau_band, w0 tau = scat for every g-point
  * fup_a / fdn_a / amean, EVERY BIN ON ITS OWN SCALE (the larger of the bin's fup_a and fdn_a maxima; the bin's own amean
    maximum) ..... max(2e-10, 10 x the oracle's distance from the closed form on that bin); 2e-10 is
    test_gpu_golden.TOL, the project's bound for one production solve against the reference's solver
  * fup_n, fdn_n, f_total, ISR, OLR ........... TOL_LEVEL / RTOL_TOA = 1e-9 against the closed form
  * surface albedo 0: solar fup_a exactly 0.0; fdn_a and amean element by element to 1e-12 relative wherever the
    element is at least 1e-30 of its bin's maximum (`exp_tab`'s (1.5 + |x|) 2^-52 with |x| <= 70 is 1.6e-14; the
    rounding of a cumulative optical depth of at most 130 layers, 130 x 2^-53 x 70 = 1e-12 if every rounding fell on
    one side); at most half of a case's elements lie below, asserted on the closed form
  * batches: test_gpu_fuzz.test_random_ir_batches_in_the_response_form's bounds with the closed form as the reference and
    the difference of the oracle's two compilations as the yardstick: max(1e-9, 10 x yardstick) for the response form,
    5 x that for the general kernel
  * scattering on (closed_forms.SCATTERING_CASES, each asserted on the exact reference alone to scatter): a whole call in
    the four forms against `radiate_exact`, the 50-digit solves of the two-stream system on the call's own tau, w0, g,
    with the bounds above -- per bin max(2e-10, 10 x the oracle's distance from exact on that bin), levels 1e-9; IR amean
    identically 0.  nz65-g16 takes the half-wave two-stream launch; above 64 layers with 8 g-points and coop_items = 0 the
    fused grid takes the call: its half-wave form (nz70), its whole-wave form (custom properties, nz66) and its paired
    form (a doubled column of 226 layers); the planner's hook is asked that they do.  custom-nz12 also against optical
    properties that take nothing from the code under test (`mixing_split`, `band_mean`)
  * the entry points on stored scattering opacities (radiate_solar_batch, radiate_ir_batch, ir_spectra_batch,
    ir_jacobian_spectral) against the same exact columns: per bin -- weights and Jacobian rows on the row's largest
    entry -- max(2e-10, 10 x the distance of the entry point's oracle-side counterpart from exact)

The closed forms take tau[nz][ng][nw] from the code under test here; tau itself is held by `band_mean` here and,
element by element, by `mixing_split` in test_gpu_mixing_split.py, which also runs the pure-absorption cases with no tau
supplied.

Measured on an MI355X (worst over all cases and launch forms; pytest -s prints each):
  * tau_band 1.7e-13, g 6.2e-15 (margin to 1e-11: 58x); sum_g w_g tau against tau_band 3.0e-16, w0 tau against scat
    8.8e-16, its spread over the g-points 2.2e-16
  * IR per bin 5.1e-12 (nz12-cold-T02, whose bin maxima span 115 decades; the oracle is 8.4e-12 from the closed form
    there): 0.025 of the bound at the most.  Solar per bin 8.0e-16, amean 1.0e-15 (margin to 2e-10: five orders)
  * level fluxes 2.8e-12, f_total 7.1e-12, OLR 2.4e-12, ISR 7.7e-16 (margin to 1e-9: 140x)
  * albedo 0: fup_a identically 0 in every form; element by element 1.0e-14 (margin to 1e-12: 98x), 15-26 % of a case's
    elements below 1e-30 of their bin's maximum
  * batches: response form 4.5e-13, general kernel 4.1e-13 of the channel's largest level flux (bound 1e-9 / 5e-9)

Measured on an MI355X, scattering on (worst over all cases and launch forms, and its share of the bound):
  * a whole call: IR per bin 7.4e-12 (rayleigh-sky-nz12, ir_tau_min = 1e-6; the oracle is 7.3e-12 from exact there):
    0.037 of the bound; solar per bin 2.2e-15, amean 2.2e-15: 1e-5 of the bound; IR amean identically 0; level fluxes
    4.9e-12, f_total 2.4e-11, OLR 5.0e-12, ISR 5.6e-16: 0.024 of 1e-9 at the most.  The fused grid's three forms and
    the stand-alone reference of custom-nz12 are no further off than the rest (IR 1.5e-15 stand-alone)
  * radiate_solar_batch: per bin 3.1e-16, amean 5.4e-16, level fluxes 1.7e-16
  * radiate_ir_batch: response form 1.6e-15, general kernel 1.4e-15 of the channel's largest level flux
  * ir_spectra_batch: spectra per bin 4.5e-12 (0.023 of the bound), level fluxes 8.0e-15; weights upward 1.1e-12 of the
    row's largest entry (0.006 of the bound), downward 6.3e-9 at the ground of dusty-nz33-no-surface, where the oracle's
    solver on unit Planck vectors is 2.6e-9 from exact (the source slope dB/tau in layers just above ir_tau_min): 0.24
    of that row's bound; custom-nz12 1e-15 throughout
  * ir_jacobian_spectral: rows upward 1.1e-12, downward 6.3e-9 (the same rows, the same share)
"""
import mpmath
import numpy as np
import pytest

import closed_forms as CF
import launch_forms as LF
from test_closed_forms_host import (STANDALONE_CASE, _rel, check_albedo_zero, check_levels, check_opr_identities,
                                    oracle_absorption, oracle_pair, oracle_scattering)
from test_gpu_parity import RTOL_OPR, RTOL_TOA, TOL_LEVEL

pytestmark = pytest.mark.gpu

TOL_BIN = 2e-10          # tests/test_gpu_golden.py TOL

# (coop_items, fused): None leaves the library's default
FORMS = {"coop-fused": (None, True), "coop-separate": (None, False), "lanes-fused": (0, True), "lanes-separate": (0, False)}


def _handle(tables, nz, nzen, form, scalars=None, albedo=None, emissivity=None, custom=None):
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, nzen, 0.3)
    coop, fused = FORMS[form]
    if coop is not None:
        r.coop_items = coop
    r.fused = fused
    for k, v in (scalars or {}).items():
        setattr(r, k, v)
    if albedo is not None:
        r.surface_albedo = albedo
    if emissivity is not None:
        r.surface_emissivity = emissivity
    if custom is not None:
        r.set_custom_optical_properties(*custom)
    return r


@pytest.fixture(scope="module")
def references():
    """Each case's closed forms, computed once and left unchanged: the launch forms of a case share them."""
    return {}


# ------------------------------------------------------------------------------------------------ band mean

@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CF.OPACITY_CASES))
def test_band_mean_scattering_depth_and_asymmetry(hip_lib, references, name, form):
    if ("opacity", name) not in references:
        tables, column, custom = CF.opacity_case(name)
        references["opacity", name] = (tables, column, custom, CF.band_mean(tables, column, custom))
    tables, column, custom, (tb, scat, gc) = references["opacity", name]
    nz = len(column["T"])
    r = _handle(tables, nz, 1, form, custom=custom)
    r.radiate(*column.args())
    tau, w0, g, tau_band = r.opr()
    e = (_rel(tau_band, tb), _rel(g, gc, np.asarray(scat > CF.TAU_MIN)))
    print("\n    %s %s: tau_band %.2e   g %.2e" % (name, form, e[0], e[1]))
    assert e[0] <= RTOL_OPR and e[1] <= RTOL_OPR
    ir0, sol0 = tables.nw - (len(tables.ir_wavl) - 1), 0
    assert np.array_equal(np.asarray(r.wrk_ir.tau_band)[::-1], tau_band[:, ir0:])
    assert np.array_equal(np.asarray(r.wrk_sol.tau_band)[::-1], tau_band[:, sol0:len(tables.sol_wavl) - 1])
    check_opr_identities(tables, (tau, w0, g, tau_band), scat, RTOL_OPR)


# ------------------------------------------------------------------------------------------------ pure absorption

def _absorption_reference(O, references, name):
    """The case, the oracle's per-bin distance from the closed forms (on the oracle's own tau), and a cache of the closed
    forms per distinct tau of the code under test (the fused and the separate launches give the same tau bit for bit)."""
    if ("absorption", name) not in references:
        case, o, closed, _ = oracle_absorption(O, name)
        dist = (CF.per_bin(o.wrk_ir.fup_a, o.wrk_ir.fdn_a, closed.ir.fup_a, closed.ir.fdn_a),
                CF.per_bin(o.wrk_sol.fup_a, o.wrk_sol.fdn_a, closed.sol.fup_a, closed.sol.fdn_a),
                CF.per_bin_one(o.wrk_sol.amean, closed.sol.amean))
        references["absorption", name] = (case, dist, {})
    return references["absorption", name]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CF.ABSORPTION_CASES))
def test_pure_absorption_against_the_exact_sweeps(O, hip_lib, references, name, form):
    case, dist, by_tau = _absorption_reference(O, references, name)
    r = _handle(case["tables"], case["nz"], case["nzen"], form, case["scalars"], case["albedo"], case["emissivity"])
    isr, olr = r.TOA_fluxes(*case["column"].args())
    tau, w0 = r.opr()[:2]
    assert np.all(w0 == 0.0)
    key = tau.tobytes()
    if key not in by_tau:
        by_tau[key] = CF.closed_for(case, tau)
    closed = by_tau[key]
    ir, sol = r.wrk_ir, r.wrk_sol
    errs = (CF.per_bin(ir.fup_a, ir.fdn_a, closed.ir.fup_a, closed.ir.fdn_a),
            CF.per_bin(sol.fup_a, sol.fdn_a, closed.sol.fup_a, closed.sol.fdn_a),
            CF.per_bin_one(sol.amean, closed.sol.amean))
    print("\n    %s %s" % (name, form))
    for what, e, d in zip(("IR", "solar", "amean"), errs, dist):
        bound = np.maximum(TOL_BIN, 10.0 * d)
        print("    %-5s per bin: worst %.2e (oracle from the closed form %.2e), largest share of the bound %.3f"
              % (what, e.max(), d.max(), (e / bound).max()))
        assert np.all(e <= bound), (what, e, bound)
    assert np.all(np.asarray(ir.amean) == 0.0)
    check_levels(ir, sol, r.f_total, isr, olr, closed, TOL_LEVEL, RTOL_TOA)
    if not np.any(case["albedo"]):
        check_albedo_zero(sol, closed.sol)


# ------------------------------------------------------------------------------------------------ scattering on

def _scattering_reference(O, references, name):
    """The case, the oracle's per-bin distance from the exact call (on the oracle's own tau, w0, g), and a cache of the
    exact call per distinct (tau, w0, g) of the code under test."""
    if ("scattering", name) not in references:
        case, _, _, _, dist = oracle_scattering(O, name)
        references["scattering", name] = (case, dist[0], {})
    return references["scattering", name]


def planned(L, case, form):
    """The plan of the library's own planner (clima_test_plan_radiate) for a single call of this case in this form."""
    tables, nz = case["tables"], case["nz"]
    coop, fused = FORMS[form]
    n_ir, n_sol = len(tables.ir_wavl) - 1, len(tables.sol_wavl) - 1
    pairs = nz % 2 == 0 and bool(np.all(CF.pair_reuse(case["column"], bool(tables.particles))[1::2]))
    assert pairs == case["doubled"]          # a doubled column is all pairs: one opacity item serves both layers of each
    return LF.hook_plan(L, nz=nz, ng=tables.ng, nzen=case["nzen"], n_ir=n_ir, n_sol=n_sol, op_n=tables.nw,
                        nsrc=nz // 2 if pairs else nz, ncol=1, batch=0, ir_batch=0,
                        rebin_mode=LF.hook_rebin_mode(L, tables.ktables[0]["weights"], False), cust_on=case["custom"] is not None,
                        compute_opacity=1, all_pairs=pairs, fused=fused, allow_fused=1, ts_block_mode=0, no_half=0,
                        coop_items=LF.DEFAULT_COOP_ITEMS if coop is None else coop, force_slots=0, nbins=max(n_ir, n_sol))


# what a case is there for: (form of the test, the planner's output, its value)
REACHES = {
    "nz65-g16": [(f, "ts_form", LF.HALF) for f in FORMS],                       # the half-wave two-stream launch
    "nz70-fused-half": [("lanes-fused", "fused_form", LF.HALF)],
    "custom-nz66-fused-wave": [("lanes-fused", "fused_form", LF.WAVE)],
    "doubled-2x113-fused-paired": [("lanes-fused", "fused_form", LF.PAIRED)],
}


def _check_bins(errs, dist, tag):
    """fup_a / fdn_a, amean: every bin on its own scale within max(TOL_BIN, 10 x the oracle's distance on that bin)"""
    for what, e, d in zip(("IR", "solar", "amean"), errs, dist):
        bound = np.maximum(TOL_BIN, 10.0 * d)
        print("    %-5s per bin: worst %.2e (oracle from the exact call %.2e), largest share of the bound %.3f"
              % (what, e.max(), d.max(), (e / bound).max()))
        assert np.all(e <= bound), (tag, what, e, bound)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CF.SCATTERING_CASES))
def test_scattering_against_the_exact_solves(O, hip_lib, references, name, form):
    """A whole call with scattering on against `CF.radiate_exact` on the call's own tau, w0, g: what hands w0 per g-point
    and g per (layer, bin) from the opacity stage to the two-stream stage, the delta scaling and the caps, per-bin albedo
    and emissivity, the sums over g-points, zenith angles and bins, amean."""
    case, dist, by_props = _scattering_reference(O, references, name)
    r = _handle(case["tables"], case["nz"], case["nzen"], form, case["scalars"], case["albedo"], case["emissivity"], case["custom"])
    isr, olr = r.TOA_fluxes(*case["column"].args())
    plan = planned(hip_lib, case, form)
    for f, field, want in REACHES.get(name, ()):
        if f == form:
            assert plan[field] == want, (field, plan)
    assert r.fused_fallbacks == 0
    tau, w0, g = r.opr()[:3]
    key = tau.tobytes() + w0.tobytes() + g.tobytes()
    if key not in by_props:
        by_props[key] = CF.closed_for(case, tau, w0, g)
    exact = by_props[key]
    ir, sol = r.wrk_ir, r.wrk_sol
    print("\n    %s %s" % (name, form))
    _check_bins(CF.scattering_errors(ir, sol, exact), dist, (name, form))
    assert np.all(np.asarray(ir.amean) == 0.0)
    check_levels(ir, sol, r.f_total, isr, olr, exact, TOL_LEVEL, RTOL_TOA)


def test_scattering_against_the_stand_alone_reference(O, hip_lib):
    """One case with nothing taken from the code under test: tau, w0 from `mixing_split` and g from `band_mean`, rounded to
    doubles; the yardstick is the oracle's distance from that same reference."""
    case, _, props, exact, dist = oracle_scattering(O, STANDALONE_CASE, standalone=True)
    for form in ("coop-fused", "lanes-separate"):
        r = _handle(case["tables"], case["nz"], case["nzen"], form, case["scalars"], case["albedo"], case["emissivity"], case["custom"])
        isr, olr = r.TOA_fluxes(*case["column"].args())
        print("\n    %s %s, stand-alone" % (STANDALONE_CASE, form))
        _check_bins(CF.scattering_errors(r.wrk_ir, r.wrk_sol, exact), dist[0], (STANDALONE_CASE, form))
        check_levels(r.wrk_ir, r.wrk_sol, r.f_total, isr, olr, exact, TOL_LEVEL, RTOL_TOA)


# ------------------------------------------------------------------------------------------------ batches

@pytest.mark.parametrize("name", ["nz12", "nz65-thin"])
def test_ir_batches_against_the_exact_sweep(O, hip_lib, name):
    """radiate_ir_batch on a pure-absorption handle: 9 columns, a few temperatures changed in each, through the general
    kernel (ir_green = 0) and the response form (ir_green = 2)."""
    case = CF.absorption_case(name)
    col, nz, ncol = case["column"], case["nz"], 9
    r = _handle(case["tables"], nz, case["nzen"], "coop-fused", case["scalars"], case["albedo"], case["emissivity"])
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
    Ts, T = _deviated_profiles(col, nz, ncol)
    trans = CF.ir_transmissions(case["tables"], tau)
    s = case["scalars"]
    exact_ir = lambda c: CF.ir_channel(case["tables"], tau, Ts[c], T[:, c], case["emissivity"], s["has_hard_surface"],   # noqa: E731
                                       s["ir_tau_min"], trans)
    _hold_ir_batches(r, oracles, col, Ts, T, exact_ir, name)


def _deviated_profiles(col, nz, ncol):
    """-> T_surface (ncol), T (nz, ncol): the column's profile with one to three temperatures changed by 1e-3 ... 40 K in
    every column but the first"""
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
    return Ts, T


def _hold_ir_batches(r, oracles, col, Ts, T, exact_ir, name):
    """radiate_ir_batch through the general kernel and the response form: the level fluxes of every column against
    `exact_ir(c)`, within max(TOL_LEVEL, 10 x the difference of the oracle's two compilations) of the channel's largest level
    flux for the response form and 5 x that for the general kernel"""
    from clima_amd import synthetic as S
    ncol = len(Ts)
    r.ir_green = 0
    gen = r.radiate_ir_batch(Ts, T)
    assert r.ir_green_batches == 0
    r.ir_green = 2
    got = r.radiate_ir_batch(Ts, T)
    assert r.ir_green_batches == 1
    worst = [0.0, 0.0]
    for c in range(ncol):
        ref = exact_ir(c)
        w = S.Column(col)
        w["T"], w["T_surface"] = T[:, c].copy(), Ts[c]
        rows = []
        for o in oracles:
            o.radiate(*w.args(), compute_solar=False, compute_opacity=False)
            rows.append((np.array(o.wrk_ir.fup_n), np.array(o.wrk_ir.fdn_n)))
        scale = max(float(np.max(np.abs(ref.fup_n))), float(np.max(np.abs(ref.fdn_n))))
        for i, want in enumerate((ref.fup_n, ref.fdn_n)):
            yard = float(np.max(np.abs(rows[0][i] - rows[1][i]))) / scale
            tol = max(TOL_LEVEL, 10.0 * yard)
            e_got = float(np.max(np.abs(np.asarray(got[i][:, c], dtype=CF.LD) - want))) / scale
            e_gen = float(np.max(np.abs(np.asarray(gen[i][:, c], dtype=CF.LD) - want))) / scale
            worst = [max(worst[0], e_got), max(worst[1], e_gen)]
            assert e_got <= tol, (c, i, "response form", e_got, tol)
            assert e_gen <= 5.0 * tol, (c, i, "general kernel", e_gen, tol)
    print("\n    %s: response form %.2e, general kernel %.2e of the channel's largest level flux" % (name, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------ stored scattering opacities
# The entry points that reuse a call's stored tau, w0, g, on a handle in the coop-fused form: each against `radiate_exact`'s
# machinery on the handle's own optical properties, with the bound of the whole call.  The yardstick of each is its
# oracle-side counterpart on the same properties.

STORED_CASES = ["dusty-nz33-no-surface", "custom-nz12"]
LEVELS = (-1, 0)                 # the top of the atmosphere and the ground


class _Stored:
    """a case's handle after one call, its optical properties, the exact IR columns and what the tests derive from them"""

    def units(self):
        """exact unit responses at LEVELS, summed over the g-points: up, dn (nw_ir, len(LEVELS), nz+1 j) as the library
        orders them (levels as LEVELS names them, x(0) = T_surface, x(1 + m) = T[m]), mpmath numbers"""
        if self._units is None:
            ir, nz = self.ir, self.case["nz"]
            up = [[[None] * (nz + 1) for _ in LEVELS] for _ in range(ir.nwc)]
            dn = [[[None] * (nz + 1) for _ in LEVELS] for _ in range(ir.nwc)]
            with mpmath.workdps(ir.dps):
                for l in range(ir.nwc):
                    for k in range(nz + 1):                              # k TOA-first, the surface last: x(nz - k)
                        fu, fd = ir.unit_mp(l, k)
                        for a, lev in enumerate(LEVELS):
                            i = nz - (lev % (nz + 1))                    # the level, TOA-first
                            up[l][a][nz - k], dn[l][a][nz - k] = fu[i], fd[i]
            self._units = (up, dn)
        return self._units


@pytest.fixture(scope="module")
def stored(O, hip_lib):
    kept = {}

    def get(name):
        if name not in kept:
            s = _Stored()
            s.case = case = CF.scattering_case(name)
            s.r = _handle(case["tables"], case["nz"], case["nzen"], "coop-fused", case["scalars"], case["albedo"],
                          case["emissivity"], case["custom"])
            s.r.radiate(*case["column"].args())
            s.opr = tuple(np.array(a) for a in s.r.opr())
            sc = case["scalars"]
            s.ir = CF.ExactIr(case["tables"], *s.opr[:3], case["emissivity"], sc["has_hard_surface"], sc["ir_tau_min"])
            s.oracles = oracle_pair(O, case)
            s._units = None
            kept[name] = s
        return kept[name]
    return get


def _rows_worst(got, ref_mp, oracle, what):
    """(nw_ir, nsel, nz+1) arrays row by row, every row on its largest entry in the exact one: within
    max(TOL_BIN, 10 x the oracle-side counterpart's distance on that row)"""
    ref = np.array([[[CF._ld(v) for v in row] for row in rows] for rows in ref_mp], dtype=CF.LD)
    scale = np.max(np.abs(ref), axis=2)
    assert np.mean(scale > 0) >= 0.5                # (nothing comes down at the top of the atmosphere: rows of zeros)

    def dist(a):
        err = np.max(np.abs(np.asarray(a, dtype=CF.LD) - ref), axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0)).astype(float)
    e, d = dist(got), dist(oracle)
    bound = np.maximum(TOL_BIN, 10.0 * d)
    print("    %-28s rows: worst %.2e (oracle side %.2e), largest share of the bound %.3f" % (what, e.max(), d.max(), (e / bound).max()))
    assert np.all(e <= bound), (what, e, bound)


@pytest.mark.parametrize("name", STORED_CASES)
def test_solar_batch_against_the_exact_solves(O, stored, name):
    """radiate_solar_batch: 5 illumination cases of 1 to 4 zenith angles (a batch of 4, the others at weight 0) with their
    own per-bin albedo and photon scale factor, against the `SolarColumn` sums."""
    s = stored(name)
    case, r, nz = s.case, s.r, s.case["nz"]
    tables, sc = case["tables"], case["scalars"]
    nsol = len(tables.sol_wavl) - 1
    rng = np.random.default_rng(5)
    ncase, nzen = 5, 4
    zu = rng.uniform(0.05, 1.0, (ncase, nzen))
    zw = rng.uniform(0.1, 0.6, (ncase, nzen))
    for c, n in enumerate((1, 2, 3, 4, 2)):
        zw[c, n:] = 0.0
    alb = rng.uniform(0.0, 0.9, (ncase, nsol))
    scale = np.array([1.0, 0.4286, 2.5, 0.8, 1.7])
    fup, fdn, ft, spec = r.radiate_solar_batch(zu, zw, alb, scale, spectra_levels=list(range(nz + 1)))
    if not hasattr(s, "sol"):
        s.sol = CF.ExactSolar(tables, *s.opr[:3])
    o = s.oracles[0]
    a = case["column"].args()
    print("\n    %s" % name)
    for c in range(ncase):
        on = zw[c] > 0
        exact = s.sol.channel(zu[c][on], zw[c][on], alb[c], sc["diurnal_fac"], scale[c])
        o.set_zenith(zu[c], zw[c])
        o.set_surface_albedo(alb[c])
        o.set_scalars(photon_scale_factor=scale[c])
        o.radiate(*a, compute_opacity=False)
        osol = o.wrk_sol
        dist = (CF.per_bin(osol.fup_a, osol.fdn_a, exact.fup_a, exact.fdn_a), CF.per_bin_one(osol.amean, exact.amean))
        errs = (CF.per_bin(spec["fup"][:, :, c], spec["fdn"][:, :, c], exact.fup_a, exact.fdn_a),
                CF.per_bin_one(spec["amean"][:, :, c], exact.amean))
        for what, e, d in zip(("solar", "amean"), errs, dist):
            bound = np.maximum(TOL_BIN, 10.0 * d)
            print("    case %d %-5s per bin: worst %.2e (oracle %.2e), largest share of the bound %.3f" % (c, what, e.max(), d.max(), (e / bound).max()))
            assert np.all(e <= bound), (c, what, e, bound)
        lv = max(float(np.max(np.abs(exact.fup_n))), float(np.max(np.abs(exact.fdn_n))))
        e_n = max(float(np.max(np.abs(fup[:, c] - exact.fup_n))), float(np.max(np.abs(fdn[:, c] - exact.fdn_n)))) / lv
        print("    case %d levels %.2e" % (c, e_n))
        assert e_n <= TOL_LEVEL
    o.set_zenith(*CF.zenith(case["nzen"]))                   # the oracle as the other tests expect it
    o.set_surface_albedo(case["albedo"])
    o.set_scalars(photon_scale_factor=sc["photon_scale_factor"])


@pytest.mark.parametrize("name", STORED_CASES)
def test_ir_batches_against_the_exact_solves(stored, name):
    """radiate_ir_batch on scattering opacities: 6 columns, a few temperatures changed in each, through the general kernel
    and the response form, with test_ir_batches_against_the_exact_sweep's bounds."""
    s = stored(name)
    col, nz = s.case["column"], s.case["nz"]
    Ts, T = _deviated_profiles(col, nz, 6)
    _hold_ir_batches(s.r, s.oracles, col, Ts, T, lambda c: s.ir.channel(Ts[c], T[:, c]), name)


@pytest.mark.parametrize("name", STORED_CASES)
def test_ir_spectra_batch_against_the_exact_solves(O, stored, name):
    """ir_spectra_batch at the top and the ground, both directions, with level fluxes and weights, for 5 random profiles of
    150-350 K: the spectra against the exact IR call, the weights against the exact unit responses."""
    import ir_spectra_batch_oracle as SB
    s = stored(name)
    case, r, nz = s.case, s.r, s.case["nz"]
    tables, sc = case["tables"], case["scalars"]
    rng = np.random.default_rng(7)
    ncol = 5
    T, Ts = rng.uniform(150.0, 350.0, (nz, ncol)), rng.uniform(150.0, 350.0, ncol)
    got = r.ir_spectra_batch(Ts, T, levels=LEVELS, parts=("up", "dn"), fluxes=True, weights=True)
    w = SB.weights(O, tables, s.opr, case["emissivity"], sc["has_hard_surface"], sc["ir_tau_min"])
    sel = [lev % (nz + 1) for lev in LEVELS]
    print("\n    %s" % name)
    for c in range(ncol):
        exact = s.ir.channel(Ts[c], T[:, c])
        o_up, o_dn = SB.from_weights(O, tables, w, Ts[c], T[:, c])              # (nw_ir, nz+1), levels ground-first
        scale = np.maximum(np.max(np.abs(exact.fup_a), axis=0), np.max(np.abs(exact.fdn_a), axis=0))
        dist = np.maximum(np.max(np.abs(o_up.T - exact.fup_a), axis=0), np.max(np.abs(o_dn.T - exact.fdn_a), axis=0)) / scale
        e = np.maximum(np.max(np.abs(got["fup"][:, :, c].T - exact.fup_a[sel]), axis=0),
                       np.max(np.abs(got["fdn"][:, :, c].T - exact.fdn_a[sel]), axis=0)) / scale
        e, dist = np.asarray(e, dtype=float), np.asarray(dist, dtype=float)
        bound = np.maximum(TOL_BIN, 10.0 * dist)
        lv = max(float(np.max(np.abs(exact.fup_n))), float(np.max(np.abs(exact.fdn_n))))
        e_n = max(float(np.max(np.abs(got["fup_n"][:, c] - exact.fup_n[sel]))), float(np.max(np.abs(got["fdn_n"][:, c] - exact.fdn_n[sel])))) / lv
        print("    column %d spectra per bin: worst %.2e (oracle side %.2e), largest share of the bound %.3f; levels %.2e"
              % (c, e.max(), dist.max(), (e / bound).max(), e_n))
        assert np.all(e <= bound), (c, e, bound)
        assert e_n <= TOL_LEVEL
    up, dn = s.units()
    _rows_worst(got["w_up"], up, w[0][:, sel, :], "weights up")
    _rows_worst(got["w_dn"], dn, w[1][:, sel, :], "weights down")


@pytest.mark.parametrize("name", STORED_CASES)
def test_ir_jacobian_spectral_against_the_exact_solves(O, stored, name):
    """ir_jacobian_spectral at the top and the ground, both directions: the exact unit responses times the 40-digit dB/dT."""
    import ir_jacobian_spectral_oracle as JS
    from ir_spectra_vjp_oracle import dplanck_dT
    s = stored(name)
    case, r, nz = s.case, s.r, s.case["nz"]
    sc, col = case["scalars"], case["column"]
    got = r.ir_jacobian_spectral(col["T_surface"], col["T"], levels=LEVELS, parts=("up", "dn"))
    o_up, o_dn, _ = JS.spectral_jacobian(O, case["tables"], s.opr, col["T_surface"], col["T"], case["emissivity"],
                                         sc["has_hard_surface"], sc["ir_tau_min"])
    sel = [lev % (nz + 1) for lev in LEVELS]
    x = [float(col["T_surface"])] + [float(t) for t in col["T"]]
    up, dn = s.units()
    with mpmath.workdps(s.ir.dps):
        ref = [[[[v * dplanck_dT(s.ir.nu(l), x[j]) for j, v in enumerate(row)] for row in part[l]] for l in range(s.ir.nwc)]
               for part in (up, dn)]
    print("\n    %s" % name)
    _rows_worst(got["up"], ref[0], o_up[:, sel, :], "jacobian up")
    _rows_worst(got["dn"], ref[1], o_dn[:, sel, :], "jacobian down")
