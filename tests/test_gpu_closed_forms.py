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
"""
import numpy as np
import pytest

import closed_forms as CF
from test_closed_forms_host import _rel, check_albedo_zero, check_levels, check_opr_identities, oracle_absorption
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


# ------------------------------------------------------------------------------------------------ batches

@pytest.mark.parametrize("name", ["nz12", "nz65-thin"])
def test_ir_batches_against_the_exact_sweep(O, hip_lib, name):
    """radiate_ir_batch on a pure-absorption handle: 9 columns, a few temperatures changed in each, through the general
    kernel (ir_green = 0) and the response form (ir_green = 2)."""
    from clima_amd import synthetic as S
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
    r.ir_green = 0
    gen = r.radiate_ir_batch(Ts, T)
    assert r.ir_green_batches == 0
    r.ir_green = 2
    got = r.radiate_ir_batch(Ts, T)
    assert r.ir_green_batches == 1
    trans = CF.ir_transmissions(case["tables"], tau)
    s = case["scalars"]
    worst = [0.0, 0.0]
    for c in range(ncol):
        ref = CF.ir_channel(case["tables"], tau, Ts[c], T[:, c], case["emissivity"], s["has_hard_surface"], s["ir_tau_min"], trans)
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
