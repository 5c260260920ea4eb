"""The CPU oracle (oracle/clima_oracle.c), in both compilations, against `closed_forms.mixing_split`: how the random-overlap
mixing step (k_rorr, clima_radtran_types.f90:823-852) splits the band mean over the g-points, element by element, against
exact rational arithmetic that has no rank routine and no `rebin` in it.  The oracle's `mrgrnk`, `rebin` and
`weights_to_bins` are restated from prose (futils does not build here); this is what holds them -- and the reading of
`rebin`'s edge rule that the kernels share with them -- to something written from the mathematics alone.  Runs without a GPU.

Bounds (none of them comes from what the code under test gives):
  * tau, and w0 wherever tau > tau_min and w0 < max_w0, relative, every element ............ 1e-12
    (`mixing_split`'s docstring adds up what double arithmetic may cost: 1e-13 where neighbouring rows are within a
    factor of two of each other; the project's RTOL_OPR is 1e-11)
  * the ill-conditioned case: no fixed bound.  More than 1e-12 (it is what it claims to be) and less than the analytic
    leakage bound ng^2 2^-53 max_k (v_above - v_k) / (v_k width_k), formed from the exact reference
  * every case of MIXING_CASES: the k-species' mixture is at least half of tau in at least 80 % of the elements, asserted
    on the exact reference.  OPACITY_CASES (the full inventory of terms) are compared too and not counted: the mixture
    is at least half of tau in 55-87 % of their elements, in 29 % of custom-varying-with-P's
  * pure absorption, the oracle's fluxes against `closed_for(case)` with tau from `mixing_split` (nothing of the oracle
    in the reference, from the tables to the fluxes): per bin max(2e-12, 10 x the difference of the two compilations),
    levels and TOA fluxes 1e-9 -- test_closed_forms_host.py's rule.  No bin of the reference alone misses it, so the
    fallback (10 x the oracle's distance with tau supplied) is not in use.  Albedo 0, element by element: RTOL_ELEMENT
    + 69.1 x 1e-12 = 7.0e-11 (BEAM_DEPTH: the tau behind the closed form is no longer the oracle's own)

Measured here (pytest -s prints each):
  * MIXING_CASES but the ill-conditioned one: tau 2.6e-13, w0 2.6e-13 at the worst (every-kind-scrambled; margin to
    1e-12: 3.9x), 1.3e-14 - 2.2e-13 on the others; steep-rows-2-decades 4.0e-13.  The two compilations agree to 1e-14
  * OPACITY_CASES: 1.1e-13 (nz65-g16-sorted)
  * the mixture's share of tau: at least half in 97-100 % of a case's elements, median 1.000
  * ill-conditioned-steep-rows (3 decades per g-point): 3.99e-12 from the exact split in BOTH compilations, which differ
    from each other by far less -- the two-build yardstick does not see it; leakage bound 1.40e-10 (35x above).  It is one
    ulp of E_7 per mixing step, four steps: the running sum of the ordered pair weights ends the seventh row an ulp
    short of the edge, and the eighth row, 1 000 times larger, fills the gap.  At 2 decades per g-point the same ulp
    is worth 3.97e-13, inside 1e-12: that case is held to the common bound
  * pure absorption with tau from `mixing_split`: IR per bin 8.4e-12 where the two compilations differ by 1.1e-11,
    largest share of a bin's bound 0.15; solar 8.2e-16, amean 1.0e-15; levels 2.5e-12, f_total 3.1e-12, OLR 2.2e-12 --
    the figures of test_closed_forms_host.py with tau supplied, to the digits shown
"""
import numpy as np
import pytest

import closed_forms as CF
from test_closed_forms_host import RTOL_ELEMENT, TOL_BIN, _oracle, check_albedo_zero, check_levels

RTOL_SPLIT = 1e-12
# An element of the direct beam that is at least 1e-30 of its bin's maximum has a cumulative optical depth over u0 of at
# most ln(1e30) = 69.1: a relative error d in tau moves it by at most 69.1 d.  Added to RTOL_ELEMENT where the closed
# form's tau is not the tau of the code under test.
BEAM_DEPTH = 69.1

_CACHE = {}


def _per_bin_rel(got, ref, where=None):
    """max over layers and g-points of |got - ref| / |ref|, per bin.  -> float64 [nw]"""
    got, ref = np.asarray(got, dtype=CF.LD), np.asarray(ref, dtype=CF.LD)
    d = np.abs(got - ref) / np.maximum(np.abs(ref), CF.LD(1e-300))
    if where is not None:
        d = np.where(where, d, 0)
    return np.max(d, axis=(0, 1)).astype(float)


def split_distance(parts, tau, w0):
    """Per bin: `tau` and `w0` (of the oracle, of the HIP path) from the exact split.  w0 where the reference neither
    zeroes nor caps it.  -> (tau [nw], w0 [nw])"""
    ok = np.asarray((parts.tau > CF.TAU_MIN) & (parts.w0 < CF.MAX_W0))
    return _per_bin_rel(tau, parts.tau), _per_bin_rel(w0, parts.w0, ok)


def case_parts(name):
    """-> tables, column, custom, exact split; computed once per process and left unchanged."""
    if ("parts", name) not in _CACHE:
        tables, column, custom = CF.mixing_case(name) if name in CF.MIXING_CASES else CF.opacity_case(name)
        _CACHE["parts", name] = (tables, column, custom, CF.mixing_parts(tables, column, custom))
    return _CACHE["parts", name]


def oracle_split(O, name):
    """One case through both compilations of the oracle.  -> tables, column, custom, exact split, and per compilation
    the per-bin distances (tau, w0) from it; the first compilation's (liborc.so, the oracle proper) is the GPU test's
    yardstick."""
    if ("oracle", name) not in _CACHE:
        tables, column, custom, parts = case_parts(name)
        dist = []
        for variant in ("", "fma"):
            o = _oracle(O, tables, len(column["T"]), 1, column, custom, variant)
            tau, w0 = o.opr()[:2]
            dist.append(split_distance(parts, tau, w0))
        _CACHE["oracle", name] = (tables, column, custom, parts, dist)
    return _CACHE["oracle", name]


ALL_CASES = list(CF.MIXING_CASES) + list(CF.OPACITY_CASES)


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_split_against_exact_arithmetic(O, name):
    tables, column, custom, parts, dist = oracle_split(O, name)
    print("\n    %s" % name)
    if name in CF.MIXING_CASES:
        frac, median = CF.check_mixing_case(parts)
        print("    the mixture is at least half of tau in %.0f %% of the elements, median share %.3f" % (100 * frac, median))
    for variant, (e_tau, e_w0) in zip(("liborc", "liborc_fma"), dist):
        print("    %-10s tau %.2e   w0 %.2e" % (variant, e_tau.max(), e_w0.max()))
        if name == CF.ILL_CONDITIONED:
            leak = CF.leakage_bound(parts, tables)
            print("    leakage bound %.2e" % leak)
            assert RTOL_SPLIT < e_tau.max() < leak, (e_tau.max(), leak)
            assert e_w0.max() < leak
        else:
            assert e_tau.max() <= RTOL_SPLIT and e_w0.max() <= RTOL_SPLIT, (e_tau, e_w0)
    assert np.any(np.asarray(parts.w0) > 0)          # w0 is compared on something


def test_exact_split_keeps_the_band_mean():
    """What `band_mean` rests on, in the reference's own terms: a mixing step conserves the weighted mean.  Exactly so
    for `_mix_step` (Fractions); and `mixing_split` against `band_mean` to the rounding of the np.longdouble sums."""
    from fractions import Fraction as F
    w = [F(1, 8), F(3, 8), F(1, 4), F(1, 4)]
    a, b = [F(1), F(5), F(2), F(7, 3)], [F(1, 7), F(0), F(4), F(4)]
    W = [1, 3, 2, 2]
    out = CF._mix_step(a, b, W)
    assert sum(x * y for x, y in zip(w, out)) == sum(x * (y + z) for x, y, z in zip(w, a, b))
    assert out == sorted(out)                         # the mixture comes out ascending
    # two g-points of weight 1/2, sums 1, 2, 3, 4 of weight 1/4 each: means (1 + 2) / 2 and (3 + 4) / 2
    assert CF._mix_step([F(0), F(2)], [F(1), F(2)], [1, 1]) == [F(3, 2), F(7, 2)]
    tables, column, custom, parts = case_parts("nk5")
    wg = np.asarray(tables.ktables[0]["weights"], dtype=CF.LD)
    mean = np.sum(parts.tau * wg[None, :, None], axis=1)
    tb = CF.band_mean(tables, column, custom)[0]
    assert float(np.max(np.abs(mean - tb) / tb)) <= 1e-17


def absorption_split(O, name):
    """One pure-absorption case: both compilations of the oracle, the closed forms on the oracle's own tau and the
    closed forms on `mixing_split`'s.  -> case, oracle, closed (tau supplied), closed (exact), two-build yardstick,
    per-bin distance of the oracle from the exact closed forms (ir, solar, amean) -- the GPU test's yardstick."""
    if ("absorption", name) not in _CACHE:
        from test_closed_forms_host import oracle_absorption
        case, o, closed_supplied, yard = oracle_absorption(O, name)
        closed = CF.closed_for(case)
        ir, sol = o.wrk_ir, o.wrk_sol
        dist = (CF.per_bin(ir.fup_a, ir.fdn_a, closed.ir.fup_a, closed.ir.fdn_a),
                CF.per_bin(sol.fup_a, sol.fdn_a, closed.sol.fup_a, closed.sol.fdn_a),
                CF.per_bin_one(sol.amean, closed.sol.amean))
        _CACHE["absorption", name] = (case, o, closed_supplied, closed, yard, dist)
    return _CACHE["absorption", name]


@pytest.mark.parametrize("name", list(CF.ABSORPTION_CASES))
def test_oracle_pure_absorption_from_tables_to_fluxes(O, name):
    """The oracle's fluxes against closed forms that take nothing from it: tau from `mixing_split`, the sweeps exact.
    Per bin max(2e-12, 10 x the two compilations' difference); a bin that missed that would be held to 10 x the
    oracle's distance with tau supplied, measured here -- no bin does (see the module's docstring)."""
    case, o, closed_supplied, closed, yard, dist = absorption_split(O, name)
    ir, sol = o.wrk_ir, o.wrk_sol
    supplied = (CF.per_bin(ir.fup_a, ir.fdn_a, closed_supplied.ir.fup_a, closed_supplied.ir.fdn_a),
                CF.per_bin(sol.fup_a, sol.fdn_a, closed_supplied.sol.fup_a, closed_supplied.sol.fdn_a),
                CF.per_bin_one(sol.amean, closed_supplied.sol.amean))
    print("\n    %s" % name)
    for what, e, y, s in zip(("IR", "solar", "amean"), dist, yard, supplied):
        bound = np.maximum(TOL_BIN, 10.0 * y)
        print("    %-5s per bin: worst %.2e (tau supplied %.2e, two compilations %.2e), largest share of the bound %.2f"
              % (what, e.max(), s.max(), y.max(), (e / bound).max()))
        assert np.all(e <= bound), (what, e, bound)
    check_levels(ir, sol, o.f_total, o.isr, o.olr, closed)
    if not np.any(case["albedo"]):
        check_albedo_zero(sol, closed.sol, RTOL_ELEMENT + BEAM_DEPTH * RTOL_SPLIT)
