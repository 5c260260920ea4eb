"""What can be held without a GPU about the exact two-stream reference (tests/exact_two_stream.py) and its fixtures
(tests/golden/exact_two_stream_*.npz, tests/golden/make_exact_two_stream.py):

  * the stored values are what the generator gives today, bit for bit, and 80 digits round to the same float64 as 50;
  * the two oracle-independent references agree: at w0 = 0 the exact solve equals the closed-form sweeps;
  * the unit responses add up to the full solve before rounding (linearity, 1e-40);
  * on the well-conditioned golden cases 36... the reference's own outputs and both oracle compilations lie within 1e-11
    of exact -- the bound test_gpu_golden._check puts on their yardsticks;
  * the fixture's conditions: the reference algorithm finite and within 1e-9 of exact on every new column;
  * every launch form of the GPU test has the columns its test counts;
  * the measure notices a change of one part in 1e6 in one layer's single-scattering albedo.
"""
import glob
import os
import sys

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")

import closed_forms as CF  # noqa: E402
import exact_two_stream as X  # noqa: E402
import exact_two_stream_cases as XC  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_exact_two_stream as M  # noqa: E402


@pytest.fixture(scope="module")
def G():
    return XC.load_golden()


@pytest.fixture(scope="module")
def E():
    return XC.load_exact()


@pytest.fixture(scope="module")
def cols(G, E):
    return XC.columns(G, E)


def test_fixtures_regenerate_bit_for_bit(G, E):
    fresh = M.generate(G)
    assert list(fresh) == list(E), "the arrays or their order changed"
    for k, v in fresh.items():
        v = np.asarray(v)
        assert v.shape == E[k].shape and v.dtype == E[k].dtype, k
        assert v.tobytes() == E[k].tobytes(), k
    files = glob.glob(os.path.join(M.HERE, "exact_two_stream_*.npz"))
    assert len(files) == len(M.split_parts(fresh)) and all(os.path.getsize(f) < 1024 * 1024 for f in files)


def test_eighty_digits_round_to_the_same_doubles(G, E):
    """ten columns again at 80 digits: golden stress (21, 33), smooth and paired cases, mixed and near-resonant columns,
    one response case, one multi-angle set, one unit matrix pair, one deviation list.  The same float64, element by
    element -- except where an element lies more than 30 decades under the largest of its row (a response that is 0, or
    e^-60000, in the mathematics: there the 50-digit solve leaves its own residual, 1e-50 of the row's largest, and so
    does the 80-digit one at 1e-80); those agree to 1e-40 of the row's largest, 30 decades under what any test measures."""
    again = {}
    for n in (21, 33, 40, 71):
        again.update(M.column_exact(G, "c%02d_" % n, dps=80))
    for n in (3, 5, 17):
        again.update(M.column_exact(E, "e%02d_" % n, dps=80))
    again.update(M.response_exact(G, "r02_", dps=80))
    again.update(M.multi_exact(E, "m01_", dps=80))
    again.update(M.unit_exact(E, "u02_", dps=80))
    again.update(M.deviations_exact(E, "e00_", dps=80))
    assert len(again) >= 50
    elements = 0
    for k, v in again.items():
        v, w = np.asarray(v), E[k]
        top = np.max(np.abs(w), axis=-1, keepdims=True)          # per row: a deviation's dB, a level of a unit matrix
        big = np.abs(w) > 1e-30 * top
        assert np.array_equal(v[big], w[big]), k
        assert np.all(np.abs(v - w) <= 1e-40 * top), k
        elements += int(np.sum(big))
    assert elements >= 3000


def test_every_form_has_its_columns(cols):
    """the counts tests/test_gpu_exact_two_stream.py asserts, from the shape rules alone; golden and new columns in each"""
    want = {(0, 1): 58, (0, 2): 86, (0, 3): 110, (2, 2): 86, (2, 3): 110, (4, 3): 80, (4, 4): 86, (4, 5): 108, (5, 2): 26, (5, 4): 41}
    for (form, slots), n in want.items():
        mine = [c for c in cols if XC.fits(c, form, slots)]
        assert len(mine) == n, (form, slots, len(mine))
        assert any(c.gold is None for c in mine) and any(c.gold is not None for c in mine), (form, slots)
    assert len(cols) == 144 and sum(c.nz >= 512 for c in cols) == 4
    assert sum(XC.natural_slots(c) > 3 for c in cols) == 34
    for form in (1, 3, 6):
        assert all(XC.fits(c, form, XC.natural_slots(c)) for c in cols)
    kinds = [c.name for c in cols if c.gold is None]
    assert sum("mixed" in k for k in kinds) == 18 and sum("res-top" in k for k in kinds) == 18 and sum("res-mid" in k for k in kinds) == 18


def test_resonant_layers_are_tuned(E):
    """the tuned layer's double lambda is within an ulp or two of (1 + off) / u0"""
    seen = 0
    for n in range(int(E["edge_n"][0])):
        kind = str(E["edge_kind"][n])
        if not kind.startswith("res-"):
            continue
        k = "e%02d_" % n
        off, u0 = float(kind[8:]), float(E[k + "sol_par"][0])
        assert 0.58 <= u0 <= 1.0
        nd = len(E[k + "tau"]) // (2 if E["edge_paired"][n] else 1)
        r = (0 if "top" in kind else nd // 2) * (2 if E["edge_paired"][n] else 1)
        lam = M.lambda_double(float(E[k + "w0"][r]), float(E[k + "g"][r]))
        assert abs(lam * u0 - (1.0 + off)) <= 1e-15, (kind, lam * u0 - 1.0)
        seen += 1
    assert seen == 36


def test_exact_equals_the_closed_forms_without_scattering(G, E):
    """w0 = 0: golden cases 4, 10, ... (w0 = g = 0; thin to thick, random Planck values) and two mixed columns with w0
    set to 0 (their g, tau = 0 and tau = 3e4 layers stay)"""
    picks = [(G, "c%02d_" % n, False) for n in (4, 10, 16, 22, 28, 34)] + [(E, "e09_", True), (E, "e01_", True)]
    for src, k, zero in picks:
        tau, g, bp = src[k + "tau"], src[k + "g"], src[k + "bplanck"]
        w0 = np.zeros_like(tau)
        assert zero or not np.any(src[k + "w0"])
        em, hs, tmin = (float(v) for v in src[k + "ir_par"])
        u0, rs = (float(v) for v in src[k + "sol_par"])
        fu, fd = X.exact_ir(tau, w0, g, em, bool(hs), tmin, bp)
        cu, cd = CF.ir_sweep(tau, bp, em, bool(hs), tmin)
        cu, cd = np.array([float(v) for v in cu]), np.array([float(v) for v in cd])
        s = max(np.max(np.abs(cu)), np.max(np.abs(cd)))
        assert max(np.max(np.abs(fu - cu)), np.max(np.abs(fd - cd))) <= 1e-13 * s, k
        am, su, sd = X.exact_solar(tau, w0, g, u0, rs)
        qu, qd, qa = (np.asarray(v, dtype=np.float64) for v in CF.solar_sweep(tau, u0, rs))
        s = max(np.max(np.abs(qu)), np.max(np.abs(qd)))
        assert max(np.max(np.abs(su - qu)), np.max(np.abs(sd - qd))) <= 1e-13 * s, k
        assert np.max(np.abs(am - qa)) <= 1e-13 * np.max(np.abs(qa)), k


def test_unit_responses_add_up_to_the_full_solve(G, E):
    """sum_k B_k unit_k = the full solve, before rounding, to 1e-40 of the largest flux.  At 80 digits: case 21 loses
    thirteen of them (that is its condition), and the statement is about the equations, not about the digits."""
    for src, k in ((G, "c21_"), (G, "c40_"), (E, "e00_"), (E, "e10_")):
        em, hs, tmin = (float(v) for v in src[k + "ir_par"])
        with mpmath.workdps(80):
            col = X.IrColumn(src[k + "tau"], src[k + "w0"], src[k + "g"], em, bool(hs), tmin)
            B = [mpmath.mpf(float(b)) for b in src[k + "bplanck"]]
            fu, fd = col.solve_mp(B)
            su, sd = [mpmath.mpf(0)] * len(B), [mpmath.mpf(0)] * len(B)
            for kk, b in enumerate(B):
                u, d = col.unit_mp(kk)
                su = [a + b * v for a, v in zip(su, u)]
                sd = [a + b * v for a, v in zip(sd, d)]
            s = max(max(abs(v) for v in fu), max(abs(v) for v in fd))
            worst = max(max(abs(a - b) for a, b in zip(su, fu)), max(abs(a - b) for a, b in zip(sd, fd))) / s
            assert worst <= mpmath.mpf("1e-40"), (k, worst)


def test_reference_true_error_per_case(O, cols):
    """The table of the reference's true error per golden case (printed: -s shows it), and the bound on the
    well-conditioned ones: 1e-11 on cases 36..., stored outputs and both oracle compilations."""
    for c in cols:
        c.ref_errors(O)
        assert c.ref_finite, c.name             # every column, golden stress cases and new ones: a yardstick that is a number
    print("\n case  nz     IR        solar     amean     (reference's true error / scale)")
    for c in cols:
        if c.gold is None:
            continue
        r, s = c.ref_errors(O), c.scales()
        rel = {q: r[q] / s[q] for q in r}
        print("  %s %4d  %.2e  %.2e  %.2e" % (c.name, c.nz, rel["ir"], rel["sol"], rel["amean"]))
        if int(c.name[1:]) >= 36:
            assert max(rel.values()) <= 1e-11, (c.name, rel)
    by = {c.name: c.ref_errors(O)["ir"] / c.scales()["ir"] for c in cols if c.gold is not None}
    assert 1e-3 < by["c21"] < 1e-2 and 1e-4 < by["c33"] < 1e-2          # the ill-conditioned ones are what they were measured to be


def test_conditions_of_the_new_columns(O, E):
    """finite in both compilations, and within 1e-9 of exact: no new column loosens its own bound beyond 1e-8"""
    errs = M.check_conditions(E, O)
    assert len(errs) >= 230 and max(errs.values()) <= M.REF_ERR_MAX


def test_the_measure_notices_a_small_change(O, cols):
    """The oracle on a column whose every w0 is raised by 1e-6 relative fails the criterion on the smooth golden cases
    and on the new columns: a kernel that treats w0 that much differently would."""
    seen = 0
    for c in cols:
        if c.group.startswith("golden stress") or c.group in ("golden c21", "golden c33") or c.nz < 5:
            continue
        w0 = c.w0 * (1.0 + 1e-6)
        a = O.two_stream_ir(c.tau, w0, c.g, c.ir_par[0], bool(c.ir_par[1]), c.ir_par[2], c.bp)
        b = O.two_stream_solar(c.tau, w0, c.g, c.sol_par[0], c.sol_par[1])
        e, r, s = c.errors([a[0], a[1], b[2], b[3], b[0]]), c.ref_errors(O), c.scales()
        seen += 1
        assert any(not XC.allowed(e[q], s[q], r[q]) for q in e), (c.name, e, r)
    assert seen >= 100
