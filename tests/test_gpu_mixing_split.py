"""The HIP path's tau and w0 (`r.opr()`) against `closed_forms.mixing_split`: how the random-overlap mixing step splits
the band mean over the g-points, element by element, against exact rational arithmetic -- no sort routine, no `rebin`,
nothing of oracle/.  Every other test of the split compares with the oracle, written from the same reading of the
reference as the kernels: a wrong entry in a window table, a skip class that fires once too often or a shared misreading
of `rebin`'s edge rule passes there whenever the oracle agrees on the tested inputs.

Every form the step can take is run:
  * the four FORMS of test_gpu_closed_forms.py (group-of-lanes and lane-per-item opacity kernels, fused grid on and off)
    on every 8-g-point case: the assembly block with its per-wave skip classes (ascending tables), the compiler network
    with the window rebin (scrambled ones), `k_opacity_coop`, the paired form (doubled columns);
  * CLIMA_HIP_REBIN=stream around the handle's construction: the streaming rebin, single-edge, and multi-edge with
    W_MULTI_EDGE; W_SINGLE_EDGE takes the streaming single-edge form by itself (the window tables refuse it);
  * the other g-point counts: the padded group-of-lanes form;
  * TOA_fluxes_batch and TOA_fluxes_batch_tensors on three columns, the case's last: `opr()` then holds that column
    (where the batch runs one call per column; test_split_after_a_column_batch says what is compared otherwise);
  * a handle with set_bin_shard(1, 3), compared on the rank's own opacity bins (`bin_shard()`): wave-mates change there.

Bounds -- none of them taken from what the kernels give:
  * tau, and w0 wherever tau > tau_min and w0 < max_w0, per bin, relative: max(RTOL_OPR = 1e-11, 10 x the oracle's
    distance from the exact split on that bin, test_mixing_split_host.py).  The keys' pair index costs at most
    2^-44 = 5.7e-14, so the floor rules everywhere but on the ill-conditioned case; each test prints which of the two
    ruled and the largest share of the bound used, and on the ill-conditioned case whether the HIP path or the oracle is
    nearer to exact (DESIGN.md section 7 claims the closed-form rows are the more accurate of the two)
  * pure absorption, HIP fluxes against `closed_for(case)` with tau from `mixing_split` (no tau supplied):
    test_gpu_closed_forms.py's rule, per bin max(2e-10, 10 x the oracle's distance from the same closed forms on that
    bin), levels and TOA fluxes 1e-9

No test here reads the reference's tree or needs oracle/_ref.

Measured on an MI355X (worst over the cases; pytest -s prints each):
  * every case but the ill-conditioned one, tau and w0 alike: group-of-lanes kernel 2.3e-13, lane-per-item tile
    6.2e-13 (fused or not), streaming rebin 2.3e-13 / 6.3e-13, other g-point counts 3.8e-13 (padded),
    batches 3.8e-13 (host and device route the same), bin shard 3.4e-13.  Largest share of a bin's bound 0.063
    (steep-rows-2-decades, streaming, lane-per-item); the floor ruled in every one (margin to 1e-11: 16x)
  * ill-conditioned-steep-rows, where the oracle is 3.99e-12 from exact and 10 x that rules: the lane-per-item tile
    (the assembly block: every row stands alone and is rebinned as sum_j w_j key) 2.0e-13 -- 20 times nearer to exact than
    the oracle, which is DESIGN.md section 7's claim --; the group-of-lanes kernel 2.1e-12, nearer than the oracle too;
    the streaming rebin in the lane-per-item tile 4.2e-12, where the oracle is the nearer by a hair.  Largest share of
    the bound 0.105
  * one-launch batches (more than 64 layers): tau_band of the last column within 2e-13 of the exact split's mean
  * pure absorption, nothing supplied: IR per bin 5.1e-12 where the oracle is 8.4e-12 from the same closed forms
    (0.025 of the bound), solar 9.5e-15, amean 9.2e-15; levels 2.8e-12, OLR 6.8e-13 (margin to 1e-9: 350x); albedo 0
    element by element 3.5e-12 (bound 7.0e-10: the HIP tau is up to 5e-14 from exact, 69 optical depths down the beam)
"""
import numpy as np
import pytest

import closed_forms as CF
from test_closed_forms_host import RTOL_ELEMENT, _rel, check_albedo_zero, check_levels
from test_gpu_closed_forms import FORMS, TOL_BIN, _handle
from test_gpu_parity import RTOL_OPR, RTOL_TOA, TOL_LEVEL
from test_mixing_split_host import ALL_CASES, BEAM_DEPTH, absorption_split, oracle_split, split_distance

pytestmark = pytest.mark.gpu


def _ng(name):
    return (CF.MIXING_CASES[name][1] if name in CF.MIXING_CASES else CF.OPACITY_CASES[name][0]).get("ng", 8)


G8 = [n for n in ALL_CASES if _ng(n) == 8]
OTHER_G = [n for n in ALL_CASES if _ng(n) != 8]


def hold(name, label, parts, yard, tau, w0, bins=None):
    """tau, w0 of the HIP path against the exact split, per bin, to max(RTOL_OPR, 10 x the oracle's distance).
    `yard`: the oracle's per-bin distances (tau, w0); `bins`: the bins to compare (a sharded rank's own)."""
    sel = slice(None) if bins is None else bins
    dist = split_distance(parts, tau, w0)
    for what, e, y in zip(("tau", "w0"), dist, yard):
        e, y = e[sel], y[sel]
        bound = np.maximum(RTOL_OPR, 10.0 * y)
        i = int(np.argmax(e / bound))
        print("    %s %s %s: worst %.2e (oracle %.2e); largest share of the bound %.3f, ruled by %s"
              % (name, label, what, e.max(), y.max(), (e / bound)[i], "the floor" if bound[i] == RTOL_OPR else "10 x the oracle"))
        assert np.all(e <= bound), (what, e, bound)
    if name == CF.ILL_CONDITIONED:
        h, o = float(dist[0][sel].max()), float(yard[0][sel].max())
        print("    %s %s: HIP %.2e from exact, oracle %.2e: %s is nearer" % (name, label, h, o, "the HIP path" if h < o else "the oracle"))


def _radiate(tables, column, custom, form="coop-fused", nzen=1):
    r = _handle(tables, len(column["T"]), nzen, form, custom=custom)
    r.radiate(*column.args())
    return r


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", G8)
def test_split_in_every_launch_form(O, hip_lib, name, form):
    tables, column, custom, parts, dist = oracle_split(O, name)
    print()
    tau, w0 = _radiate(tables, column, custom, form).opr()[:2]
    hold(name, form, parts, dist[0], tau, w0)


@pytest.mark.parametrize("form", ["coop-separate", "lanes-fused"])
@pytest.mark.parametrize("name", G8)
def test_split_with_the_streaming_rebin(O, hip_lib, name, form, monkeypatch):
    """CLIMA_HIP_REBIN=stream, read when the handle is made: the streaming rebin in place of the window form --
    single-edge for the Gauss-Legendre weights and W_SINGLE_EDGE, multi-edge for W_MULTI_EDGE."""
    tables, column, custom, parts, dist = oracle_split(O, name)
    monkeypatch.setenv("CLIMA_HIP_REBIN", "stream")
    r = _handle(tables, len(column["T"]), 1, form, custom=custom)
    monkeypatch.delenv("CLIMA_HIP_REBIN")
    r.radiate(*column.args())
    print()
    tau, w0 = r.opr()[:2]
    hold(name, "stream " + form, parts, dist[0], tau, w0)


# (the ids end in -0 so that the cases keep the names under which earlier results are filed)
@pytest.mark.parametrize("name", OTHER_G, ids=[n + "-0" for n in OTHER_G])
def test_split_at_other_g_point_counts(O, hip_lib, name):
    """The group-of-lanes kernel with the next power of two of lanes per item, the lanes beyond ng padded."""
    tables, column, custom, parts, dist = oracle_split(O, name)
    r = _handle(tables, len(column["T"]), 1, "coop-fused", custom=custom)
    r.radiate(*column.args())
    print()
    tau, w0 = r.opr()[:2]
    hold(name, "padded", parts, dist[0], tau, w0)


def _three_columns(column):
    """Two other columns in front of the case's: warmer and denser, cooler and thinner."""
    from clima_amd import synthetic as S
    cols = []
    for dT, f in ((7.0, 1.3), (-5.0, 0.8)):
        c = S.Column({k: (np.array(v, copy=True, order="K") if isinstance(v, np.ndarray) else v) for k, v in column.items()})
        c["T"] = c["T"] + dT
        c["T_surface"] = float(c["T_surface"]) + dT
        c["densities"] = np.asfortranarray(c["densities"] * f)
        cols.append(c)
    return cols + [column]


@pytest.mark.parametrize("route", ["host", "tensors"])
@pytest.mark.parametrize("name", list(CF.MIXING_CASES))
def test_split_after_a_column_batch(O, hip_lib, name, route, monkeypatch):
    """A batch that runs one call per column (at most 64 layers, other g-point counts) works in the handle's own buffers
    and `opr()` holds the last column's.  The one-launch form (8 g-points, more than 64 layers: the lane-per-item tile
    inside the fused grid, 64 columns per launch) leaves its optical properties in the batch arena BY DESIGN
    (radtran_dev.h, `Holds::batch_left`): of the last column the handle keeps the spectra and the band optical depths, which
    are compared with the exact split's weighted mean; the split itself is then compared on the same batch with
    CLIMA_HIP_BATCH_ONE_LAUNCH=0 (read per call), and the tile's split inside the fused grid is
    test_split_in_every_launch_form's lanes-fused."""
    from test_gpu_batch_device import tensors
    tables, column, custom, parts, dist = oracle_split(O, name)
    nz = len(column["T"])
    r = _handle(tables, nz, 1, "coop-fused", custom=custom)
    cols = _three_columns(column)
    run = (lambda: r.TOA_fluxes_batch(cols)) if route == "host" else (lambda: r.TOA_fluxes_batch_tensors(**tensors(cols, r.np)))
    print()
    if tables.ng == 8 and nz > 64:
        run()
        wg = np.asarray(tables.ktables[0]["weights"], dtype=CF.LD)
        mean = np.sum(parts.tau * wg[None, :, None], axis=1)                     # TOA-first; wrk_*.tau_band ground-first
        nsol, ir0 = len(tables.sol_wavl) - 1, tables.nw - (len(tables.ir_wavl) - 1)
        e = max(_rel(np.asarray(r.wrk_sol.tau_band)[::-1], mean[:, :nsol]), _rel(np.asarray(r.wrk_ir.tau_band)[::-1], mean[:, ir0:]))
        print("    %s batch %s, one launch: tau_band of the last column %.2e" % (name, route, e))
        assert e <= RTOL_OPR
        monkeypatch.setenv("CLIMA_HIP_BATCH_ONE_LAUNCH", "0")
    run()
    tau, w0 = r.opr()[:2]
    hold(name, "batch " + route, parts, dist[0], tau, w0)


@pytest.mark.parametrize("name", list(CF.MIXING_CASES))
def test_split_on_a_bin_shard(O, hip_lib, name):
    tables, column, custom, parts, dist = oracle_split(O, name)
    r = _handle(tables, len(column["T"]), 1, "coop-fused", custom=custom)
    r.set_bin_shard(1, 3)
    op_lo, op_n = r.bin_shard()[:2]
    assert 0 < op_n < tables.nw and op_lo > 0
    r.radiate(*column.args())
    print()
    tau, w0 = r.opr()[:2]
    hold(name, "shard 1 of 3, bins %d-%d" % (op_lo, op_lo + op_n - 1), parts, dist[0], tau, w0, slice(op_lo, op_lo + op_n))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CF.ABSORPTION_CASES))
def test_pure_absorption_from_tables_to_fluxes(O, hip_lib, name, form):
    """HIP fluxes against closed forms that take nothing from the code under test and nothing from the oracle: tau from
    `mixing_split`, the sweeps exact."""
    case, _, _, closed, _, dist = absorption_split(O, name)
    r = _handle(case["tables"], case["nz"], case["nzen"], form, case["scalars"], case["albedo"], case["emissivity"])
    isr, olr = r.TOA_fluxes(*case["column"].args())
    assert np.all(r.opr()[1] == 0.0)
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
    check_levels(ir, sol, r.f_total, isr, olr, closed, TOL_LEVEL, RTOL_TOA)
    if not np.any(case["albedo"]):
        check_albedo_zero(sol, closed.sol, RTOL_ELEMENT + BEAM_DEPTH * RTOL_OPR)
