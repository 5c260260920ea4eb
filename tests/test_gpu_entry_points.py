"""Every entry point on every row of the launch-form table (tests/launch_forms.py): the single call, the resident
pipeline, the host and device column batches with spectra, IR-only calls and radiate_ir_batch on stored opacities, the
Jacobians.  tests/test_launch_form_table.py shows, without a device, that the rows reach every kernel instance the
planner can choose; here each of them computes what the oracle (or, where the contract is an equality, the column's own
call) computes.  Every comparison uses the helper and the bound the project already has for that entry point.

E1  TOA_fluxes against the oracle at the default coop_items and at 0          test_gpu_parity._compare_once
E2  upload_column + radiate_resident x 3, deferring / not / synchronous         bitwise; merged_integrations
E3  TOA_fluxes_batch, 5 / 1 / 4 columns in chunks of 2, rows and spectra        bitwise against each column's own call
E4  TOA_fluxes_batch_tensors(sync=False) with the same request                  bytewise the host batch
E5  the batch's columns 0 and 4 against the oracle                              RTOL_TOA, TOL_LEVEL
E6  IR-only call and radiate_ir_batch (general and response form)               _compare_once; test_gpu_ir_green.TOL_LEVEL
E7  ir_jacobian against the exact Jacobian, ir_jacobian_reduced                 test_gpu_ir_jacobian.TOL; bitwise

Worst figures over all rows, measured on an MI355X (bound in brackets; test_worst_figures prints them):
  E1 OLR, ISR (relative)                8.7e-12  [1e-9]   r2-150
  E1 level rows                         9.5e-12  [1e-9]   c257
  E5 batch OLR, ISR (relative)          2.7e-11  [1e-9]   r2c-70
  E5 batch level rows                   7.6e-11  [1e-9]   r2c-70
  E6 IR-only level rows                 9.7e-12  [1e-9]   c257
  E6 radiate_ir_batch, ir_green = 0     1.5e-11  [2e-11]  nz2
  E6 radiate_ir_batch, ir_green = 2     1.1e-11  [2e-11]  g4-70
  E7 ir_jacobian, of the largest entry  2.7e-10  [5e-10]  w512
  E7 ir_jacobian, column 0 of its own   1.3e-14  [5e-10]  p258
  E2, E3, E4 and ir_jacobian_reduced are equalities.

E7, conditioning.  A column of the Jacobian on its own scale (ir_jacobian_oracle.column_scaled_error) is held to 5e-10 by
the surface column on every row, by the columns nz/2+1 and nz (the top layer) on the rows with custom optical properties
only: elsewhere the upper layers are optically thin, their unit responses carry the source slope 1 / tau, and the
yardstick itself -- the same exact Jacobian built on the oracle's other compilation (FMA contraction on) -- differs
from the first by as much as the library does (test_gpu_ir_jacobian's docstring says the same of these columns).
Those rows (CONDITIONED) are held to the rule of test_gpu_fuzz, the larger of 5e-10 and 10 yardsticks:
  column nz      worst error 3.9e-05 at w225 (yardstick 2.6e-05); closest to its bound w512, 2.4e-07 (yardstick 3.4e-08)
  column nz/2+1  worst error 5.4e-07 at w512 (yardstick 1.5e-07); closest to its bound h170, 1.2e-09 (yardstick 1.9e-10)
over all rows the error is between 0.4 and 7.2 yardsticks.  Every row, conditioned or not, is also held to 5e-10 of the
largest entry of the compared columns, test_gpu_ir_jacobian's own measure.

E2, merged_integrations: (2, 1) wherever the call's prep launch clears nothing, (0, 3) elsewhere -- the rule
include/clima_radtran_hip.h states.  Of the fused rows these are the half-wave ones; the unfused rows with one g-point
group or more than 512 layers (g4-70, b513) have nothing cleared in the prep launch either, and merge too.

E3 on the rows of exact pairs: a single call on such a column takes the paired form, a chunk never does, so the
column's own call in the chunk's form is a batch of that column alone (the two forms agree to 1e-16 of ISR, not bit
for bit); E5 holds the same batch to the oracle.

What the rows found: radiate(compute_opacity=False) directly after a one-launch batch ran on the handle's own optical
properties -- an earlier call's, or none -- where radiate_ir_batch and ir_jacobian refuse; it refuses now (every
one-launch row, first h65).  The same class, found by reading once the handle's state was stated in one place (Holds,
radtran_dev.h): opr() after a one-launch batch copied out an earlier call's optical properties (E3 holds it to the
refusal, and on the other rows to the single call's arrays), and an IR-only call after a change of shard ran on bins
the handle never computed (test_stored_opacities_cover_the_shard_asked_for)."""
import numpy as np
import pytest

import ir_jacobian_oracle as J
import launch_forms as LF
from test_gpu_batch_device import tensors
from test_gpu_batch_spectra import NAMES, device_spectra
from test_gpu_ir_green import TOL_LEVEL as TOL_IR_BATCH
from test_gpu_ir_jacobian import TOL as TOL_JACOBIAN
from test_gpu_merged_integration import _assert_same_state
from test_gpu_parity import RTOL_TOA, TOL_LEVEL, _compare_once, _custom_props, _scaled

pytestmark = pytest.mark.gpu

NCOL = 5
WORST = {}     # figure -> (value, row, bound)
JACOBIAN_REFUSAL = r"^ir_jacobian: the response form takes 4 <= nz <= 512 \(nz = %d\)$"
# E7: rows whose Jacobian columns are held to the rule of test_gpu_fuzz (conditioning, not a defect: see the module docstring)
CONDITIONED = frozenset(
    "s64 h65 h100 h130 h170 h224 w225 w257 w350 w512 p230 p258 p402 c256 c257 r1-70 r1-130 r1-200 r2-100 r2-150 r2-200 r2-300 "
    "g4-70 g16-100 g16-300 g32-40 z17-100 z17-130".split())


class OtherCompilation:
    """the oracle's two-stream solver as its other compilation (FMA contraction on): the yardstick of test_gpu_fuzz"""

    def __init__(self, O):
        self.O = O

    def two_stream_ir(self, *a):
        return self.O.two_stream_ir(*a, variant="fma")


IR_BATCH_REFUSAL = r"^radiate_ir_batch: nz = %d exceeds what the wave two-stream kernel holds \(512\)$"


def note(figure, value, row, bound):
    value = float(value)
    print("%-8s %-34s %.2e  [%.0e]" % (row.name, figure, value, bound))
    if value >= WORST.get(figure, (-1.0,))[0]:
        WORST[figure] = (value, row.name, bound)


def configure(row, h, oracle=False):
    """the row's settings on a handle or an oracle object"""
    if oracle:
        if row.scalars():
            h.set_scalars(**row.scalars())
    else:
        for k, v in row.scalars().items():
            setattr(h, k, v)
    surf = row.surface()
    if surf is not None:
        if oracle:
            h.set_surface_albedo(surf[0])
            h.set_surface_emissivity(surf[1])
        else:
            h.surface_albedo, h.surface_emissivity = surf
    if row.custom:
        h.set_custom_optical_properties(*_custom_props())
    return h


class RowState:
    """a row's handles, oracle and results, made on first use and kept for the module"""

    def __init__(self, row, O):
        self.row, self.O, self.kept = row, O, {}

    def handle(self, key=None, coop0=False):
        """key None: a fresh handle nobody else uses"""
        from clima_amd.radtran import Radtran
        if key is not None and key in self.kept:
            return self.kept[key]
        r = configure(self.row, self.row.make(Radtran))
        assert r.coop_items == LF.DEFAULT_COOP_ITEMS and r.fused
        if coop0:
            r.coop_items = 0
        if key is not None:
            self.kept[key] = r
        return r

    def oracle(self):
        if "oracle" not in self.kept:
            self.kept["oracle"] = configure(self.row, self.row.make(self.O.OracleRadtran), oracle=True)
        return self.kept["oracle"]

    def columns(self):
        if "columns" not in self.kept:
            self.kept["columns"] = self.row.columns(NCOL)
        return self.kept["columns"]

    def levels(self):
        return [self.row.nz, 0, self.row.nz // 2]

    def host_batch(self):
        """(handle, results of the 5-column host batch with rows and spectra, the state it left)"""
        if "host_batch" not in self.kept:
            r = self.handle("batch")
            got = r.TOA_fluxes_batch(self.columns(), return_fluxes=True, spectra_levels=self.levels())
            self.kept["host_batch"] = (r, got, left_state(r))
        return self.kept["host_batch"]

    def own_calls(self):
        """every column's own TOA_fluxes call on a second handle: (ISR, OLR), the five rows, the state"""
        if "own" not in self.kept:
            one = self.handle("own", coop0=self.row.one_launch)
            out = []
            for c in self.columns():
                if self.row.doubled:
                    # A single call on a column of exact pairs takes the paired form, a chunk never does (its columns are
                    # not known to be all pairs): two kernels that agree to rounding (1e-16 of ISR measured), not bit for
                    # bit.  The column's own call in the chunk's form is a batch of that column alone.
                    isr, olr = one.TOA_fluxes_batch([c])
                    toa = (isr[0], olr[0])
                else:
                    toa = one.TOA_fluxes(*c.args())
                out.append((toa, left_state(one)))
            self.kept["own"] = out
        return self.kept["own"]


def left_state(r):
    """level rows, f_total, and the per-bin arrays a batch has to leave as the last column's"""
    return dict(ir_fup_n=np.array(r.wrk_ir.fup_n), ir_fdn_n=np.array(r.wrk_ir.fdn_n), sol_fup_n=np.array(r.wrk_sol.fup_n),
                sol_fdn_n=np.array(r.wrk_sol.fdn_n), f_total=np.array(r.f_total), ir_fup_a=np.array(r.wrk_ir.fup_a),
                ir_fdn_a=np.array(r.wrk_ir.fdn_a), sol_fup_a=np.array(r.wrk_sol.fup_a), sol_fdn_a=np.array(r.wrk_sol.fdn_a),
                sol_amean=np.array(r.wrk_sol.amean), ir_tau_band=np.array(r.wrk_ir.tau_band),
                sol_tau_band=np.array(r.wrk_sol.tau_band))


ROW_NAMES = ("ir_fup_n", "ir_fdn_n", "sol_fup_n", "sol_fdn_n", "f_total")


def assert_state_is(r, want, what):
    got = left_state(r)
    for k in ROW_NAMES + ("ir_fup_a", "sol_amean", "ir_tau_band", "sol_tau_band"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


@pytest.fixture(scope="module")
def states(O):
    kept = {}

    def get(row):
        if row.name not in kept:
            kept[row.name] = RowState(row, O)
        return kept[row.name]
    return get


def level_errors(rows, o):
    """the five level rows against the oracle's state, each channel's up and down on their common scale (_compare_once)"""
    worst = 0.0
    for ch, w in (("ir", o.wrk_ir), ("sol", o.wrk_sol)):
        scale = max(float(np.max(np.abs(w.fup_n))), float(np.max(np.abs(w.fdn_n))), 1e-300)
        worst = max(worst, float(np.max(np.abs(rows[ch + "_fup_n"] - w.fup_n))) / scale,
                    float(np.max(np.abs(rows[ch + "_fdn_n"] - w.fdn_n))) / scale)
    return max(worst, _scaled(rows["f_total"], o.f_total))


rows = pytest.mark.parametrize("row", LF.ROWS, ids=repr)


# ------------------------------------------------------------------ E1
@rows
def test_e1_single_call_against_the_oracle(states, row):
    s = states(row)
    o, col = s.oracle(), row.column()
    for key, coop0 in (("single", False), ("single0", True)):
        r = s.handle(key, coop0)
        isr, olr = _compare_once(r, o, col)
        isr_o, olr_o = o.TOA_fluxes(*col.args())
        note("E1 OLR, ISR (relative)", max(abs(olr - olr_o) / abs(olr_o), abs(isr - isr_o) / max(abs(isr_o), 1e-300)), row, RTOL_TOA)
        note("E1 level rows", level_errors(left_state(r), o), row, TOL_LEVEL)
        assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ E2
@rows
def test_e2_resident_pipeline(states, row):
    s = states(row)
    A, B = row.columns(2)
    pair = []
    for defer in (True, False):
        h = s.handle(coop0=True)
        h.defer_integration = defer
        for c in (A, B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
        pair.append(h)
    r, ref = pair
    _assert_same_state(r, ref, "deferring against not")
    sync = s.handle(coop0=True)
    sync.TOA_fluxes(*A.args())
    _assert_same_state(r, sync, "pipelined against the synchronous call")
    # the pending integration goes out in the next call's prep launch exactly where that launch clears nothing
    # (include/clima_radtran_hip.h, radtran_defer_integration_set): of the fused rows, the half-wave ones
    plan = row.plans["single0"]
    merged = 2 if not plan.prep_clears else 0
    if plan.fused[0] != LF.NONE:
        assert (merged == 2) == (plan.fused[0] == LF.HALF)
    assert r.merged_integrations == (merged, 3 - merged)
    assert ref.merged_integrations == (0, 0)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0 and sync.fused_fallbacks == 0


# ------------------------------------------------------------------ E3
def assert_batch_is_own_calls(got, own, levels, what):
    isr, olr, fl, spec = got
    for c, (toa, st) in enumerate(own):
        assert (isr[c], olr[c]) == toa, (what, c)
        for k, name in enumerate(ROW_NAMES):
            np.testing.assert_array_equal(fl[:, k, c], st[name], err_msg="%s: column %d %s" % (what, c, name))
        for name in NAMES:
            np.testing.assert_array_equal(spec[name][:, :, c], st[name][levels], err_msg="%s: column %d %s" % (what, c, name))


@rows
def test_e3_host_batch(states, row):
    from clima_amd.radtran import ClimaException
    s = states(row)
    cols, own = s.columns(), s.own_calls()
    r, got, state = s.host_batch()
    assert got[2].shape == (row.nz + 1, 5, NCOL)
    assert_batch_is_own_calls(got, own, s.levels(), "5 columns")
    for k in own[-1][1]:
        np.testing.assert_array_equal(state[k], own[-1][1][k], err_msg="the state after 5 columns: " + k)
    for n in (1, 4):
        r.TOA_fluxes_batch(cols[:n])
        assert_state_is(r, own[n - 1][1], "the state after %d column(s)" % n)
    warm = type(cols[3])(cols[3], T=np.asarray(cols[3]["T"]) + 2.0)     # (the batch of 4 left column 3's state)
    if row.one_launch:
        with pytest.raises(ClimaException, match="needs opacities"):
            r.radiate(*warm.args(), compute_solar=False, compute_opacity=False)
        with pytest.raises(ClimaException, match="needs opacities"):     # (it copied out an earlier call's, or zeros)
            r.opr()
    else:
        # one call per column is bit for bit the single call: the optical properties the batch left are column 3's
        single = s.handle()
        single.radiate(*cols[3].args())
        for got_a, want_a, name in zip(r.opr(), single.opr(), ("tau", "w0", "g", "tau_band")):
            np.testing.assert_array_equal(got_a, want_a, err_msg="opr() after the batch of 4: " + name)
        o = s.oracle()
        o.radiate(*cols[3].args())
        _compare_once(r, o, warm, compute_solar=False, compute_opacity=False)
    assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ E4
@rows
def test_e4_device_batch(states, row):
    s = states(row)
    r, want, want_state = s.host_batch()
    r.TOA_fluxes_batch(s.columns(), return_fluxes=True, spectra_levels=s.levels())     # (E3 may have left a shorter batch's state)
    got = device_spectra(r, s.columns(), s.levels(), sync=False)
    for g, w, name in zip(got, want, ("ISR", "OLR", "fluxes")):
        assert g.tobytes() == w.tobytes(), name
    assert sorted(got[3]) == sorted(NAMES)
    for name in NAMES:
        assert np.ascontiguousarray(got[3][name]).tobytes() == np.ascontiguousarray(want[3][name]).tobytes(), name
    assert_state_is(r, want_state, "the state after the device batch")
    isr, olr, fl = r.TOA_fluxes_batch_tensors(**tensors(s.columns(), r.np), return_fluxes=True, sync=False)
    r.synchronize()
    assert isr.cpu().numpy().tobytes() == want[0].tobytes() and olr.cpu().numpy().tobytes() == want[1].tobytes()
    assert np.transpose(fl.cpu().numpy(), (2, 1, 0)).tobytes() == np.ascontiguousarray(want[2]).tobytes()
    assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ E5
@rows
def test_e5_batch_against_the_oracle(states, row):
    s = states(row)
    _, (isr, olr, fl, _), _ = s.host_batch()
    o = s.oracle()
    for c in (0, NCOL - 1):
        isr_o, olr_o = o.TOA_fluxes(*s.columns()[c].args())
        e_toa = max(abs(olr[c] - olr_o) / abs(olr_o), abs(isr[c] - isr_o) / max(abs(isr_o), 1e-300))
        e_lv = level_errors({name: fl[:, k, c] for k, name in enumerate(ROW_NAMES)}, o)
        note("E5 batch OLR, ISR (relative)", e_toa, row, RTOL_TOA)
        note("E5 batch level rows", e_lv, row, TOL_LEVEL)
        assert e_toa <= RTOL_TOA and e_lv <= TOL_LEVEL, (c, e_toa, e_lv)


# ------------------------------------------------------------------ E6
def ir_batch_columns(col, nz):
    """the profile, one level +3 K, the surface -1 K, two neighbours +0.1 K"""
    T = np.repeat(np.asarray(col["T"], dtype=float)[:, None], 4, axis=1)
    Ts = np.full(4, float(col["T_surface"]))
    T[nz // 2, 1] += 3.0
    Ts[2] -= 1.0
    T[0, 3] += 0.1
    T[min(1, nz - 1), 3] += 0.1
    return Ts, T


@rows
def test_e6_ir_on_stored_opacities(states, row):
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException
    s = states(row)
    r, o, col, nz = s.handle("single0", coop0=True), s.oracle(), row.column(), row.nz
    r.radiate(*col.args())           # (w0 left to the fused grid where the row is fused)
    o.radiate(*col.args())
    warm = S.Column(col, T=np.asarray(col["T"]) + 2.0, T_surface=float(col["T_surface"]) + 2.0)
    _compare_once(r, o, warm, compute_solar=False, compute_opacity=False)
    note("E6 IR-only level rows", level_errors(left_state(r), o), row, TOL_LEVEL)
    Ts, T = ir_batch_columns(col, nz)
    if nz > 512:
        with pytest.raises(ClimaException, match=IR_BATCH_REFUSAL % nz):
            r.radiate_ir_batch(Ts, T)
        return
    want = []
    for c in range(4):
        o.radiate(*S.Column(col, T=T[:, c].copy(), T_surface=Ts[c]).args(), compute_solar=False, compute_opacity=False)
        want.append((np.array(o.wrk_ir.fup_n), np.array(o.wrk_ir.fdn_n), np.array(o.f_total)))
    for mode in (0, 2) if nz >= 4 else (0,):
        n0 = r.ir_green_batches
        r.ir_green = mode
        got = r.radiate_ir_batch(Ts, T)
        assert r.ir_green_batches == n0 + (mode == 2)
        for c in range(4):
            e = max(_scaled(got[i][:, c], want[c][i]) for i in range(3))
            note("E6 radiate_ir_batch, ir_green = %d" % mode, e, row, TOL_IR_BATCH)
            assert e <= TOL_IR_BATCH, (mode, c, e)
    r.ir_green = 1
    assert r.fused_fallbacks == 0


def test_stored_opacities_cover_the_shard_asked_for(states):
    """Row h65, no communicator.  One shard's opacity pass, then the other shard: the stored block holds none of the bins
    an IR-only call would now work on, and the call refuses (it returned rows of bins nobody computed).  The legitimate
    order stays: an unsharded pass covers every bin, so a shard taken afterwards runs its IR-only step, and its per-bin
    fup_a on the shard's own bins is the unsharded handle's IR-only call's, bit for bit: measured so on an MI355X (the
    planner picks the same stand-alone half-wave form for the shard's IR bins as for all five), and asserted."""
    from clima_amd.radtran import ClimaException
    row = LF.BY_NAME["h65"]
    s, col = states(row), row.column()
    warm = type(col)(col, T=np.asarray(col["T"]) + 2.0)
    a = s.handle()
    a.set_bin_shard(0, 2)
    a.radiate(*col.args())
    a.set_bin_shard(1, 2)
    with pytest.raises(ClimaException, match="needs opacities"):
        a.radiate(*warm.args(), compute_opacity=False)
    shard, whole = s.handle(), s.handle()
    for h in (shard, whole):
        h.radiate(*col.args())
    shard.set_bin_shard(0, 2)
    ir_lo, ir_n = shard.bin_shard()[2:4]
    assert 0 < ir_n < row.bins()[0]
    for h in (shard, whole):
        h.radiate(*warm.args(), compute_solar=False, compute_opacity=False)
    got, want = (np.array(h.wrk_ir.fup_a)[:, ir_lo:ir_lo + ir_n] for h in (shard, whole))
    print("h65      IR-only fup_a of shard (0, 2) against the unsharded call: %.2e  [%.0e]" % (_scaled(got, want), TOL_LEVEL))
    np.testing.assert_array_equal(got, want)
    assert shard.fused_fallbacks == 0 and whole.fused_fallbacks == 0


# ------------------------------------------------------------------ E7
@rows
def test_e7_jacobians(states, row):
    from clima_amd.atmosphere import rce_jacobian_map
    from clima_amd.radtran import ClimaException
    from test_gpu_ir_jacobian_reduced import loop_reduce
    s = states(row)
    r, col, nz = s.handle("single0", coop0=True), row.column(), row.nz
    r.radiate(*col.args())
    if row.doubled:
        group, out_rows, _ = rce_jacobian_map((nz - 2) // 2, np.arange((nz - 2) // 2) % 5 == 1)
    else:
        group, out_rows = np.arange(nz + 1) // 2 + 1, None
    if nz < 4 or nz > 512:
        with pytest.raises(ClimaException, match=JACOBIAN_REFUSAL % nz):
            r.ir_jacobian(col["T_surface"], col["T"])
        with pytest.raises(ClimaException, match=r"the response form takes 4 <= nz <= 512 \(nz = %d\)" % nz):
            r.ir_jacobian_reduced(col["T_surface"], col["T"], group, out_rows)
        return
    got = r.ir_jacobian(col["T_surface"], col["T"])
    parts = r.ir_jacobian_reduced(col["T_surface"], col["T"], group, out_rows, parts=True)
    for a, b in zip(parts, loop_reduce(got, group, np.arange(1, nz + 2) if out_rows is None else out_rows)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(r.ir_jacobian_reduced(col["T_surface"], col["T"], group, out_rows), parts[2])
    assert r.fused_fallbacks == 0
    picks = [0, nz // 2 + 1, nz]
    args = (row.tables_cached(), r.opr(), col["T_surface"], col["T"], r.surface_emissivity, r.has_hard_surface, r.ir_tau_min)
    want = J.exact_jacobian(s.O, *args, zenith_weights=r.zenith_weights, cols=picks)
    other = J.exact_jacobian(OtherCompilation(s.O), *args, zenith_weights=r.zenith_weights, cols=picks)
    # of the largest |value| of the columns compared, every entry: test_gpu_ir_jacobian's own measure, on every row
    by_matrix = max(float(np.max(np.abs(a[:, picks] - b[:, picks]))) / float(np.max(np.abs(b[:, picks]))) for a, b in zip(got, want))
    note("E7 ir_jacobian, of the largest entry", by_matrix, row, TOL_JACOBIAN)
    assert by_matrix <= TOL_JACOBIAN
    missed = []
    for j in picks:
        e = max(J.column_scaled_error(a, b, j) for a, b in zip(got, want))
        yard = max(J.column_scaled_error(a, b, j) for a, b in zip(other, want))
        bound = max(TOL_JACOBIAN, 10.0 * yard) if row.name in CONDITIONED else TOL_JACOBIAN
        what = "0" if j == 0 else "nz/2+1" if j < nz else "nz"
        print("%-8s E7 column %-7s error %.2e  yardstick %.2e  bound %.2e" % (row.name, what, e, yard, bound))
        note("E7 ir_jacobian, column %s" % what, e, row, bound)
        if e > bound:
            missed.append((what, e, yard, bound))
    assert not missed, missed


def test_worst_figures():
    """prints what the module docstring records"""
    for figure in sorted(WORST):
        value, name, bound = WORST[figure]
        print("%-36s %.1e  [%.0e]  at %s" % (figure, value, bound, name))
        assert value <= bound
