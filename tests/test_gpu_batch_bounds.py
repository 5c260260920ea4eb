"""Column batches with per-column surface albedo, surface emissivity, zenith angles and photon scale factor
(radtran_toa_fluxes_batch_bounds and its device-array form; `bounds=` of Radtran.TOA_fluxes_batch and
TOA_fluxes_batch_tensors) on every row of the launch-form table (tests/launch_forms.py: 8 bins, chunks of 2).

Per row 5 columns (`row.columns(5)`) under five different bounds (`bounds_for`): the per-bin albedo and emissivity ramps
of `Row.surface()` scaled differently per column, one column with albedo 0 everywhere, one with albedo 1 and emissivity
1; the handle's zenith cosines and weights scaled differently per column (the cosines by factors whose products have no
exact reciprocal); a different photon scale factor per column.

B1  batches of 5, 1 and 4 columns against each column's own call after the five setters      bitwise; state; fields
B2  all five arrays NULL, every column given the handle's values, one array at a time         bytewise
B3  TOA_fluxes_batch_tensors(bounds=..., sync=False); the two builders of the blocks          bytewise the host form
B4  columns 0 and 4 against the oracle with its four setters                                  RTOL_TOA, TOL_LEVEL
B5  a pure-absorption case against the closed forms, column by column and bin by bin          TOL_BIN
B6  the repeat after an expired hand-off wait (fused_spins = 0) runs under the same bounds    bitwise the unfused batch
B7  refusals

The own call's form follows E3 of test_gpu_entry_points.py: coop_items = 0 on the rows that take one launch per
chunk, a batch of the column alone on the rows of exact pairs."""
import ctypes as C
import types
from fractions import Fraction

import numpy as np
import pytest

import closed_forms as CF
import launch_forms as LF
from test_gpu_batch_device import tensors
from test_gpu_batch_spectra import NAMES
from test_gpu_closed_forms import TOL_BIN
from test_gpu_entry_points import ROW_NAMES, RowState, assert_batch_is_own_calls, assert_state_is, left_state, level_errors
from test_gpu_parity import RTOL_TOA, TOL_LEVEL

pytestmark = pytest.mark.gpu

NCOL = 5
FIELDS = ("surface_albedo", "surface_emissivity", "zenith_u", "zenith_weights", "photon_scale_factor")
U_FACTORS = (1.0, 0.9, 0.77, 0.61, 1.0 / 3.0)        # of the handle's cosines (all in (0, 1])
W_FACTORS = (1.0, 0.5, 1.25, 0.3, 0.7)               # of the handle's weights
SCALES = (1.0, 0.4286, 2.5, 0.1, 1.7)


def ramps(row):
    """the per-bin ramps of Row.surface(), whether the row's own handle has them or not"""
    return LF.Row.surface(types.SimpleNamespace(per_bin_surface=True, bins=row.bins))


def bounds_for(row, r):
    """the five arrays, (NCOL, ...) each, for a handle `r` of the row"""
    al, em = ramps(row)
    u, w = np.asarray(r.zenith_u, dtype=float), np.asarray(r.zenith_weights, dtype=float)
    albedo = np.stack([0.0 * al, np.ones_like(al), 0.5 * al, 1.1 * al, 0.25 * al])
    emissivity = np.stack([em, np.ones_like(em), 0.9 * em, 0.8 * em, 0.95 * em])
    assert albedo.max() <= 1.0 and emissivity.max() <= 1.0
    b = dict(surface_albedo=albedo, surface_emissivity=emissivity, zenith_u=np.stack([f * u for f in U_FACTORS]),
             zenith_weights=np.stack([f * w for f in W_FACTORS]), photon_scale_factor=np.array(SCALES))
    return {k: np.ascontiguousarray(v) for k, v in b.items()}


def first(bounds, n):
    return {k: v[:n] for k, v in bounds.items()}


def fields_of(r):
    return {k: np.array(getattr(r, k), dtype=float, copy=True) for k in FIELDS}


def set_fields(h, values, oracle=False):
    """the five setters (`values`: name -> one column's value; any subset)"""
    if not oracle:
        for k, v in values.items():
            setattr(h, k, float(v) if k == "photon_scale_factor" else v)
        return
    if "surface_albedo" in values:
        h.set_surface_albedo(values["surface_albedo"])
    if "surface_emissivity" in values:
        h.set_surface_emissivity(values["surface_emissivity"])
    if "zenith_u" in values:
        h.set_zenith(values["zenith_u"], values["zenith_weights"])
    if "photon_scale_factor" in values:
        h.set_scalars(photon_scale_factor=float(values["photon_scale_factor"]))


class BoundsState(RowState):
    """RowState with the bounds, the bounds batch and the own calls under the setters"""

    def bounds(self):
        if "bounds" not in self.kept:
            self.kept["bounds"] = bounds_for(self.row, self.handle("bnd"))
        return self.kept["bounds"]

    def own_call(self, one, col):
        """a column's own call in the chunk's form (E3's rule for the rows of exact pairs): ((ISR, OLR), state)"""
        if self.row.doubled:
            isr, olr = one.TOA_fluxes_batch([col])
            toa = (isr[0], olr[0])
        else:
            toa = one.TOA_fluxes(*col.args())
        return toa, left_state(one)

    def own_under(self, names):
        """every column's own call on a second handle that had the setters `names` applied with that column's values;
        the handle's fields are put back afterwards"""
        key = ("own",) + tuple(names)
        if key not in self.kept:
            one = self.handle("own", coop0=self.row.one_launch)
            keep, b, out = fields_of(one), self.bounds(), []
            for c, col in enumerate(self.columns()):
                set_fields(one, {k: b[k][c] for k in names})
                out.append(self.own_call(one, col))
            set_fields(one, keep)
            self.kept[key] = out
        return self.kept[key]

    def bounds_batch(self):
        """(handle, the plain call's state before, its fields before, results of the 5-column bounds batch, the state it left)"""
        if "bounds_batch" not in self.kept:
            r = self.handle("bnd")
            r.TOA_fluxes(*self.row.column().args())
            before, fields = left_state(r), fields_of(r)
            got = r.TOA_fluxes_batch(self.columns(), return_fluxes=True, spectra_levels=self.levels(), bounds=self.bounds())
            self.kept["bounds_batch"] = (r, before, fields, got, left_state(r))
        return self.kept["bounds_batch"]


@pytest.fixture(scope="module")
def states(O):
    kept = {}

    def get(row):
        if row.name not in kept:
            kept[row.name] = BoundsState(row, O)
        return kept[row.name]
    return get


rows = pytest.mark.parametrize("row", LF.ROWS, ids=repr)


def assert_same_results(got, want, what):
    for g, w, name in zip(got[:3], want[:3], ("ISR", "OLR", "fluxes")):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, name)
    if len(want) > 3:
        assert sorted(got[3]) == sorted(want[3])
        for name in want[3]:
            assert np.ascontiguousarray(got[3][name]).tobytes() == np.ascontiguousarray(want[3][name]).tobytes(), (what, name)


# ------------------------------------------------------------------ B1
@rows
def test_b1_own_calls(states, row):
    s = states(row)
    cols, b, own = s.columns(), s.bounds(), s.own_under(FIELDS)
    r, before, fields, got, state = s.bounds_batch()
    assert got[2].shape == (row.nz + 1, 5, NCOL)
    assert_batch_is_own_calls(got, own, s.levels(), "5 columns")
    for k in own[-1][1]:
        np.testing.assert_array_equal(state[k], own[-1][1][k], err_msg="the state after 5 columns: " + k)
    for n in (1, 4):      # (4: two full chunks, the second one's first column is the batch's column 2)
        got_n = r.TOA_fluxes_batch(cols[:n], return_fluxes=True, spectra_levels=s.levels(), bounds=first(b, n))
        assert got_n[2].shape == (row.nz + 1, 5, n)
        assert_batch_is_own_calls(got_n, own[:n], s.levels(), "%d column(s)" % n)
        assert_state_is(r, own[n - 1][1], "the state after %d column(s)" % n)
    # the columns differ under their bounds: the own calls of two columns on the SAME atmosphere are not one answer
    one = s.handle("own", coop0=row.one_launch)
    keep = fields_of(one)
    set_fields(one, {k: b[k][1] for k in FIELDS})
    other = s.own_call(one, cols[0])
    set_fields(one, keep)
    assert other[0] != own[0][0]
    # the handle's own fields are what they were, and a plain call runs under them
    for k, v in fields_of(r).items():
        np.testing.assert_array_equal(v, fields[k], err_msg=k)
    r.TOA_fluxes(*row.column().args())
    after = left_state(r)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg="the plain call after the bounds batch: " + k)
    assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ B2
@rows
def test_b2_null_is_the_handle(states, row):
    s = states(row)
    cols, b = s.columns(), s.bounds()
    r = s.handle("null")
    want = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=s.levels())
    want_state = left_state(r)
    plain = r.TOA_fluxes_batch(cols, return_fluxes=True)
    fields = fields_of(r)
    tiled = {k: np.ascontiguousarray(np.broadcast_to(v, (NCOL,) + np.shape(v))) for k, v in fields.items()}
    for what, bounds in (("all five NULL", {}), ("the handle's own values", tiled)):
        got = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=s.levels(), bounds=bounds)
        assert_same_results(got, want, what)
        state = left_state(r)
        for k in want_state:
            np.testing.assert_array_equal(state[k], want_state[k], err_msg="%s: the state: %s" % (what, k))
        assert_same_results(r.TOA_fluxes_batch(cols, return_fluxes=True, bounds=bounds), plain, what + ", no spectra")
    # one array at a time (the zenith cosines and weights, as on the oracle, are two arrays: each alone)
    for name in FIELDS:
        own = s.own_under((name,))
        isr, olr, fl = r.TOA_fluxes_batch(cols, return_fluxes=True, bounds={name: b[name]})
        for c, (toa, st) in enumerate(own):
            assert (isr[c], olr[c]) == toa, (name, c)
            for k, rn in enumerate(ROW_NAMES):
                np.testing.assert_array_equal(fl[:, k, c], st[rn], err_msg="%s alone: column %d %s" % (name, c, rn))
    assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ B3
def pack_both(r, bounds, n):
    """(device-built blocks, host-built blocks, block_count) of the two test hooks; bounds: name -> array or absent"""
    dp = C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(bounds[k][:n]) if k in bounds else None for k in FIELDS]
    args = [a.ctypes.data_as(dp) if a is not None else None for a in arrs]
    cc = C.c_int()
    r._L.clima_test_pack_bounds(r._ptr, C.byref(C.c_int(n)), *args, None, C.byref(cc), r._err)
    r._check()
    out = []
    for fn in (r._L.clima_test_pack_bounds, r._L.clima_test_pack_bounds_host):
        blocks = np.full(n * cc.value, np.nan)
        fn(r._ptr, C.byref(C.c_int(n)), *args, blocks.ctypes.data_as(dp), C.byref(cc), r._err)
        r._check()
        out.append(blocks)
    return out[0], out[1], cc.value


@rows
def test_b3_device_form(states, row):
    import torch
    s = states(row)
    cols, b = s.columns(), s.bounds()
    r, _, _, want, want_state = s.bounds_batch()
    r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=s.levels(), bounds=b)     # (B1 may have left a shorter batch's state)
    bt = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    isr, olr, fl, spec = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, sync=False, spectra_levels=s.levels(), bounds=bt)
    r.synchronize()
    got = (isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0)),
           {k: np.transpose(v.cpu().numpy(), (1, 2, 0)) for k, v in spec.items()})
    assert sorted(got[3]) == sorted(NAMES)
    assert_same_results(got, want, "the device form")
    assert_state_is(r, want_state, "the state after the device form")
    # without spectra (nsel = 0), two arrays given and three NULL
    some = {k: b[k] for k in ("zenith_u", "photon_scale_factor")}
    want2 = r.TOA_fluxes_batch(cols, return_fluxes=True, bounds=some)
    isr, olr, fl = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, sync=False, bounds={k: bt[k] for k in some})
    r.synchronize()
    assert_same_results((isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0))), want2, "two arrays, no spectra")
    # the blocks themselves: both builders, every array given and some NULL
    n_ir, n_sol, _ = row.bins()
    for bounds in (b, some, {}):
        dev, host, cc = pack_both(r, bounds, NCOL)
        assert cc == n_sol + n_ir + 3 * row.nzen + 1
        assert not np.isnan(host).any()
        assert dev.tobytes() == host.tobytes()
    # ... of which the reciprocals: correctly rounded quotients, inexact ones among them
    host = pack_both(r, b, NCOL)[1].reshape(NCOL, -1)
    u, iu = host[:, n_sol + n_ir:n_sol + n_ir + row.nzen], host[:, n_sol + n_ir + 2 * row.nzen:n_sol + n_ir + 3 * row.nzen]
    np.testing.assert_array_equal(u, b["zenith_u"])
    np.testing.assert_array_equal(iu, 1.0 / b["zenith_u"])
    inexact = [Fraction(float(a)) * Fraction(float(x)) != 1 for a, x in zip(iu.ravel(), u.ravel())]      # (exact rationals)
    assert any(inexact)
    assert r.fused_fallbacks == 0


# ------------------------------------------------------------------ B4
@rows
def test_b4_against_the_oracle(states, row):
    s = states(row)
    _, _, _, (isr, olr, fl, _), _ = s.bounds_batch()
    o, b = s.oracle(), s.bounds()
    for c in (0, NCOL - 1):
        set_fields(o, {k: b[k][c] for k in FIELDS}, oracle=True)
        isr_o, olr_o = o.TOA_fluxes(*s.columns()[c].args())
        e_toa = max(abs(olr[c] - olr_o) / abs(olr_o), abs(isr[c] - isr_o) / max(abs(isr_o), 1e-300))
        e_lv = level_errors({name: fl[:, k, c] for k, name in enumerate(ROW_NAMES)}, o)
        print("%-8s column %d: OLR, ISR (relative) %.2e [%.0e]   level rows %.2e [%.0e]" % (row.name, c, e_toa, RTOL_TOA, e_lv, TOL_LEVEL))
        assert e_toa <= RTOL_TOA and e_lv <= TOL_LEVEL, (c, e_toa, e_lv)


# ------------------------------------------------------------------ B5
def test_b5_against_the_closed_forms(hip_lib):
    """The pure-absorption case nz12 (3 zenith angles, hard surface) as a bounds batch: five times the case's column,
    each under its own albedo, emissivity, zenith angles and scale; every column's per-bin spectra at every level against
    closed_forms.solar_channel / ir_channel with that column's values."""
    from clima_amd.radtran import Radtran
    case = CF.absorption_case("nz12")
    tables, nz, sc = case["tables"], case["nz"], case["scalars"]
    r = Radtran(tables, nz, case["nzen"], 0.3)
    for k, v in sc.items():
        setattr(r, k, v)
    r.surface_albedo, r.surface_emissivity = case["albedo"], case["emissivity"]
    al, em = case["albedo"], case["emissivity"]
    u, w = np.asarray(r.zenith_u, dtype=float), np.asarray(r.zenith_weights, dtype=float)
    b = dict(surface_albedo=np.stack([0.0 * al, np.ones_like(al), 0.5 * al, 1.1 * al, 0.25 * al]),
             surface_emissivity=np.stack([em, np.ones_like(em), 0.9 * em, 0.8 * em, 0.95 * em]),
             zenith_u=np.stack([f * u for f in U_FACTORS]), zenith_weights=np.stack([f * w for f in W_FACTORS]),
             photon_scale_factor=np.array(SCALES))
    cols = [case["column"]] * NCOL
    isr, olr, fl, spec = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=list(range(nz + 1)), bounds=b)
    tau, w0 = r.opr()[:2]            # (64 layers at most: one call per column, the handle's block is the last column's)
    assert np.all(w0 == 0.0)
    trans = CF.ir_transmissions(tables, tau)
    col = case["column"]
    for c in range(NCOL):
        ir = CF.ir_channel(tables, tau, col["T_surface"], col["T"], b["surface_emissivity"][c], sc["has_hard_surface"], sc["ir_tau_min"], trans)
        sol = CF.solar_channel(tables, tau, b["zenith_u"][c], b["zenith_weights"][c], b["surface_albedo"][c], sc["diurnal_fac"],
                               b["photon_scale_factor"][c])
        e_ir = CF.per_bin(spec["ir_fup_a"][:, :, c], spec["ir_fdn_a"][:, :, c], ir.fup_a, ir.fdn_a)
        e_sol = CF.per_bin(spec["sol_fup_a"][:, :, c], spec["sol_fdn_a"][:, :, c], sol.fup_a, sol.fdn_a)
        print("column %d: IR per bin worst %.2e, solar per bin worst %.2e  [%.0e]" % (c, e_ir.max(), e_sol.max(), TOL_BIN))
        assert np.all(e_ir <= TOL_BIN) and np.all(e_sol <= TOL_BIN), (c, e_ir, e_sol)
        if c == 0:
            assert np.all(spec["sol_fup_a"][:, :, c] == 0.0)      # albedo 0, no scattering: nothing comes back up


# ------------------------------------------------------------------ B6
def test_b6_the_repeat_runs_under_the_same_bounds(states):
    """Row h100 (one launch per chunk) with fused_spins = 0: every two-stream item's wait expires, the batch is computed
    again through the separate launches (fused_fallbacks + 1) -- under the same bounds, which stayed in their arena:
    bitwise the batch of a handle that runs unfused (the pattern of test_gpu_batch_device.py's repeat test)."""
    import torch
    row = LF.BY_NAME["h100"]
    s = states(row)
    cols, b = s.columns(), s.bounds()
    ref = s.handle()
    ref.fused = False
    want = ref.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=s.levels(), bounds=b)
    assert ref.fused_fallbacks == 0
    plain = ref.TOA_fluxes_batch(cols, return_fluxes=True)
    assert not np.array_equal(plain[0], want[0])                  # (the bounds are not the handle's fields)
    r = s.handle()
    r.fused_spins = 0
    n0 = r.fused_fallbacks
    got = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=s.levels(), bounds=b)
    assert r.fused_fallbacks == n0 + 1
    assert_same_results(got, want, "the repeated host batch")
    bt = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    isr, olr, fl, spec = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, sync=False, spectra_levels=s.levels(), bounds=bt)
    assert r.fused_fallbacks == n0 + 1                            # nothing has been looked at yet
    r.synchronize()
    assert r.fused_fallbacks == n0 + 2
    got = (isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0)),
           {k: np.transpose(v.cpu().numpy(), (1, 2, 0)) for k, v in spec.items()})
    assert_same_results(got, want, "the repeated device batch")


# ------------------------------------------------------------------ B7
def test_b7_refusals(states):
    import torch
    from clima_amd.radtran import ClimaException
    from test_gpu_batch_device import stacked
    row = LF.BY_NAME["h65"]
    s = states(row)
    cols, b = s.columns(), s.bounds()
    r = s.handle()
    n, nz = NCOL, row.nz
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    a = stacked(cols, r.np)

    def d(x):
        return x.ctypes.data_as(dp) if x is not None else None

    isr, olr = np.empty(n), np.empty(n)
    head = (r._ptr, C.byref(C.c_int(n)), d(a["T_surface"]), d(a["T"]), d(a["P"]), d(a["densities"]), d(a["dz"]),
            C.byref(C.c_int(1 if r.np > 0 else 0)), d(a.get("pdensities")), d(a.get("radii")), d(isr), d(olr), None)
    five = tuple(d(b[k]) for k in FIELDS)
    # nsel = 0 with the spectrum arrays NULL passes, and is the Python call without spectra
    r._L.radtran_toa_fluxes_batch_bounds(*head, *five, C.byref(C.c_int(0)), None, None, None, None, None, r._err)
    r._check()
    want = r.TOA_fluxes_batch(cols, bounds=b)
    assert isr.tobytes() == want[0].tobytes() and olr.tobytes() == want[1].tobytes()
    # nsel = 1 with all four NULL: the spectra batch's text
    lv = np.array([nz + 1], dtype=np.int32)
    r._L.radtran_toa_fluxes_batch_bounds(*head, *five, C.byref(C.c_int(1)), lv.ctypes.data_as(ip), None, None, None, None, r._err)
    with pytest.raises(ClimaException, match="^toa_fluxes_batch_spectra: none of ir_fup, ir_fdn, sol_fup, sol_fdn was given"):
        r._check()
    # ... and what the plain batch refuses, with its text
    r._L.radtran_toa_fluxes_batch_bounds(r._ptr, C.byref(C.c_int(0)), *head[2:], *five, C.byref(C.c_int(0)), None, None, None, None, None, r._err)
    with pytest.raises(ClimaException, match='^"T" has the wrong input dimension.$'):
        r._check()
    # the device form: a bounds array on the host is refused by name, with nothing enqueued
    t = tensors(cols, r.np)
    bt = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    d_isr, d_olr = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev_head = (r._ptr, C.byref(C.c_int(n)), t["T_surface"].data_ptr(), t["T"].data_ptr(), t["P"].data_ptr(), t["densities"].data_ptr(),
                t["dz"].data_ptr(), C.byref(C.c_int(1 if r.np > 0 else 0)), t["pdensities"].data_ptr() if r.np > 0 else None,
                t["radii"].data_ptr() if r.np > 0 else None, d_isr.data_ptr(), d_olr.data_ptr(), None)
    r.synchronize()
    r.profile(True)              # events around every kernel: kernel_time counts what is enqueued from here on
    r.profile_reset()
    for k in FIELDS:
        given = [b[x].ctypes.data if x == k else bt[x].data_ptr() for x in FIELDS]
        r._L.radtran_toa_fluxes_batch_bounds_device(*dev_head, *given, C.byref(C.c_int(0)), None, None, None, None, None, None, r._err)
        with pytest.raises(ClimaException, match='^toa_fluxes_batch_device: "%s" is not device memory of this handle\'s device' % k):
            r._check()
    r.synchronize()
    assert [r.kernel_time(k)[1] for k in range(4)] == [0, 0, 0, 0]        # nothing was enqueued
    r.TOA_fluxes_batch_tensors(**t, bounds=bt)
    assert r.kernel_time(1)[1] > 0                                         # (a batch that runs is counted)
    r.profile(False)
    # the Python checks come first: an unknown key and a wrong shape, by name
    with pytest.raises(ClimaException, match='"albedo" is not one of'):
        r.TOA_fluxes_batch(cols, bounds={"albedo": b["surface_albedo"]})
    with pytest.raises(ClimaException, match='"zenith_u" has the shape'):
        r.TOA_fluxes_batch_tensors(**t, bounds={"zenith_u": bt["zenith_u"][:, :1].contiguous()})
    # afterwards the handle computes what it did
    again = r.TOA_fluxes_batch(cols, bounds=b)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()
