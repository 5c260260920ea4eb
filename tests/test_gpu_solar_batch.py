"""radtran_radiate_solar_batch: many illumination cases (zenith angles and weights, surface albedo, photon scale factor)
on the stored optical properties, and its kernel k_twostream_sol_batch (clima_amd/csrc/solar_batch.inc) through the
hook clima_test_solar_batch.

G1  every golden column as one case of a 9-case batch: that case against the reference's own two_stream_solar
    (tests/golden), the other eight against oracle.two_stream_solar; default form and the 4-wave form; 8, 1, 12 g-points
G2  3 and 16 angles per case: sum_z w_z x (oracle at u_z) in long double, one weight exactly 0
G3  the entry point on rows of the launch-form table: against own calls after the setters, the oracle, a handle with
    one angle; the per-case form forced; the shared form's counter
G4  a case's bytes do not depend on the batch around it
G5  the handle's state and fields are untouched
G6  a pure-absorption case against the closed forms, bin by bin
G7  refusals

The rule of G1 / G2 is tests/test_gpu_golden.py::_check: TOL = 2e-10 of the channel's largest flux (up and down together;
amean on its own), or 10 x the difference of the reference algorithm's two compilations (FMA contraction on / off) on
the same inputs where that is larger.

G7 holds every refusal text but one.  f_total on a handle without level rows is refused on what Holds records (`rows`,
set by every call that leaves level rows, cleared by a graph replay), and Holds gives opacities only to a handle that
ran such a call and takes them away with the rows: no sequence of entry points reaches the text.  What can be held is
the other side: test_f_total_after_a_profile_reset."""
import ctypes as C

import numpy as np
import pytest

import closed_forms as CF
import launch_forms as LF
from test_gpu_batch_bounds import FIELDS, bounds_for, fields_of, set_fields
from test_gpu_closed_forms import TOL_BIN
from test_gpu_entry_points import RowState, configure, left_state
from test_gpu_golden import TOL, _load_gold, _yardstick
from test_gpu_parity import RTOL_TOA, TOL_LEVEL, TOL_SPEC, _scaled

pytestmark = pytest.mark.gpu

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
U1 = 1.0 / np.sqrt(3.0)
DRAW_U = (0.02, 0.3, U1, 0.9, 1.0)
DRAW_R = (0.0, 0.15, 1.0)
NCASE = 9
WBIN8 = np.array([0.0625, 0.125, 0.1875, 0.125, 0.0625, 0.25, 0.125, 0.0625])      # test_gpu_golden._run's


def _i(v):
    return C.byref(C.c_int(int(v)))


def _p(a):
    return a.ctypes.data_as(DP)


def weights(ng):
    return WBIN8 if ng == 8 else np.full(ng, 1.0 / ng) if ng > 1 else np.ones(1)


def run_hook(L, tau, w0, g, ng, force_nw, zen_u, zen_w, rsfc):
    """clima_test_solar_batch: zen_u, zen_w (ncol, nzen), rsfc (ncol) -> fup, fdn, amean (ncol, nz+1) TOA-first"""
    tau, w0, g = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g))
    zen_u, zen_w, rsfc = (np.ascontiguousarray(a, dtype=np.float64) for a in (zen_u, zen_w, rsfc))
    n, nzen = zen_u.shape
    nz = len(tau)
    out = [np.full((n, nz + 1), np.nan) for _ in range(3)]
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_solar_batch(_i(nz), _i(ng), _i(force_nw), _p(tau), _p(w0), _p(g), _p(wb), _i(n), _i(nzen), _p(zen_u), _p(zen_w),
                             _p(rsfc), *[_p(o) for o in out], err)
    assert err.value == b"", err.value
    return out


def hold(got, ref, yard, tag):
    """got, ref: (fup, fdn, amean); yard: (flux yardstick, amean yardstick), absolute"""
    scale = max(np.max(np.abs(ref[0])), np.max(np.abs(ref[1])))
    tol = max(TOL * scale, 10.0 * yard[0])
    e = max(np.max(np.abs(got[0] - ref[0])), np.max(np.abs(got[1] - ref[1])))
    assert e <= tol, (tag, "fluxes", e, tol)
    tol = max(TOL * np.max(np.abs(ref[2])), 10.0 * yard[1])
    e = np.max(np.abs(got[2] - ref[2]))
    assert e <= tol, (tag, "amean", e, tol)


def oracle_solar(O, tau, w0, g, u0, rs):
    """((fup, fdn, amean), (flux yardstick, amean yardstick)) of the oracle's two compilations"""
    a = O.two_stream_solar(tau, w0, g, u0, rs)
    b = O.two_stream_solar(tau, w0, g, u0, rs, variant="fma")
    ref = (a[2], a[3], a[0])
    assert all(np.all(np.isfinite(x)) for x in ref), (u0, rs)
    return ref, (max(np.max(np.abs(b[2] - a[2])), np.max(np.abs(b[3] - a[3]))), np.max(np.abs(b[0] - a[0])))


@pytest.fixture(scope="module")
def gold():
    return _load_gold()


@pytest.fixture(scope="module")
def g1_cases(gold, O):
    """per golden column: (key, j, zen_u (9, 1), rsfc (9), references and yardsticks of the nine cases), computed once"""
    out = []
    rng = np.random.default_rng(20261)
    pairs = [(u, r) for u in DRAW_U for r in DRAW_R]
    for n in range(int(gold["ncases"][0])):
        k = "c%02d_" % n
        tau, w0, g = gold[k + "tau"], gold[k + "w0"], gold[k + "g"]
        j = (0, 4, 8)[n % 3]
        u0, rs = (float(x) for x in gold[k + "sol_par"])
        zu, rsfc, refs = np.empty((NCASE, 1)), np.empty(NCASE), []
        for c in range(NCASE):
            if c == j:
                zu[c, 0], rsfc[c] = u0, rs
                y = _yardstick(gold, k)
                refs.append(((gold[k + "sol_fup"], gold[k + "sol_fdn"], gold[k + "sol_amean"]), (y[1], y[2])))
                continue
            while True:
                u, r = pairs[rng.integers(len(pairs))]
                if not (u == U1 and np.any(np.asarray(w0) == 0.0)):      # the reference divides 0 by 0 there: another pair
                    break
            zu[c, 0], rsfc[c] = u, r
            refs.append(oracle_solar(O, tau, w0, g, u, r))
        out.append((k, j, zu, rsfc, refs))
    return out


# ------------------------------------------------------------------ G1
@pytest.mark.parametrize("ng,force_nw", [(8, 0), (1, 0), (12, 0), (8, 4), (12, 4), (1, 4)])
def test_g1_golden_columns(hip_lib, gold, g1_cases, ng, force_nw):
    ran, want = 0, 0
    seen_u1 = False
    for k, j, zu, rsfc, refs in g1_cases:
        tau = gold[k + "tau"]
        assert len(tau) <= 512
        if force_nw == 4 and len(tau) > 256:
            continue
        want += 1
        got = run_hook(hip_lib, tau, gold[k + "w0"], gold[k + "g"], ng, force_nw, zu, np.ones_like(zu), rsfc)
        for c in range(NCASE):
            hold([o[c] for o in got], refs[c][0], refs[c][1], (k, "case %d" % c, "golden" if c == j else "oracle", ng, force_nw))
            seen_u1 = seen_u1 or zu[c, 0] == U1
        ran += 1
    assert ran == want and (force_nw == 4 or ran == int(gold["ncases"][0])) and ran >= 30
    assert seen_u1                                  # u0 = 1/sqrt(3) met zero-thickness slots and real layers


# ------------------------------------------------------------------ G2
@pytest.mark.parametrize("nzen", [3, 16])
def test_g2_several_angles_per_case(hip_lib, gold, O, nzen):
    LD = np.longdouble
    rng = np.random.default_rng(77 + nzen)
    for n in range(36, 68):
        k = "c%02d_" % n
        tau, w0, g = gold[k + "tau"], gold[k + "w0"], gold[k + "g"]
        ncase = 3
        zu = rng.uniform(0.05, 1.0, (ncase, nzen))
        zw = rng.uniform(0.0, 1.0, (ncase, nzen))
        zw[1, nzen // 2] = 0.0                       # a weight of exactly 0
        rsfc = np.array([0.0, 1.0, 0.3])
        got = run_hook(hip_lib, tau, w0, g, 8, 0, zu, zw, rsfc)
        for c in range(ncase):
            ref, yard = [np.zeros(len(tau) + 1, dtype=LD) for _ in range(3)], [LD(0), LD(0)]
            for z in range(nzen):
                rz, yz = oracle_solar(O, tau, w0, g, zu[c, z], rsfc[c])
                for a in range(3):
                    ref[a] += LD(zw[c, z]) * rz[a].astype(LD)
                yard = [yard[0] + LD(zw[c, z]) * yz[0], yard[1] + LD(zw[c, z]) * yz[1]]
            hold([o[c] for o in got], [np.asarray(r, dtype=np.float64) for r in ref], [float(y) for y in yard], (k, c, nzen))


# ------------------------------------------------------------------ G3
G3_ROWS = ("nz1", "nz2", "s64", "h65", "h130", "w257", "w512", "b513", "p402", "c130", "g4-70", "g16-100")
SOL_FIELDS = tuple(f for f in FIELDS if f != "surface_emissivity")


@pytest.fixture(scope="module")
def states(O):
    kept = {}

    def get(row):
        if row.name not in kept:
            kept[row.name] = RowState(row, O)
        return kept[row.name]
    return get


def batch_of(r, b, levels, **kw):
    return r.radiate_solar_batch(b["zenith_u"], b["zenith_weights"], b["surface_albedo"], b["photon_scale_factor"],
                                 spectra_levels=levels, **kw)


def hold_case(got, c, w, levels, what):
    """case c of a batch's results against the state `w` (left_state) of a solar call"""
    fup, fdn, ft, spec = got
    n_scale = max(np.max(np.abs(w["sol_fup_n"])), np.max(np.abs(w["sol_fdn_n"])), 1e-300)
    e_lv = max(np.max(np.abs(fup[:, c] - w["sol_fup_n"])), np.max(np.abs(fdn[:, c] - w["sol_fdn_n"]))) / n_scale
    a_scale = max(np.max(np.abs(w["sol_fup_a"])), np.max(np.abs(w["sol_fdn_a"])), 1e-300)
    e_sp = max(np.max(np.abs(spec["fup"][:, :, c] - w["sol_fup_a"][levels, :])), np.max(np.abs(spec["fdn"][:, :, c] - w["sol_fdn_a"][levels, :]))) / a_scale
    e_am = float(np.max(np.abs(spec["amean"][:, :, c] - w["sol_amean"][levels, :])) / max(float(np.max(np.abs(w["sol_amean"]))), 1e-300))
    print("%s case %d: level rows %.2e [%.0e]  spectra %.2e  amean %.2e [%.0e]" % (what, c, e_lv, TOL_LEVEL, e_sp, e_am, TOL_SPEC))
    assert e_lv <= TOL_LEVEL and e_sp <= TOL_SPEC and e_am <= TOL_SPEC, (what, c, e_lv, e_sp, e_am)


@pytest.mark.parametrize("name", G3_ROWS)
def test_g3_entry_point(states, name):
    row = LF.BY_NAME[name]
    s = states(row)
    col, levels = row.column(), s.levels()
    r = s.handle("solar")
    r.radiate(*col.args())
    ir_net = np.array(r.wrk_ir.fdn_n) - np.array(r.wrk_ir.fup_n)
    b = bounds_for(row, r)
    covered = row.nz <= 512
    n0 = r.solar_batch_shared()[1]
    got = batch_of(r, b, levels)
    assert r.solar_batch_shared() == (1, n0 + (1 if covered else 0))
    assert got[0].shape == got[1].shape == got[2].shape == (row.nz + 1, 5) and sorted(got[3]) == ["amean", "fdn", "fup"]
    r.solar_batch_shared(0)
    per_case = batch_of(r, b, levels)
    assert r.solar_batch_shared() == (0, n0 + (1 if covered else 0))          # the counter moves only with the shared form
    assert r.solar_batch_shared(1)[0] == 1
    # every case against its own call on a second handle after the setters
    one = s.handle("own")
    one.radiate(*col.args())
    keep = fields_of(one)
    own = []
    for c in range(5):
        set_fields(one, {k: b[k][c] for k in SOL_FIELDS})
        one.radiate(*col.args(), compute_solar=True, compute_opacity=False)
        own.append(left_state(one))
    set_fields(one, keep)
    for what, res in (("shared" if covered else "per case (nz > 512)", got), ("per case, forced", per_case)):
        for c in range(5):
            hold_case(res, c, own[c], levels, "%s %s" % (name, what))
            np.testing.assert_array_equal(res[2][:, c], (res[1][:, c] - res[0][:, c]) + ir_net, err_msg="f_total")
    assert not np.array_equal(got[0][:, 1], got[0][:, 2])
    # cases 0 and 4 against the oracle with its setters
    o = s.oracle()
    for c in (0, 4):
        set_fields(o, {k: b[k][c] for k in SOL_FIELDS}, oracle=True)
        o.radiate(*col.args())
        w = o.wrk_sol
        scale = max(float(np.max(np.abs(w.fup_n))), float(np.max(np.abs(w.fdn_n))), 1e-300)
        isr_o = w.fdn_n[-1] - w.fup_n[-1]
        for what, res in (("default", got), ("per case", per_case)):
            e_lv = max(np.max(np.abs(res[0][:, c] - w.fup_n)), np.max(np.abs(res[1][:, c] - w.fdn_n))) / scale
            e_toa = abs((res[1][-1, c] - res[0][-1, c]) - isr_o) / max(abs(isr_o), 1e-300)
            print("%s %s case %d against the oracle: ISR %.2e [%.0e]  level rows %.2e [%.0e]" % (name, what, c, e_toa, RTOL_TOA, e_lv, TOL_LEVEL))
            assert e_toa <= RTOL_TOA and e_lv <= TOL_LEVEL, (what, c, e_toa, e_lv)
            assert _scaled(res[3]["amean"][:, :, c], np.asarray(w.amean)[levels, :]) <= TOL_SPEC


def test_g3_one_angle_on_a_handle_with_three(states, O):
    """nzen = 1 in the batch on row h65 (3 angles in the handle): a second HIP handle and an oracle made with one angle"""
    from clima_amd.radtran import Radtran
    row = LF.BY_NAME["h65"]
    s = states(row)
    col, levels = row.column(), s.levels()
    r = s.handle("solar")
    assert len(r.zenith_u) == 3
    r.radiate(*col.args())
    us = np.array([0.9, U1, 0.2])
    al = np.stack([f * np.asarray(r.surface_albedo, dtype=float) for f in (1.0, 0.0, 0.5)])
    with row.environment():
        one = configure(row, Radtran(row.tables_cached(), row.nz, 1, 0.25))
        o = configure(row, O.OracleRadtran(row.tables_cached(), row.nz, 1, 0.25), oracle=True)
    one.radiate(*col.args())
    for shared in (1, 0):
        r.solar_batch_shared(shared)
        got = r.radiate_solar_batch(us, surface_albedo=al, spectra_levels=levels)
        for c in range(3):
            vals = dict(zenith_u=us[c:c + 1], zenith_weights=np.ones(1), surface_albedo=al[c])
            set_fields(one, vals)
            one.radiate(*col.args(), compute_solar=True, compute_opacity=False)
            hold_case(got, c, left_state(one), levels, "h65 one angle, shared=%d" % shared)
            set_fields(o, vals, oracle=True)
            o.radiate(*col.args())
            w = o.wrk_sol
            scale = max(float(np.max(np.abs(w.fup_n))), float(np.max(np.abs(w.fdn_n))))
            assert max(np.max(np.abs(got[0][:, c] - w.fup_n)), np.max(np.abs(got[1][:, c] - w.fdn_n))) <= TOL_LEVEL * scale
    r.solar_batch_shared(1)


# ------------------------------------------------------------------ G4
def cases_per_block(L, n):
    out = C.c_int()
    L.clima_test_solar_batch_cases_per_block(_i(n), C.byref(out))
    return out.value


@pytest.mark.parametrize("ng,n_col", [(8, 41), (12, 45), (8, 60)])
def test_g4_a_case_does_not_depend_on_its_batch(hip_lib, gold, ng, n_col):
    k = "c%02d_" % n_col
    tau, w0, g = gold[k + "tau"], gold[k + "w0"], gold[k + "g"]
    rng = np.random.default_rng(5)
    nzen = 2
    # enough cases for several blocks in z, by the launcher's own rule
    blocks = lambda n: (n + cases_per_block(hip_lib, n) - 1) // cases_per_block(hip_lib, n)   # noqa: E731
    many = next(n for n in range(NCASE + 1, 400) if blocks(n) >= 4 and cases_per_block(hip_lib, n) < NCASE)
    assert blocks(40) == 4 and blocks(NCASE) == 2 and many <= 40      # (a block's share of `many` ends inside the first nine cases)
    zu, zw, rs = rng.uniform(0.05, 1.0, (many, nzen)), rng.uniform(0.1, 1.0, (many, nzen)), rng.uniform(0.0, 1.0, many)
    rs[0], rs[1] = 0.0, 1.0
    nine = run_hook(hip_lib, tau, w0, g, ng, 0, zu[:NCASE], zw[:NCASE], rs[:NCASE])
    again = run_hook(hip_lib, tau, w0, g, ng, 0, zu[:NCASE], zw[:NCASE], rs[:NCASE])
    big = run_hook(hip_lib, tau, w0, g, ng, 0, zu, zw, rs)
    for a in range(3):
        assert nine[a].tobytes() == again[a].tobytes()
        assert big[a][:NCASE].tobytes() == nine[a].tobytes()
        assert np.all(np.isfinite(big[a]))
    for c in (0, 3, 8):
        alone = run_hook(hip_lib, tau, w0, g, ng, 0, zu[c:c + 1], zw[c:c + 1], rs[c:c + 1])
        pair = run_hook(hip_lib, tau, w0, g, ng, 0, zu[[5, c]], zw[[5, c]], rs[[5, c]])
        for a in range(3):
            assert alone[a][0].tobytes() == nine[a][c].tobytes(), (c, a)
            assert pair[a][1].tobytes() == nine[a][c].tobytes(), (c, a)


def test_g4_entry_point_batches(states):
    row = LF.BY_NAME["h130"]
    s = states(row)
    r = s.handle("solar")
    r.radiate(*row.column().args())
    rng = np.random.default_rng(6)
    n_sol = row.bins()[1]
    zu, zw = rng.uniform(0.05, 1.0, (40, row.nzen)), rng.uniform(0.1, 1.0, (40, row.nzen))
    al, sc = rng.uniform(0.0, 1.0, (40, n_sol)), rng.uniform(0.1, 2.0, 40)
    lv = s.levels()
    big = r.radiate_solar_batch(zu, zw, al, sc, spectra_levels=lv)
    nine = r.radiate_solar_batch(zu[:9], zw[:9], al[:9], sc[:9], spectra_levels=lv)
    last = r.radiate_solar_batch(zu[7:9], zw[7:9], al[7:9], sc[7:9], spectra_levels=lv)
    for a in range(3):
        assert np.ascontiguousarray(big[a][:, :9]).tobytes() == np.ascontiguousarray(nine[a]).tobytes()
        assert np.ascontiguousarray(last[a][:, 1]).tobytes() == np.ascontiguousarray(nine[a][:, 8]).tobytes()
    for name in nine[3]:
        assert np.ascontiguousarray(big[3][name][:, :, :9]).tobytes() == nine[3][name].tobytes()
        assert np.ascontiguousarray(last[3][name][:, :, 1]).tobytes() == np.ascontiguousarray(nine[3][name][:, :, 8]).tobytes()


# ------------------------------------------------------------------ G5
@pytest.mark.parametrize("name", ["h130", "b513"])
def test_g5_state_and_fields_are_untouched(states, name):
    row = LF.BY_NAME[name]
    s = states(row)
    col = row.column()
    r = s.handle("solar")
    r.radiate(*col.args())
    T = np.stack([np.asarray(col["T"], dtype=float) + d for d in (0.0, 1.5)], axis=1)
    Ts = np.array([col["T_surface"], col["T_surface"] + 2.0])
    if row.nz <= 512:
        ir_before = r.radiate_ir_batch(Ts, T)
    r.radiate(*col.args(), compute_opacity=False)
    before, fields = left_state(r), fields_of(r)
    b = bounds_for(row, r)
    for shared in (1, 0):
        r.solar_batch_shared(shared)
        batch_of(r, b, s.levels())
        after = left_state(r)
        for k in before:
            assert after[k].tobytes() == before[k].tobytes(), (shared, k)
        for k, v in fields_of(r).items():
            assert v.tobytes() == fields[k].tobytes(), (shared, k)
    r.solar_batch_shared(1)
    r.radiate(*col.args(), compute_opacity=False)
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), ("the call after the batch", k)
    if row.nz <= 512:
        for a, w in zip(r.radiate_ir_batch(Ts, T), ir_before):
            assert a.tobytes() == w.tobytes()


# ------------------------------------------------------------------ G6
def test_g6_pure_absorption_against_the_closed_forms(hip_lib):
    from clima_amd.radtran import Radtran
    case = CF.absorption_case("nz12")
    tables, nz, sc = case["tables"], case["nz"], case["scalars"]
    r = Radtran(tables, nz, case["nzen"], 0.3)
    for k, v in sc.items():
        setattr(r, k, v)
    r.surface_albedo, r.surface_emissivity = case["albedo"], case["emissivity"]
    r.radiate(*case["column"].args())
    tau, w0 = r.opr()[:2]
    assert np.all(w0 == 0.0)
    al = case["albedo"]
    u, w = np.asarray(r.zenith_u, dtype=float), np.asarray(r.zenith_weights, dtype=float)
    zu, zw = np.stack([u, 0.77 * u, u / 3.0]), np.stack([w, 1.25 * w, 0.3 * w])
    alb, scale = np.stack([0.0 * al, np.ones_like(al), 0.5 * al]), np.array([1.0, 0.4286, 2.5])
    for shared in (1, 0):
        r.solar_batch_shared(shared)
        fup, fdn, ft, spec = r.radiate_solar_batch(zu, zw, alb, scale, spectra_levels=list(range(nz + 1)))
        for c in range(3):
            sol = CF.solar_channel(tables, tau, zu[c], zw[c], alb[c], sc["diurnal_fac"], scale[c])
            e = CF.per_bin(spec["fup"][:, :, c], spec["fdn"][:, :, c], sol.fup_a, sol.fdn_a)
            e_am = CF.per_bin_one(spec["amean"][:, :, c], sol.amean)
            print("shared=%d case %d: per bin worst %.2e, amean %.2e [%.0e]" % (shared, c, e.max(), e_am.max(), TOL_BIN))
            assert np.all(e <= TOL_BIN) and np.all(e_am <= TOL_BIN), (shared, c, e, e_am)
            if c == 0:
                assert np.all(spec["fup"][:, :, c] == 0.0)      # albedo 0, no scattering: nothing comes back up


# ------------------------------------------------------------------ G7
def test_g7_refusals(states):
    from clima_amd.radtran import ClimaException
    row = LF.BY_NAME["h100"]
    s = states(row)
    col = row.column()
    nz, n_sol = row.nz, row.bins()[1]
    n, nzen = 2, 2
    zu, zw = np.full((n, nzen), 0.5), np.full((n, nzen), 0.5)
    out = [np.zeros((nz + 1, n), order="F") for _ in range(3)]
    spec = np.zeros((n, 1, n_sol))
    lv = np.array([1], dtype=np.int32)

    def call(r, ncol=n, nz_=nzen, u=zu, w=zw, fup=out[0], fdn=out[1], ft=out[2], nsel=0, level=None, sp=(None, None, None)):
        d = lambda x: _p(x) if x is not None else None   # noqa: E731
        r._L.radtran_radiate_solar_batch(r._ptr, _i(ncol), _i(nz_), d(u), d(w), None, None, d(fup), d(fdn), d(ft), _i(nsel),
                                         level.ctypes.data_as(IP) if level is not None else None, *[d(x) for x in sp], r._err)
        r._check()

    fresh = s.handle()
    with pytest.raises(ClimaException, match="^radiate_solar_batch needs opacities: call radiate with compute_opacity first$"):
        call(fresh)
    assert row.one_launch
    fresh.TOA_fluxes_batch(s.columns())
    with pytest.raises(ClimaException, match="^radiate_solar_batch needs opacities"):
        call(fresh)
    r = s.handle("refuse")
    r.radiate(*col.args())
    before, n0 = left_state(r), r.solar_batch_shared()[1]
    texts = [
        (dict(ncol=0), r"ncol must be at least 1 \(ncol = 0\)"),
        (dict(nz_=0), r"nzen must lie in 1\.\.16 \(nzen = 0\)"),
        (dict(nz_=17), r"nzen must lie in 1\.\.16 \(nzen = 17\)"),
        (dict(u=None), '"zenith_u" is a required argument'),
        (dict(w=None), '"zenith_weights" is a required argument'),
        (dict(fup=None), '"fup_n" is a required argument'),
        (dict(fdn=None), '"fdn_n" is a required argument'),
        (dict(nsel=-1), r"nsel must not be negative \(nsel = -1\)"),
        (dict(nsel=1, sp=(spec, None, None)), '"spec_level" is a required argument'),
        (dict(nsel=1, level=np.array([0], dtype=np.int32), sp=(spec, None, None)), r"spec_level\(1\) = 0 is outside 1\.\.%d" % (nz + 1)),
        (dict(nsel=1, level=np.array([nz + 2], dtype=np.int32), sp=(spec, None, None)), r"spec_level\(1\) = %d is outside 1\.\.%d" % (nz + 2, nz + 1)),
        (dict(nsel=1, level=lv), "nsel = 1, but none of sol_fup, sol_fdn, sol_amean was given"),
    ]
    for kw, text in texts:
        with pytest.raises(ClimaException, match="^radiate_solar_batch: " + text):
            call(r, **kw)
    assert r.solar_batch_shared()[1] == n0                       # nothing ran
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    # f_total may be NULL; nsel = 0 leaves the spectrum arrays unread
    call(r, ft=None)
    call(r)
    # the Python checks come first
    with pytest.raises(ClimaException, match='"nope" is not one of fup, fdn, amean'):
        r.radiate_solar_batch(zu, zw, spectra_levels=[0], spectra=("nope",))
    with pytest.raises(ClimaException, match=r'"surface_albedo" has the shape \(2, 3\), not \(2, %d\)' % n_sol):
        r.radiate_solar_batch(zu, zw, surface_albedo=np.ones((2, 3)))
    # a communicator (one rank), and a bin shard on it: the whole spectrum is needed; nothing runs, the state stays
    cm = s.handle()
    cm.comm_init_rank(1, 0, type(cm).comm_unique_id())
    cm.radiate(*col.args())
    before, n0, reduces = left_state(cm), cm.solar_batch_shared()[1], cm.comm()[2]
    with pytest.raises(ClimaException, match=r"^radiate_solar_batch: needs the whole spectrum \(a communicator\)$"):
        call(cm)
    assert cm.solar_batch_shared()[1] == n0 and cm.comm()[2] == reduces
    after = left_state(cm)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    cm.set_bin_shard(0, 2)
    with pytest.raises(ClimaException, match=r"^radiate_solar_batch: needs the whole spectrum \(a bin shard of 2, a communicator\)$"):
        call(cm)
    cm.comm_destroy()
    # a bin shard without a communicator
    sh = s.handle()
    sh.radiate(*col.args())
    sh.set_bin_shard(0, 2)
    with pytest.raises(ClimaException, match=r"^radiate_solar_batch: needs the whole spectrum \(a bin shard of 2\)$"):
        call(sh)
    assert sh.solar_batch_shared()[1] == 0


def test_f_total_after_a_profile_reset(states):
    """whether the handle holds level rows is what Holds records, not a counter of the profiling: a batch with f_total
    runs after profile_reset(), and gives what it gave before"""
    row = LF.BY_NAME["h100"]
    s = states(row)
    r = s.handle()
    r.radiate(*row.column().args())
    u = np.array([0.3, 0.9])
    want = r.radiate_solar_batch(u)
    r.profile(True)
    r.profile_reset()
    got = r.radiate_solar_batch(u)
    r.profile(False)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["nz1", "s64"])
def test_g4_the_chunk_seam(states, name):
    """more than 512 cases run as chunks of 512: the cases behind the seam are the cases they are alone, in both forms
    (their angles, albedo, scale, level rows and spectra all sit at offsets of the chunk's first case)"""
    row = LF.BY_NAME[name]
    s = states(row)
    r = s.handle("solar")
    r.radiate(*row.column().args())
    rng = np.random.default_rng(9)
    n, n_sol, lv = 515, row.bins()[1], s.levels()
    zu, zw = rng.uniform(0.05, 1.0, (n, row.nzen)), rng.uniform(0.1, 1.0, (n, row.nzen))
    al, sc = rng.uniform(0.0, 1.0, (n, n_sol)), rng.uniform(0.1, 2.0, n)
    for shared in (1, 0):
        r.solar_batch_shared(shared)
        big = r.radiate_solar_batch(zu, zw, al, sc, spectra_levels=lv)
        for lo, hi in ((511, 513), (514, 515)):
            part = r.radiate_solar_batch(zu[lo:hi], zw[lo:hi], al[lo:hi], sc[lo:hi], spectra_levels=lv)
            for a in range(3):
                assert np.ascontiguousarray(big[a][:, lo:hi]).tobytes() == np.ascontiguousarray(part[a]).tobytes(), (shared, lo, a)
            for k in part[3]:
                assert np.ascontiguousarray(big[3][k][:, :, lo:hi]).tobytes() == part[3][k].tobytes(), (shared, lo, k)
        assert not np.array_equal(big[0][:, 512], big[0][:, 0])
    r.solar_batch_shared(1)
