"""Two resident calls in flight (include/clima_radtran_hip.h, radtran_calls_in_flight_set): consecutive pipelined
`radiate_resident` calls alternate between two sets of work buffers and two streams, everything else joins first.  Every
comparison here is BITWISE -- level rows, f_total, the seven spectra -- against the same sequence on a second handle with
`calls_in_flight = 1`, whose calls run one behind the other.

Shapes (nw = 100, 4 zenith angles, calls_in_flight = 2: these grids are far too small for the automatic rule):
  nz = 70,  coop_items = 0: the fused half-wave grid with whole stores -- the benchmark's form
  nz = 230, coop_items = 0: the whole-wave fused grid accumulates, so the prep pass clears the slot's own spectra
  nz = 40:                  not fused, separate launches"""
import numpy as np
import pytest

from test_gpu_merged_integration import SPECTRA, _assert_same_state, _rows

pytestmark = pytest.mark.gpu

SHAPES = [(70, True), (230, True), (40, False)]


@pytest.fixture(scope="module")
def tables():
    from clima_amd import synthetic as S
    return S.modern_earth_tables(nw=100)


def _columns(nz):
    from clima_amd import synthetic as S
    return S.perturbed_columns(2, nz=nz, seed=23)


def _handle(tables, nz, coop0, mode, nzen=4, albedo=0.2):
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, nzen, albedo)
    if coop0:
        r.coop_items = 0
    assert r.calls_in_flight == 0            # automatic by default
    r.calls_in_flight = mode
    assert r.calls_in_flight == mode
    return r


def _pair(tables, nz, coop0):
    """(handle that keeps two calls in flight, reference handle that runs one at a time)"""
    return _handle(tables, nz, coop0, 2), _handle(tables, nz, coop0, 1)


@pytest.mark.parametrize("nz,coop0", SHAPES)
def test_pipelined_with_uploads(tables, nz, coop0):
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, coop0)
    for h in (r, ref):
        for c in (A, B, A, B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 4 and ref.overlapped_calls == 0
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
    assert np.all(_rows(r)[: nz + 1] > 0.0)          # (upward IR at every level: the rows were written)
    # ... and the call before the last one was B's, in the other slot: a different column gives different rows
    ref.upload_column(*B.args())
    ref.radiate_resident()
    ref.synchronize()
    assert not np.array_equal(_rows(r), _rows(ref))


@pytest.mark.parametrize("nz,coop0", SHAPES)
def test_pipelined_one_upload(tables, nz, coop0):
    """the second call's slot has never seen the column: one device copy in front of its prep pass"""
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, coop0)
    for h in (r, ref):
        h.upload_column(*B.args())
        for _ in range(3):
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 2
    assert r.fused_fallbacks == 0
    # an upload between pipelined calls, then two calls on it: the slot that was passed over gets the column copied
    for h in (r, ref):
        h.radiate_resident()
        h.upload_column(*A.args())
        h.radiate_resident()
        h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref, "after an upload between pipelined calls")
    assert r.overlapped_calls == 4
    assert r.fused_fallbacks == 0


def test_reading_rows_between_calls(tables):
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    seen = []
    for c in (A, B, A):
        got = []
        for h in (r, ref):
            h.upload_column(*c.args())
            h.radiate_resident()
            got.append(np.asarray(h.wrk_ir.fup_n).copy())
        np.testing.assert_array_equal(got[0], got[1])
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1])       # A's rows, then B's: each read saw its own call
    np.testing.assert_array_equal(seen[0], seen[2])
    assert r.overlapped_calls == 0                    # every read joined: each call stayed where the handle was
    # ... and a pipelined pair behind it is still right
    for h in (r, ref):
        for c in (B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 1


def _ir_only(h, A, B):
    c = dict(A)
    c["T"] = np.asarray(A["T"]) + 2.5
    h.upload_column(c["T_surface"] + 1.0, c["T"], c["P"], c["densities"], c["dz"], c.get("pdensities"), c.get("radii"))
    h.radiate_resident(compute_solar=False, compute_opacity=False)
    h.synchronize()
    return []


def _toa(h, A, B):
    return [np.array(h.TOA_fluxes(*B.args()))]


def _ir_batch(h, A, B):
    T = np.stack([np.asarray(B["T"]) + d for d in (0.0, 1.0, -2.0)], axis=1)
    return list(h.radiate_ir_batch(np.array([B["T_surface"]] * 3), T))


def _jacobian(h, A, B):
    return list(h.ir_jacobian(B["T_surface"], B["T"]))


def _toa_batch(h, A, B):
    return list(h.TOA_fluxes_batch([A, B, A], return_fluxes=True))


def _spectra(h, A, B):
    s = h.spectra_all()
    return [s[k].copy() for k in SPECTRA]


def _opr(h, A, B):
    return list(h.opr())


def _solar_batch(h, A, B):
    u = np.array([[0.3, 0.8], [0.55, 0.95], [0.2, 0.6]])
    return list(h.radiate_solar_batch(u, np.full_like(u, 0.5)))


def _flux_tensor(h, A, B):
    """the pointer goes out and is read in stream order: on the handle's stream, with no other library call"""
    import torch
    t = h.flux_tensor()
    stream = torch.cuda.ExternalStream(h.stream())
    with torch.cuda.stream(stream):
        got = t.clone()
    stream.synchronize()
    return [got.cpu().numpy()]


@pytest.mark.parametrize("then", [_ir_only, _toa, _ir_batch, _jacobian, _toa_batch, _spectra, _opr, _solar_batch, _flux_tensor],
                         ids=lambda f: f.__name__.strip("_"))
def test_two_in_flight_followed_by(tables, then):
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    got = []
    for h in (r, ref):
        for c in (A, B):                     # B's call runs beside A's, in the other slot
            h.upload_column(*c.args())
            h.radiate_resident()
        got.append(then(h, A, B))
    assert r.overlapped_calls == 1 and ref.overlapped_calls == 0
    assert len(got[0]) == len(got[1])
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    _assert_same_state(r, ref, "after " + then.__name__)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0


def _set_albedo(h):
    h.surface_albedo = np.linspace(0.05, 0.6, len(h.surface_albedo))


def _set_scale(h):
    h.photon_scale_factor = 0.4286


@pytest.mark.parametrize("setter", [_set_albedo, _set_scale], ids=lambda f: f.__name__.strip("_"))
def test_setter_between_calls(tables, setter):
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    old = _handle(tables, nz, True, 1)       # A alone, under the old value
    old.upload_column(*A.args())
    old.radiate_resident()
    old.synchronize()
    # the call in flight when the setter comes ran with the old value (its rows, read behind the setter)
    for h in (r, ref):
        for c in (B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        setter(h)
    np.testing.assert_array_equal(_rows(r), _rows(old))
    _assert_same_state(r, old, "the call before the setter")
    # ... and the next calls with the new one
    for h in (r, ref):
        for c in (A, B):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref, "the calls after the setter")
    assert not np.array_equal(np.asarray(r.wrk_sol.fup_n), np.asarray(old.wrk_sol.fup_n))
    # and with no read in between: call i under the old value, call i + 1 under the new
    r2, ref2 = _pair(tables, nz, True)
    for h in (r2, ref2):
        h.upload_column(*A.args())
        h.radiate_resident()
        h.upload_column(*B.args())
        h.radiate_resident()
        setter(h)
        h.upload_column(*A.args())
        h.radiate_resident()
        h.synchronize()
    _assert_same_state(r2, ref2, "setter between two pipelined calls")
    assert r2.fused_fallbacks == 0


def _expiry_handles(tables, nz, fused_ref):
    from clima_amd.radtran import Radtran
    r = _handle(tables, nz, True, 2)
    ref = Radtran(tables, nz, 4, 0.2)
    ref.coop_items = 0
    ref.calls_in_flight = 1
    ref.fused = fused_ref
    return r, ref


def test_forced_expiry_of_the_last_of_four(tables):
    """fused_spins = 0 on the last of four pipelined calls: every hand-off wait of its fused grid that is not satisfied at
    the first poll expires; the synchronise repeats that one call through the separate launches, in its own slot.
    Reference: a handle with the fused grid off."""
    nz = 70
    A, B = _columns(nz)
    r, ref = _expiry_handles(tables, nz, False)
    for h in (r, ref):
        for i, c in enumerate((A, B, A, B)):
            h.upload_column(*c.args())
            if i == 3 and h is r:
                h.fused_spins = 0
            h.radiate_resident()
        n0 = h.fused_fallbacks
        h.synchronize()
        assert h.fused_fallbacks == n0 + (1 if h is r else 0)
    assert r.overlapped_calls == 3
    _assert_same_state(r, ref)


def test_forced_expiry_of_the_third_of_four(tables):
    """fused_spins = 0 on the third of four pipelined calls only; the fourth runs beside it, in the other slot, with the
    handle's usual bound.  The timeout word then holds the third call's id, not the latest call's: nothing is repeated, and
    the fourth call's results -- the only ones observable -- are what they would have been.  The reference runs the same
    four calls one at a time with the fused grid on: the fourth call's state is that of a fused call, which no repeat
    through the separate launches touched.  (The handle with the fused grid off is the reference of the case above, where
    the repeat runs; here nothing runs through the separate launches, and at this shape those differ from the fused grid
    in the last bits -- 6.9e-13 of the largest level flux, measured: their whole-wave kernel sums a bin's g-points in
    another order than the fused half-wave grid.)"""
    nz = 70
    A, B = _columns(nz)
    r, ref = _expiry_handles(tables, nz, True)
    for h in (r, ref):
        spins = h.fused_spins
        for i, c in enumerate((A, B, A, B)):
            h.upload_column(*c.args())
            if h is r:
                h.fused_spins = 0 if i == 2 else spins
            h.radiate_resident()
        n0 = h.fused_fallbacks
        h.synchronize()
        assert h.fused_fallbacks == n0              # an older call's expiry needs no repair
    assert r.overlapped_calls == 3
    _assert_same_state(r, ref)


def test_automatic_mode_keeps_small_grids_in_one_chain(tables):
    from clima_amd.radtran import Radtran
    nz = 70
    A, B = _columns(nz)
    r = Radtran(tables, nz, 4, 0.2)
    for c in (A, B, A):
        r.upload_column(*c.args())
        r.radiate_resident()
    r.synchronize()
    assert r.overlapped_calls == 0
    assert r.merged_integrations[0] + r.merged_integrations[1] == 3      # each call kept its integration back, as before


def test_automatic_mode_at_the_benchmark_shape():
    """config 2 (200 layers, 1 000 bins, 8 zenith angles): 7 928 waves against the 2 048 of one residency round"""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    tb = S.modern_earth_tables()
    A, B = S.perturbed_columns(2, nz=200, seed=23)
    r, ref = Radtran(tb, 200, 8, 0.15), Radtran(tb, 200, 8, 0.15)
    ref.calls_in_flight = 1
    for h in (r, ref):
        for c in (A, B, A, B, A, B):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 5 and ref.overlapped_calls == 0
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
