"""A resident call keeps its frequency integration back; the next compute_opacity call launches it in one grid with
its own prep pass (k_prep_integrate), everything else launches it first, alone (include/clima_radtran_hip.h,
radtran_defer_integration_set).  Every comparison here is BITWISE, against the same sequence on a second handle with
`defer_integration = 0`, whose calls integrate at once.

Shapes (nw = 100: a partial last 32-bin chunk in both channels):
  nz = 70,  coop_items = 0: the fused half-wave grid, whole stores -> the merged launch is taken; 71 levels are five
                            level blocks of 16, the last one partial
  nz = 40:                  unfused, the prep pass clears the spectra -> the pending integration goes alone
  nz = 230, coop_items = 0: the whole-wave fused grid accumulates, so the prep pass clears -> alone"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPECTRA = ("ir_fup_a", "ir_fdn_a", "ir_tau_band", "sol_fup_a", "sol_fdn_a", "sol_amean", "sol_tau_band")


@pytest.fixture(scope="module")
def tables():
    from clima_amd import synthetic as S
    return S.modern_earth_tables(nw=100)


def _columns(nz):
    from clima_amd import synthetic as S
    return S.perturbed_columns(2, nz=nz, seed=23)


def _pair(tables, nz, coop0):
    """(deferring handle, reference handle that integrates at once)"""
    from clima_amd.radtran import Radtran
    out = []
    for defer in (True, False):
        r = Radtran(tables, nz, 4, 0.2)
        if coop0:
            r.coop_items = 0
        assert r.defer_integration          # on by default
        r.defer_integration = defer
        assert r.defer_integration == defer
        out.append(r)
    return out


def _rows(r):
    return np.concatenate([np.asarray(r.wrk_ir.fup_n), np.asarray(r.wrk_ir.fdn_n), np.asarray(r.wrk_sol.fup_n),
                           np.asarray(r.wrk_sol.fdn_n), np.asarray(r.f_total)])


def _assert_same_state(r, ref, what=""):
    np.testing.assert_array_equal(_rows(r), _rows(ref), err_msg="level rows / f_total " + what)
    a, b = r.spectra_all(), ref.spectra_all()
    for k in SPECTRA:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k + " " + what)


@pytest.mark.parametrize("nz,coop0,merged", [(70, True, 2), (40, False, 0), (230, True, 0)])
def test_three_pipelined_calls(tables, nz, coop0, merged):
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, coop0)
    for h in (r, ref):
        for c in (A, B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
    assert r.merged_integrations == (merged, 3 - merged)
    assert ref.merged_integrations == (0, 0)
    assert np.all(_rows(r)[: nz + 1] > 0.0)          # (upward IR at every level: the rows were written)


def test_reading_rows_between_calls_flushes(tables):
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
    assert r.merged_integrations == (0, 3)
    # ... and a pipelined pair behind it is still right
    for h in (r, ref):
        for c in (B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.merged_integrations == (1, 4)


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


@pytest.mark.parametrize("then", [_ir_only, _toa, _ir_batch, _jacobian, _toa_batch, _spectra], ids=lambda f: f.__name__.strip("_"))
def test_deferred_call_followed_by(tables, then):
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    got = []
    for h in (r, ref):
        for c in (A, B):                     # the second call takes the first one's integration along: B's is pending
            h.upload_column(*c.args())
            h.radiate_resident()
        got.append(then(h, A, B))
    # (a synchronous call resolves what it finds pending by the same rule: TOA_fluxes' own prep launch takes B's integration)
    # ... and the IR-only resident call keeps its own integration back in turn: its synchronise launches that one too)
    assert r.merged_integrations == {_toa: (2, 0), _ir_only: (1, 2)}.get(then, (1, 1))
    assert len(got[0]) == len(got[1])
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    _assert_same_state(r, ref, "after " + then.__name__)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0


def test_flux_tensor_read_in_stream_order(tables):
    import torch
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    stream = torch.cuda.ExternalStream(r.stream())
    want = {}
    for name, c in (("A", A), ("B", B)):
        ref.upload_column(*c.args())
        ref.radiate_resident()
        ref.synchronize()
        want[name] = _rows(ref)[: 4 * (nz + 1)]
    r.upload_column(*A.args())
    r.radiate_resident()
    t = r.flux_tensor()                      # hands the pointer out: what is pending goes out now
    with torch.cuda.stream(stream):
        got = t.clone()
    stream.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want["A"])
    assert r.merged_integrations == (0, 1)
    # deferral is off from then on: a read with no library call at all between the call and it
    r.upload_column(*B.args())
    r.radiate_resident()
    with torch.cuda.stream(stream):
        got = t.clone()
    stream.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want["B"])
    r.upload_column(*A.args())
    r.radiate_resident()
    r.synchronize()
    assert r.merged_integrations == (0, 1)
    assert r.defer_integration               # the switch itself is the caller's


def test_forced_repeat_of_the_last_deferred_call(tables):
    """fused_spins = 0 on the last of three deferred calls: every hand-off wait of its fused grid that is not satisfied
    at the first poll expires, the synchronise finds the flag behind the call's (stand-alone) integration and repeats the
    call through the separate launches -- whose results are those of a handle with the fused grid off."""
    from clima_amd.radtran import Radtran
    nz = 70
    A, B = _columns(nz)
    r, _ = _pair(tables, nz, True)
    ref = Radtran(tables, nz, 4, 0.2)
    ref.coop_items = 0
    ref.defer_integration = False
    ref.fused = False
    for h in (r, ref):
        for i, c in enumerate((A, B, A)):
            h.upload_column(*c.args())
            if i == 2 and h is r:
                h.fused_spins = 0
            h.radiate_resident()
        n0 = h.fused_fallbacks
        h.synchronize()
        assert h.fused_fallbacks == n0 + (1 if h is r else 0)
    assert r.merged_integrations == (2, 1)
    _assert_same_state(r, ref)
