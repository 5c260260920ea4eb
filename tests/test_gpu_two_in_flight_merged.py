"""Two resident calls in flight, each keeping its frequency integration back IN ITS CALL SLOT: the call that next takes
the slot -- two calls on, on the same lane -- launches it in one grid with its own prep pass (k_prep_integrate), a join
launches what is pending in both slots, the older call's first (include/clima_radtran_hip.h,
radtran_calls_in_flight_set).  Every comparison here is BITWISE -- level rows, f_total, the seven spectra -- against the
same sequence on a second handle with `calls_in_flight = 1`, whose calls run one behind the other.

Shapes (nw = 100, 4 zenith angles, calls_in_flight = 2), those of test_gpu_two_in_flight.py:
  nz = 70,  coop_items = 0: the fused half-wave grid with whole stores -> the merged launch is taken
  nz = 230, coop_items = 0: the whole-wave fused grid accumulates, so the prep pass clears -> never merged
  nz = 40:                  not fused, separate launches, the prep pass clears -> never merged

merged_integrations after N >= 2 pipelined calls and one synchronize: at nz = 70 calls 3 .. N each take the integration
of the call two before them along, and the join launches the last two alone, the older one included (it is not
dropped): (N - 2, 2).  Where a call's own prep pass clears, the call integrates at once -- nothing is kept back that
could not merge: (0, 0).  A kept-back integration still meets a prep pass that clears when the launch form changes
between two calls (coop_items): it then goes out first, alone, on that slot's lane."""
import numpy as np
import pytest

from test_gpu_merged_integration import SPECTRA, _assert_same_state, _rows
from test_gpu_two_in_flight import (_flux_tensor, _ir_batch, _ir_only, _jacobian, _opr, _set_albedo, _set_scale,
                                    _solar_batch, _spectra, _toa, _toa_batch)

pytestmark = pytest.mark.gpu

SHAPES = [(70, True), (230, True), (40, False)]


@pytest.fixture(scope="module")
def tables():
    from clima_amd import synthetic as S
    return S.modern_earth_tables(nw=100)


def _columns(nz):
    from clima_amd import synthetic as S
    return S.perturbed_columns(2, nz=nz, seed=23)


def _handle(tables, nz, coop0, mode, fused=True):
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, 4, 0.2)
    if coop0:
        r.coop_items = 0
    r.calls_in_flight = mode
    r.fused = fused
    return r


def _pair(tables, nz, coop0):
    """(handle that keeps two calls in flight, reference handle that runs one at a time)"""
    return _handle(tables, nz, coop0, 2), _handle(tables, nz, coop0, 1)


def _counts(nz, n):
    """merged_integrations of n >= 2 pipelined calls and one synchronize, two in flight (the module's docstring)"""
    return (n - 2, 2) if nz == 70 else (0, 0)


@pytest.mark.parametrize("uploads", ["each", "one"])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
@pytest.mark.parametrize("nz,coop0", SHAPES)
def test_pending_in_both_slots_at_the_end(tables, nz, coop0, n, uploads):
    """n pipelined calls, then synchronize: the join finds an integration pending in either slot"""
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, coop0)
    for h in (r, ref):
        for i in range(n):
            if uploads == "each" or i == 0:
                h.upload_column(*(A, B)[(i + (uploads == "one")) % 2].args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == n - 1 and ref.overlapped_calls == 0
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
    assert r.merged_integrations == _counts(nz, n)
    assert ref.merged_integrations == ((n - 1, 1) if nz == 70 else (0, n))     # one at a time: the chain of one lane
    assert np.all(_rows(r)[: nz + 1] > 0.0)          # (upward IR at every level: the rows were written)


def test_kept_back_integration_in_front_of_a_prep_pass_that_clears(tables):
    """two pipelined calls in the half-wave fused form keep their integrations back, one in each slot; then coop_items
    goes back to its default, which takes these calls out of the fused grid: their prep pass clears the spectra.  Calls 3
    and 4 find the pending integration of their slot and launch it first, alone, on that slot's lane, and integrate
    at once themselves."""
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, False)
    for h in (r, ref):
        default = h.coop_items
        h.coop_items = 0
        for c in (A, B):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.coop_items = default
        for c in (B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 3 and r.fused_fallbacks == 0
    assert r.merged_integrations == (0, 2)


def _upload(h, A, B):
    h.upload_column(*B.args())
    return []


def _albedo(h, A, B):
    _set_albedo(h)
    return []


def _scale(h, A, B):
    _set_scale(h)
    return []


READS = (_ir_only, _toa, _ir_batch, _jacobian, _toa_batch, _spectra, _opr, _solar_batch, _flux_tensor)


@pytest.mark.parametrize("then", READS + (_albedo, _scale, _upload), ids=lambda f: f.__name__.strip("_"))
def test_three_pipelined_calls_followed_by(tables, then):
    """three pipelined calls leave an integration pending in either slot (the third took the first one's along); then an
    entry point that joins -- or an upload, which does not --, two more pipelined calls and a synchronize"""
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    got = []
    for h in (r, ref):
        for c in (A, B, A):
            h.upload_column(*c.args())
            h.radiate_resident()
        assert h.merged_integrations == ((1, 0) if h is r else (2, 0))
        got.append(then(h, A, B))
    assert r.overlapped_calls == 2 and ref.overlapped_calls == 0
    assert len(got[0]) == len(got[1])
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    if then in READS:
        _assert_same_state(r, ref, "after " + then.__name__)
    for h in (r, ref):
        for c in (B, A):
            if then is not _upload or c is A:        # (the upload under test is the fourth call's)
                h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref, "two calls after " + then.__name__)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
    if then is _upload:                              # nothing joined: five pipelined calls
        assert r.overlapped_calls == 4 and r.merged_integrations == _counts(nz, 5)


def test_reading_rows_between_calls(tables):
    """every read joins and launches what is pending: nothing merges across it, and the rows are each call's own"""
    nz = 70
    A, B = _columns(nz)
    r, ref = _pair(tables, nz, True)
    seen = []
    for c in (A, B, A):
        got = []
        for h in (r, ref):
            h.upload_column(*c.args())
            h.radiate_resident()
            got.append(_rows(h).copy())
        np.testing.assert_array_equal(got[0], got[1])
        seen.append(got[0])
    assert not np.array_equal(seen[0], seen[1])       # A's rows, then B's: each read saw its own call
    np.testing.assert_array_equal(seen[0], seen[2])
    assert r.overlapped_calls == 0                    # every read joined: each call stayed where the handle was
    assert r.merged_integrations == (0, 3)
    # ... and three pipelined calls behind it: the first stays where the handle is, the third merges the first's
    for h in (r, ref):
        for c in (B, A, B):
            h.upload_column(*c.args())
            h.radiate_resident()
        h.synchronize()
    _assert_same_state(r, ref)
    assert r.overlapped_calls == 2
    assert r.merged_integrations == (1, 5)


def test_forced_expiry_of_the_last_of_four(tables):
    """fused_spins = 0 on the last of four pipelined calls, an integration pending in either slot: the synchronise joins,
    launches both, finds the flag and repeats that one call through the separate launches, in its own slot, its
    integration behind the repair.  Reference: a handle with the fused grid off."""
    nz = 70
    A, B = _columns(nz)
    r, ref = _handle(tables, nz, True, 2), _handle(tables, nz, True, 1, fused=False)
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
    assert r.merged_integrations == _counts(nz, 4)
    _assert_same_state(r, ref)


def test_automatic_mode_at_the_benchmark_shape():
    """config 2 (200 layers, 1 000 bins, 8 zenith angles), six calls: two in flight by the automatic rule, calls 3 .. 6
    each merge the integration of the call two before them"""
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
    assert r.merged_integrations == (4, 2) and ref.merged_integrations == (5, 1)
    assert r.fused_fallbacks == 0 and ref.fused_fallbacks == 0
