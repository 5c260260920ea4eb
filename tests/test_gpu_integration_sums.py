"""Every sum over the bins, fup_n(i) = sum_l fup_a(i,l) * (freq(l) - freq(l+1)) (clima_radtran_radiate.f90:184-192), held
to the exact rational sum of its own inputs (tests/exact_bin_sums.py) at the bin counts where an integration kernel takes
another path: k_integrate_one and k_prep_integrate (integrate_block: a chunk, the wraps of its chunk loop, the LDS limits),
the two-launch pair k_integrate_partial / k_integrate_final, the batch pair k_integrate_partial_b / k_integrate_final_b
(its eight-wide loop, an empty shard) and k_rows_integrate.

Hook level (clima_test_integrate: the production launchers on arrays given directly).  Integer inputs: every product and
partial sum is an integer below 2^53, so a kernel must return the exact sum BITWISE whatever its order; a dropped, repeated
or mis-weighted bin changes the integer.  Real inputs: |got - S| <= (INT_CHUNK + nchunk + 3) 2^-53 A, derived in
exact_bin_sums.py, never measured; every test prints the largest share of that bound it saw.  Forms 0 (what a call
launches) and 1 (the two-launch pair, forced) agree bitwise: integrate_block's "same association as the two-launch form".

Handle level: the entry points compute lo / n, nchunk, LDS and buffer sizes themselves, so each is run on handles of
1025, 3393 and 5441 bins in both channels and its level rows are held to the exact sums of the per-bin arrays the same
call left or returned."""
import ctypes as C

import numpy as np
import pytest

import exact_bin_sums as E

pytestmark = pytest.mark.gpu

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
_worst = {}


def _i(v):
    return C.byref(C.c_int(int(v)))


def _p(a):
    return a.ctypes.data_as(DP)


def _ints(*v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _note(test, share):
    """the largest share of the bound a test saw, printed as it grows"""
    _worst[test] = max(_worst.get(test, 0.0), share)
    return share


def _report(test):
    print("\n    %s: largest share of the bound %.3f" % (test, _worst.get(test, 0.0)))


class Channel:
    """freq [nw+1], up / dn [ncol][nw][nl], the owned range"""

    def __init__(self, freq, arrays, lo=0, n=None):
        self.freq = np.ascontiguousarray(freq, dtype=np.float64)
        self.up, self.dn = (np.ascontiguousarray(arrays[:, k]) for k in (0, 1))
        self.nw = len(self.freq) - 1
        self.lo, self.n = lo, self.nw - lo if n is None else n
        assert self.up.shape[1] == self.nw and 0 <= self.lo and self.lo + self.n <= self.nw

    def dims(self):
        return _ints(self.nw, self.lo, self.n)

    def rows(self, col=0):
        return self.up[col], self.dn[col]


def integrate(L, form, ir, sol, do_solar=True, flux_n=None, flux_part=None, spec_pad=0, flux_pad=0):
    """clima_test_integrate, forms 0 and 1 -> (flux_n [ncol][4][nl], flux_part [4][nl] or None)"""
    ncol, _, nl = ir.up.shape
    assert sol.up.shape[0] == ncol and sol.up.shape[2] == nl
    flux = np.full((ncol, 4, nl), np.nan) if flux_n is None else np.array(flux_n, dtype=np.float64).reshape(ncol, 4, nl)
    part = None if flux_part is None else np.array(flux_part, dtype=np.float64).reshape(4, nl)
    err = C.create_string_buffer(1025)
    L.clima_test_integrate(_i(form), _i(nl - 1), _i(ncol), _i(max(ir.nw, sol.nw) * nl + spec_pad), _i(4 * nl + flux_pad),
                           ir.dims(), _p(ir.freq), sol.dims(), _p(sol.freq), _p(ir.up), _p(ir.dn), _p(sol.up), _p(sol.dn),
                           _i(do_solar), _p(flux), None if part is None else _p(part), _i(0), None, err)
    assert err.value == b"", err.value.decode()
    return flux, part


def integrate_batch(L, ir, flux_n, col0, out, spec_pad=0):
    """clima_test_integrate, form 2 -> out [3][col0 + ncol][nl]"""
    ncol, _, nl = ir.up.shape
    out = np.array(out, dtype=np.float64)
    assert out.shape == (3, col0 + ncol, nl)
    flux = np.ascontiguousarray(flux_n, dtype=np.float64)
    err = C.create_string_buffer(1025)
    L.clima_test_integrate(_i(2), _i(nl - 1), _i(ncol), _i(ir.nw * nl + spec_pad), _i(0), ir.dims(), _p(ir.freq), _ints(0, 0, 0),
                           None, _p(ir.up), _p(ir.dn), None, None, _i(0), _p(flux), None, _i(col0), _p(out), err)
    assert err.value == b"", err.value.decode()
    return out


def _exact(ch, col=0):
    """[(S, A) of up, (S, A) of dn] over the channel's owned bins"""
    return [E.exact_rows(a, ch.freq, ch.lo, ch.n) for a in ch.rows(col)]


def _ints_of(ch, col=0):
    return [E.int_rows(a, ch.freq, ch.lo, ch.n) for a in ch.rows(col)]


def _assert_int_rows(got, want, what):
    got = np.asarray(got)
    assert np.all(got == np.floor(got)) and [int(x) for x in got.tolist()] == want, \
        "%s: %s, exact %s" % (what, [int(x) for x in got.tolist()][:4], want[:4])


def _assert_within(test, got, SA, factor, what):
    sh = max(E.shares(got, SA[0], SA[1], factor))
    _note(test, sh)
    assert sh <= 1.0, "%s: %.3g of the bound %d u A" % (what, sh, factor)
    return sh


def _int_channels(key, nl, n_ir, n_sol, ncol=1):
    rng = E.case_rng(*key)
    return Channel(*E.integer_channel(rng, n_ir, nl, ncol)), Channel(*E.integer_channel(rng, n_sol, nl, ncol))


def _real_channels(key, nl, n_ir, n_sol, ncol=1, signed=False):
    rng = E.case_rng(*key)
    return (Channel(*E.real_channel(rng, n_ir, nl, ncol, signed)), Channel(*E.real_channel(rng, n_sol, nl, ncol, signed)))


# ------------------------------------------------------------------ hook level: forms 0 and 1
def _hold_integer(L, ir, sol, forms=(0, 1), what=""):
    want = _ints_of(ir) + _ints_of(sol)
    for form in forms:
        flux, _ = integrate(L, form, ir, sol)
        for a in range(4):
            _assert_int_rows(flux[0, a], want[a], "%s form %d row %d" % (what, form, a))


def _hold_real(test, L, ir, sol, what=""):
    exact = _exact(ir) + _exact(sol)
    factor = E.chunked_factor(max(ir.n, sol.n))
    got = [integrate(L, form, ir, sol)[0] for form in (0, 1)]
    for form in (0, 1):
        for a in range(4):
            _assert_within(test, got[form][0, a], exact[a], factor, "%s form %d row %d" % (what, form, a))
    # (where form 0 took the two launches itself this compares the pair with itself)
    np.testing.assert_array_equal(got[0], got[1], err_msg="%s: the one launch and the two-launch pair differ" % what)


@pytest.mark.parametrize("count", E.COUNTS)
def test_integer_inputs_give_the_exact_sums_bitwise(hip_lib, count):
    for nl in E.LEVELS:
        ir, sol = _int_channels((10, count, nl), nl, count, count)
        _hold_integer(hip_lib, ir, sol, what="%d bins x %d levels" % (count, nl))


@pytest.mark.parametrize("count", E.COUNTS)
def test_real_inputs_within_the_derived_bound(hip_lib, count):
    nl = E.LEVELS_OF[count]
    ir, sol = _real_channels((11, count), nl, count, count)
    _hold_real("real inputs, %d bins" % count, hip_lib, ir, sol, "%d bins x %d levels" % (count, nl))
    _report("real inputs, %d bins" % count)


def test_mixed_signs_the_bound_is_on_the_absolute_sum(hip_lib):
    """spectra in [-1, 1]: A is far above |S|, and the error is held against A -- against |S| no bound of this kind holds"""
    count, nl, test = 1025, 17, "mixed signs"
    ir, sol = _real_channels((12,), nl, count, count, signed=True)
    exact = _exact(ir) + _exact(sol)
    assert all(abs(s) < a / 4 for S, A in exact for s, a in zip(S, A))
    _hold_real(test, hip_lib, ir, sol, "mixed signs")
    flux, _ = integrate(hip_lib, 0, ir, sol)
    on_sum = max(max(E.shares(flux[0, a], exact[a][0], [abs(s) for s in exact[a][0]], E.chunked_factor(count))) for a in range(4))
    print("\n    mixed signs: largest share of the bound on A %.3f; the same errors over the bound with |S| in A's place %.3f"
          % (_worst[test], on_sum))


@pytest.mark.parametrize("n_ir,n_sol", E.UNEQUAL)
def test_unequal_channels(hip_lib, n_ir, n_sol):
    """nchunk is the larger channel's: the shorter channel's later chunks are empty and add 0.0"""
    test = "unequal channels %d / %d" % (n_ir, n_sol)
    for nl in (16, 17):
        ir, sol = _int_channels((13, n_ir, n_sol, nl), nl, n_ir, n_sol)
        _hold_integer(hip_lib, ir, sol, what=test)
    ir, sol = _real_channels((14, n_ir, n_sol), 17, n_ir, n_sol)
    _hold_real(test, hip_lib, ir, sol, test)
    _report(test)


# (IR bins, lo, n), (solar bins, lo, n): a bin shard inside its channel; the last one takes the two launches in form 0
SHARDS = [((100, 33, 40), (90, 1, 31)), ((1100, 37, 1025), (90, 33, 40)), ((60, 20, 33), (2100, 50, 2049)),
          ((5600, 100, 5441), (5600, 159, 5441))]


@pytest.mark.parametrize("ir_dims,sol_dims", SHARDS, ids=lambda d: "%d-%d-%d" % d)
def test_a_bin_shard_sums_its_own_bins_and_leaves_them_in_flux_part(hip_lib, ir_dims, sol_dims):
    test, nl = "bin shard %s %s" % (ir_dims, sol_dims), 17
    L = hip_lib
    rng = E.case_rng(15, *ir_dims)
    for real in (False, True):
        gen = E.real_channel if real else E.integer_channel
        ir = Channel(*gen(rng, ir_dims[0], nl), lo=ir_dims[1], n=ir_dims[2])
        sol = Channel(*gen(rng, sol_dims[0], nl), lo=sol_dims[1], n=sol_dims[2])
        assert ir.lo > 0 and ir.n < ir.nw and sol.lo > 0 and sol.n < sol.nw
        exact, want = _exact(ir) + _exact(sol), _ints_of(ir) + _ints_of(sol)
        factor = E.chunked_factor(max(ir.n, sol.n))
        got = []
        for form in (0, 1):
            flux, part = integrate(L, form, ir, sol, flux_part=E.integer_rows(rng, nl))
            np.testing.assert_array_equal(part, flux[0], err_msg="form %d: flux_part is not what flux_n holds" % form)
            for a in range(4):
                if real:
                    _assert_within(test, flux[0, a], exact[a], factor, "form %d row %d" % (form, a))
                else:
                    _assert_int_rows(flux[0, a], want[a], "form %d row %d" % (form, a))
            got.append(flux)
        np.testing.assert_array_equal(got[0], got[1])
    _report(test)


@pytest.mark.parametrize("count", [33, 1025, 5441])
def test_without_solar_the_solar_rows_stay_or_are_put_back(hip_lib, count):
    """do_solar = 0: the solar rows of flux_n stay the last solar call's; on a bin shard flux_n holds REDUCED rows by then
    and this rank's partial solar rows are put back from flux_part.  The solar arrays are NaN: nobody reads them."""
    L, nl = hip_lib, 17
    rng = E.case_rng(16, count)
    ir = Channel(*E.integer_channel(rng, count, nl))
    sol = Channel(*E.integer_channel(rng, count, nl))
    sol.up[:], sol.dn[:] = np.nan, np.nan
    want = _ints_of(ir)
    for form in (0, 1):
        given = E.integer_rows(rng, nl)
        flux, _ = integrate(L, form, ir, sol, do_solar=False, flux_n=given)
        np.testing.assert_array_equal(flux[0, 2:], given[2:], err_msg="form %d: the solar rows did not stay" % form)
        for a in range(2):
            _assert_int_rows(flux[0, a], want[a], "form %d row %d" % (form, a))
        reduced, mine = E.integer_rows(rng, nl), E.integer_rows(rng, nl)
        flux, part = integrate(L, form, ir, sol, do_solar=False, flux_n=reduced, flux_part=mine)
        np.testing.assert_array_equal(flux[0, 2:], mine[2:], err_msg="form %d: the solar rows were not put back" % form)
        np.testing.assert_array_equal(part[2:], mine[2:], err_msg="form %d: flux_part's solar rows changed" % form)
        for a in range(2):
            _assert_int_rows(flux[0, a], want[a], "form %d row %d" % (form, a))
            _assert_int_rows(part[a], want[a], "form %d flux_part row %d" % (form, a))


@pytest.mark.parametrize("count", [33, 1025])
def test_three_columns_in_one_grid(hip_lib, count):
    """form 0 with ncol = 3 (a column batch's chunk: gridDim.z), the columns' arrays and rows a stride apart with NaN between"""
    L, test = hip_lib, "three columns, %d bins" % count
    for nl in (16, 33):
        ir, sol = _int_channels((17, count, nl), nl, count, count + 3, ncol=3)
        flux, _ = integrate(L, 0, ir, sol, spec_pad=7, flux_pad=5)
        for c in range(3):
            want = _ints_of(ir, c) + _ints_of(sol, c)
            for a in range(4):
                _assert_int_rows(flux[c, a], want[a], "column %d row %d" % (c, a))
    nl = 17
    ir, sol = _real_channels((18, count), nl, count, count + 3, ncol=3)
    flux, _ = integrate(L, 0, ir, sol, spec_pad=7, flux_pad=5)
    factor = E.chunked_factor(count + 3)
    for c in range(3):
        exact = _exact(ir, c) + _exact(sol, c)
        for a in range(4):
            _assert_within(test, flux[c, a], exact[a], factor, "column %d row %d" % (c, a))
        one = integrate(L, 0, Channel(ir.freq, np.stack([ir.up[c:c + 1], ir.dn[c:c + 1]], axis=1)),
                        Channel(sol.freq, np.stack([sol.up[c:c + 1], sol.dn[c:c + 1]], axis=1)))[0]
        np.testing.assert_array_equal(flux[c], one[0], err_msg="column %d differs from its own call" % c)
    _report(test)


def test_the_hook_refuses_what_the_kernels_do_not_cover(hip_lib):
    """the two-launch pair and flux_part are one column's; so is do_solar = 0 (integrate_block keeps or puts back the solar
    rows of the first column's flux_n whatever the column: a column batch always computes them)"""
    ir, sol = _int_channels((22,), 17, 40, 40, ncol=3)

    def refused(**kw):
        ncol, _, nl = ir.up.shape
        flux, err = np.zeros((ncol, 4, nl)), C.create_string_buffer(1025)
        part = kw.get("part")
        hip_lib.clima_test_integrate(_i(kw.get("form", 0)), _i(nl - 1), _i(ncol), _i(40 * nl), _i(4 * nl), ir.dims(), _p(ir.freq),
                                     sol.dims(), _p(sol.freq), _p(ir.up), _p(ir.dn), _p(sol.up), _p(sol.dn), _i(kw.get("do_solar", 1)),
                                     _p(flux), None if part is None else _p(part), _i(0), None, err)
        assert np.all(flux == 0.0)
        return err.value.decode()

    assert "do_solar = 0 takes one column" in refused(do_solar=0)
    assert "the two-launch form takes one column" in refused(form=1)
    assert "flux_part belongs to one column" in refused(part=np.zeros((4, 17)))


# ------------------------------------------------------------------ hook level: the batch pair (form 2)
SENTINEL = -12345.0


def _hold_batch(test, L, ir, flux_n, col0, real):
    ncol, _, nl = ir.up.shape
    out = integrate_batch(L, ir, flux_n, col0, np.full((3, col0 + ncol, nl), SENTINEL), spec_pad=3)
    assert np.all(out[:, :col0] == SENTINEL), "rows in front of col0 were written"
    factor = E.chunked_factor(ir.n)
    sol = [E.given_rows(flux_n[2]), E.given_rows(flux_n[3])]
    for c in range(ncol):
        got = out[:, col0 + c]
        if real:
            exact = _exact(ir, c)
            for a in range(2):
                _assert_within(test, got[a], exact[a], factor, "col0 %d column %d row %d" % (col0, c, a))
            _assert_within(test, got[2], E.exact_f_total(exact[0], exact[1], *sol), factor + 3, "col0 %d column %d f_total" % (col0, c))
            # ... and f_total is f_total_level of the rows beside it, bit for bit (clima_radtran.f90:287)
            np.testing.assert_array_equal(got[2], (flux_n[3] - flux_n[2]) + (got[1] - got[0]))
        else:
            want = _ints_of(ir, c)
            for a in range(2):
                _assert_int_rows(got[a], want[a], "col0 %d column %d row %d" % (col0, c, a))
            total = [(int(sd) - int(su)) + (d - u) for u, d, su, sd in zip(want[0], want[1], flux_n[2].tolist(), flux_n[3].tolist())]
            _assert_int_rows(got[2], total, "col0 %d column %d f_total" % (col0, c))
    return out


@pytest.mark.parametrize("ncol", [1, 3])
@pytest.mark.parametrize("count", E.BATCH_COUNTS)
def test_batch_pair(hip_lib, count, ncol):
    """k_integrate_partial_b / k_integrate_final_b: the chunk sums are added in groups of eight (256 bins)"""
    test = "batch pair, %d bins x %d columns" % (count, ncol)
    for nl in (2, 17):
        rng = E.case_rng(19, count, ncol, nl)
        ir = Channel(*E.integer_channel(rng, count, nl, ncol))
        for col0 in (0, 2):
            _hold_batch(test, hip_lib, ir, E.integer_rows(rng, nl), col0, real=False)
    rng = E.case_rng(20, count, ncol)
    ir = Channel(*E.real_channel(rng, count, 17, ncol))
    _hold_batch(test, hip_lib, ir, rng.uniform(0.5e15, 1.5e15, size=(4, 17)), 2, real=True)
    _report(test)


def test_batch_pair_on_a_shard_without_ir_bins_beside_one_with(hip_lib):
    """a rank whose bin shard holds solar bins only: ir_n = 0, one empty chunk, rows of 0.0 and f_total from the solar rows
    alone; its neighbour owns every IR bin; a third split shows the two add up to the whole"""
    nl, ncol, nw = 17, 3, 300
    rng = E.case_rng(21)
    freq, arrays = E.integer_channel(rng, nw, nl, ncol)
    flux_n = E.integer_rows(rng, nl)
    outs = {}
    for lo, n in ((0, 0), (0, nw), (nw, 0), (0, 257), (257, 43)):
        ir = Channel(freq, arrays, lo=lo, n=n)
        outs[lo, n] = _hold_batch("empty shard", hip_lib, ir, flux_n, 1, real=False)[:, 1:]
    for key in ((0, 0), (nw, 0)):
        assert np.all(outs[key][:2] == 0.0) and np.all(outs[key][2] == (flux_n[3] - flux_n[2])[None, :])
    np.testing.assert_array_equal(outs[0, 257][:2] + outs[257, 43][:2], outs[0, nw][:2])


# ------------------------------------------------------------------ handle level
# Handles of E.HANDLE_BINS bins in both channels (exact_bin_sums.handle_tables), one zenith angle, albedo 0.3, at two
# layer counts: 16 layers (17 levels: two level groups), where every level is held, and 70 layers -- at most 64 layers
# nothing is fused, every prep pass clears and a column batch runs one call per column whatever the bin count, so the
# merged launch (k_prep_integrate) and the one-launch batch are reached at 70 only (the fused half-wave grid; 71 levels:
# five level groups), where the first and last level of every group are held.
NZ_FUSED = E.HANDLE_NZ_FUSED


def _levels_held(nz, whole=False):
    nl = nz + 1
    if whole or nl <= 2 * E.INT_LV + 1:
        return list(range(nl))
    return sorted({i for g in range(0, nl, E.INT_LV) for i in (g, min(g + E.INT_LV - 1, nl - 1))})


_made = {}


def _tables(nbins):
    if ("t", nbins) not in _made:
        _made["t", nbins] = E.handle_tables(nbins)
    return _made["t", nbins]


def _columns(nz):
    if ("c", nz) not in _made:
        _made["c", nz] = E.handle_columns(3, nz)
    return _made["c", nz]


def _handle(hip_lib, nbins, nz=E.HANDLE_NZ):
    from clima_amd.radtran import Radtran
    r = Radtran(_tables(nbins), nz, 1, 0.3)
    assert len(r.ir.freq) - 1 == len(r.sol.freq) - 1 == nbins
    return r


def _plan(L, nz, nbins, batch):
    """the library's plan for a call (a batch's chunk of three columns) on such a handle, and whether it integrates in one launch"""
    import launch_forms as LF
    return LF.hook_plan(L, nz=nz, ng=8, nzen=1, n_ir=nbins, n_sol=nbins, op_n=nbins, nsrc=nz, ncol=3 if batch else 1, batch=batch,
                        ir_batch=0, rebin_mode=0, cust_on=0, compute_opacity=1, all_pairs=0, fused=1, allow_fused=1, ts_block_mode=0,
                        no_half=0, coop_items=0 if batch else LF.DEFAULT_COOP_ITEMS, force_slots=0, nbins=nbins)


def _state(r):
    """the four level rows, f_total and the four per-bin arrays [bins][levels] of the handle's last call"""
    s = r.spectra_all()
    rows = [np.array(x) for x in (r.wrk_ir.fup_n, r.wrk_ir.fdn_n, r.wrk_sol.fup_n, r.wrk_sol.fdn_n, r.f_total)]
    spec = [np.ascontiguousarray(s[k].T) for k in ("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a")]
    return rows, spec


def _hold_rows(test, rows, spec, freqs, levels, ranges=None, channels=("ir", "sol"), total=True, what=""):
    """rows [ir up, ir dn, sol up, sol dn, f_total] (levels) against the exact sums of spec (the four arrays [bins][levels])
    over `ranges` = ((ir_lo, ir_n), (sol_lo, sol_n)) at `levels`; the condition on the inputs first.  -> the exact rows"""
    ranges = ranges or tuple((0, s.shape[0]) for s in spec[::2])
    factor = E.chunked_factor(max(n for _, n in ranges))
    exact = [None] * 4
    for c, name in enumerate(("ir", "sol")):
        if name not in channels:
            continue
        lo, n = ranges[c]
        up, dn = (spec[2 * c + k][:, levels] for k in (0, 1))
        exact[2 * c], exact[2 * c + 1] = E.exact_rows(up, freqs[c], lo, n), E.exact_rows(dn, freqs[c], lo, n)
        share = E.worst_bin_share(up, dn, freqs[c], lo, n, exact[2 * c][0], exact[2 * c + 1][0])
        assert share >= E.MIN_BIN_SHARE, "%s %s: a bin carries %.1e of its rows' sums: change the input" % (what, name, share)
        for k in (0, 1):
            _assert_within(test, np.asarray(rows[2 * c + k])[levels], exact[2 * c + k], factor, "%s %s row %d" % (what, name, k))
    if total and all(e is not None for e in exact):
        _assert_within(test, np.asarray(rows[4])[levels], E.exact_f_total(*exact), factor + 3, what + " f_total")
    return exact


def _freqs(r):
    return np.array(r.ir.freq), np.array(r.sol.freq)


@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_radiate_synchronous(hip_lib, nbins):
    """the rows come through the host's block where the integration is one launch (<= 5440 bins: k_integrate_one stores
    them there itself), by a copy behind the two-launch pair otherwise; then the same call without the solar part"""
    test = "radiate, %d bins" % nbins
    nz = E.HANDLE_NZ
    r = _handle(hip_lib, nbins)
    col = _columns(nz)[0]
    assert _plan(hip_lib, nz, nbins, False)["integrate_one_launch"] == int(E.fits_one_launch(nbins))
    r.radiate(*col.args())
    rows, spec = _state(r)
    levels = _levels_held(nz)
    _hold_rows(test, rows, spec, _freqs(r), levels, what="radiate")
    other = _columns(nz)[1]
    r.radiate(*other.args(), compute_solar=False)
    rows2, spec2 = _state(r)
    _hold_rows(test, rows2, spec2, _freqs(r), levels, channels=("ir",), what="radiate without solar")
    assert not np.array_equal(rows2[0], rows[0])
    np.testing.assert_array_equal(rows2[2], rows[2], err_msg="the solar rows did not stay")
    np.testing.assert_array_equal(rows2[3], rows[3], err_msg="the solar rows did not stay")
    np.testing.assert_array_equal(rows2[4], (rows2[3] - rows2[2]) + (rows2[1] - rows2[0]))
    _report(test)


def _expected_pipeline(L, nz, nbins, n):
    """(overlapped_calls, merged_integrations) of n >= 2 pipelined calls and one synchronize with two calls in flight,
    from the rules alone: a second call goes beside the first only where the integration fits one launch
    (two_in_flight_allowed); a call keeps its integration back only where that holds and its prep pass clears nothing
    (DEFER_FOR_A_MERGE); calls 3 .. n find one in their slot and merge it where prep_integrate_merges' LDS limit allows,
    else launch it alone; the join launches the last two alone."""
    fits, clears = E.fits_one_launch(nbins), _plan(L, nz, nbins, False)["prep_clears"] != 0
    if not fits:
        return 0, (0, 0)
    if clears:
        return n - 1, (0, 0)
    return n - 1, ((n - 2, 2) if E.merges(nbins) else (0, n))


@pytest.mark.parametrize("nz", [E.HANDLE_NZ, NZ_FUSED])
@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_four_pipelined_resident_calls(hip_lib, nbins, nz):
    test = "pipelined, %d bins, %d layers" % (nbins, nz)
    r = _handle(hip_lib, nbins, nz)
    r.calls_in_flight = 2
    A, B = _columns(nz)[:2]
    levels, n = _levels_held(nz, whole=True), 4      # (the only place k_prep_integrate's integration blocks run: every level)
    overlapped, pair = _expected_pipeline(hip_lib, nz, nbins, n)
    if nz == NZ_FUSED:      # the forms meant: merges at 1025 bins, kept back but alone at 3393, neither at 5441
        assert (overlapped, pair) == {1025: (3, (2, 2)), 3393: (3, (0, 4)), 5441: (0, (0, 0))}[nbins]
    got = {}
    for k, order in enumerate(((A, B, A, B), (B, A, B, A))):
        for c in order:
            r.upload_column(*c.args())
            r.radiate_resident()
        r.synchronize()
        assert r.fused_fallbacks == 0
        assert r.overlapped_calls == (k + 1) * overlapped
        assert r.merged_integrations == ((k + 1) * pair[0], (k + 1) * pair[1])
        got[k] = _state(r)
    for k, c in ((0, B), (1, A)):
        r.radiate(*c.args())
        rows, spec = _state(r)
        for a, b in zip(got[k][0] + got[k][1], rows + spec):
            np.testing.assert_array_equal(a, b, err_msg="pipelined call and synchronous call differ")
        _hold_rows(test, got[k][0], got[k][1], _freqs(r), levels, what="last of four, column %s" % "BA"[k])
    _report(test)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("nz", [E.HANDLE_NZ, NZ_FUSED])
@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_column_batch_of_three(hip_lib, nbins, nz, route):
    """one launch per chunk where the chunk's plan is fused and the integration fits one launch (k_integrate_one with
    gridDim.z = 3 on the arena's strides), one call per column otherwise -- the handle then holds the last column's
    optical properties, which a one-launch batch leaves in its arena (Holds::batch_left: opr() is refused)"""
    from clima_amd.radtran import ClimaException
    test = "batch %s, %d bins, %d layers" % (route, nbins, nz)
    r = _handle(hip_lib, nbins, nz)
    cols = _columns(nz)
    levels = _levels_held(nz)
    plan = _plan(hip_lib, nz, nbins, True)
    one_launch = plan["fused_form"] != 0 and E.fits_one_launch(nbins)
    if nz == NZ_FUSED:
        assert one_launch == (nbins != 5441)
    if route == "host":
        _, _, fl, spec = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=levels)
        fl = np.transpose(fl, (2, 1, 0))                                          # (ncol, 5, nl)
    else:
        from test_gpu_batch_device import tensors
        _, _, fl, spec = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, spectra_levels=levels)
        fl = fl.cpu().numpy()
        spec = {k: np.transpose(v.cpu().numpy(), (1, 2, 0)) for k, v in spec.items()}   # (nsel, bins, ncol) like the host's
    if one_launch:
        with pytest.raises(ClimaException, match="needs opacities"):
            r.opr()
    else:
        r.opr()
    freqs = _freqs(r)
    sel = list(range(len(levels)))
    for c in range(3):
        arrays = [np.ascontiguousarray(spec[k][:, :, c].T) for k in ("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a")]   # [bins][nsel]
        _hold_rows(test, [fl[c, a][levels] for a in range(5)], arrays, freqs, sel, what="column %d" % c)
    _report(test)


@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_ir_batch_and_solar_batch_of_three(hip_lib, nbins):
    test = "IR / solar batch, %d bins" % nbins
    nz = E.HANDLE_NZ
    r = _handle(hip_lib, nbins)
    cols = _columns(nz)
    levels = _levels_held(nz)
    freqs = _freqs(r)
    r.radiate(*cols[0].args())
    # radiate_ir_batch hands out no per-bin arrays: every column against the single IR-only call on the same inputs, whose
    # sums are held to the exact ones here, within test_gpu_parity.py::test_batched_shared_opacity_ir_calls' rtol = 1e-11
    Ts = np.array([float(c["T_surface"]) for c in cols])
    T = np.stack([np.asarray(c["T"]) for c in cols], axis=1)
    fup, fdn, ftot = r.radiate_ir_batch(Ts, T)
    for c in range(3):
        w = cols[0].__class__(cols[0])
        w["T"], w["T_surface"] = T[:, c].copy(), Ts[c]
        r.radiate(*w.args(), compute_solar=False, compute_opacity=False)
        rows, spec = _state(r)
        _hold_rows(test, rows, spec, freqs, levels, channels=("ir",), what="IR-only call %d" % c)
        np.testing.assert_allclose(fup[:, c], rows[0], rtol=1e-11)
        # (that test has NO comparison of the downward row with a single call: this one is new here.  The row falls by four
        #  decades towards the top and is held like that test's f_total, on the row's scale -- the shared-matrix batch kernel
        #  splits the solve's arithmetic differently, 6e-13 of the scale here.  What holds the integration are the exact sums
        #  of the single calls above and the hook-level tests of the batch pair.)
        np.testing.assert_allclose(fdn[:, c], rows[1], rtol=1e-11, atol=1e-11 * np.max(np.abs(rows[1])))
        np.testing.assert_allclose(ftot[:, c], rows[4], rtol=1e-11, atol=1e-11 * np.max(np.abs(rows[4])))
    # radiate_solar_batch returns the per-bin arrays it summed at the levels asked for: all of them
    u = np.array([0.35, 0.6, 0.85])
    up_n, dn_n, _, spec = r.radiate_solar_batch(u, spectra_levels=levels, spectra=("fup", "fdn"))
    factor = E.chunked_factor(nbins)
    for c in range(3):
        for got, name in ((up_n, "fup"), (dn_n, "fdn")):
            a = np.ascontiguousarray(spec[name][:, :, c].T)
            _assert_within(test, got[levels, c], E.exact_rows(a, freqs[1]), factor, "solar case %d %s" % (c, name))
        share = E.worst_bin_share(spec["fup"][:, :, c].T, spec["fdn"][:, :, c].T, freqs[1])
        assert share >= E.MIN_BIN_SHARE, share
    _report(test)


@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_ir_spectra_batch_sums(hip_lib, nbins):
    """k_rows_integrate: a product and a sequential add over the n bins: (n + 3) u A"""
    test = "ir_spectra_batch, %d bins" % nbins
    nz = E.HANDLE_NZ
    r = _handle(hip_lib, nbins)
    cols = _columns(nz)
    r.radiate(*cols[0].args())
    Ts = np.array([float(c["T_surface"]) for c in cols])
    T = np.stack([np.asarray(c["T"]) for c in cols], axis=1)
    sel = [-1, 0, 7, 16, -1]
    out = r.ir_spectra_batch(Ts, T, levels=sel, parts=("up", "dn"), fluxes=True)
    freq = _freqs(r)[0]
    for c in range(3):
        up, dn = out["fup"][:, :, c], out["fdn"][:, :, c]              # [bins][nsel]
        exact = E.exact_rows(up, freq), E.exact_rows(dn, freq)
        assert E.worst_bin_share(up, dn, freq, 0, None, exact[0][0], exact[1][0]) >= E.MIN_BIN_SHARE
        _assert_within(test, out["fup_n"][:, c], exact[0], E.sequential_factor(nbins), "column %d up" % c)
        _assert_within(test, out["fdn_n"][:, c], exact[1], E.sequential_factor(nbins), "column %d dn" % c)
    _report(test)


@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_bin_shard_one_of_three(hip_lib, nbins):
    """set_bin_shard(1, 3) without a communicator: the rows are this shard's partial sums over its own bins"""
    test = "bin shard 1 of 3, %d bins" % nbins
    nz = E.HANDLE_NZ
    r = _handle(hip_lib, nbins)
    r.set_bin_shard(1, 3)
    op_lo, op_n, ir_lo, ir_n, sol_lo, sol_n = r.bin_shard()
    assert 0 < ir_lo and 0 < ir_n < nbins and ir_lo + ir_n < nbins and (sol_lo, sol_n) == (ir_lo, ir_n)
    r.radiate(*_columns(nz)[0].args())
    rows, spec = _state(r)
    _hold_rows(test, rows, spec, _freqs(r), _levels_held(nz), ranges=((ir_lo, ir_n), (sol_lo, sol_n)), what="shard")
    _report(test)
