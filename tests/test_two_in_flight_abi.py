"""Two resident calls in flight: the C surface and the rule, without a device.  The new entry points are declared,
exported and in the Python signature table; the switch defaults to automatic; and the rule (clima_test_two_in_flight:
the function the library itself asks, fed the library's own launch plan) says what include/clima_radtran_hip.h says of it."""
import ctypes as C
import itertools
import re

import build_inspect
import launch_forms as LF

NEW = ("radtran_calls_in_flight_set", "radtran_calls_in_flight_get", "radtran_overlapped_calls_get", "clima_test_two_in_flight")
CUS = 256                          # MI355X: one residency round of the fused grid is 2 waves x 4 SIMDs x 256 = 2 048 waves
RULE_OK = dict(mode=0, switch_on=1, shard_world=1, has_comm=0, profile=0, capturing=0, flux_ptr_taken=0, unjoined=1,
               sampled=0, cus=CUS, fields_dirty=0, int_pending=0)
RULE_FIELDS = tuple(RULE_OK)


def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from clima_amd import lib
    text = build_inspect.header_text()
    for n in NEW:
        assert re.search(r"\bvoid\s+%s\s*\(" % n, text), "%s is not declared" % n
        assert hasattr(hip_lib, n), "library does not export %s" % n
        assert n in lib.SIGNATURES
    assert len(RULE_FIELDS) == int(re.search(r"#define\s+CLIMA_TWO_IN_FLIGHT_RULE_N\s+(\d+)", text).group(1))


def test_switch_defaults_to_automatic_and_counter_starts_at_zero(hip_lib):
    L = hip_lib
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    v, n = C.c_int(-1), C.c_int(-1)
    L.radtran_calls_in_flight_get(h, C.byref(v))
    assert v.value == 0
    for want, given in ((1, 1), (2, 2), (0, 0), (2, 7), (0, -3)):       # clamped to 0..2
        L.radtran_calls_in_flight_set(h, C.byref(C.c_int(given)))
        L.radtran_calls_in_flight_get(h, C.byref(v))
        assert v.value == want
    L.radtran_overlapped_calls_get(h, C.byref(n))
    assert n.value == 0
    L.deallocate_radtran(h)
    L.radtran_calls_in_flight_set(None, C.byref(C.c_int(2)))            # a null handle: nothing set, nothing counted
    L.radtran_calls_in_flight_get(None, C.byref(v))
    L.radtran_overlapped_calls_get(None, C.byref(n))
    assert (v.value, n.value) == (0, 0)


def _call(nz, nw, nzen=4, doubled=False, coop_items=0):
    """a full radiate call on a handle of synthetic.make_tables(nw=nw) (its channels: 60 % IR, 60 % solar bins)"""
    n_ir, n_sol = nw - int(round(0.4 * nw)), int(round(0.6 * nw))
    return dict(nz=nz, ng=8, nzen=nzen, n_ir=n_ir, n_sol=n_sol, op_n=nw, nsrc=nz // 2 if doubled else nz, ncol=1, batch=0,
                ir_batch=0, rebin_mode=0, cust_on=0, compute_opacity=1, all_pairs=int(doubled), fused=1, allow_fused=1,
                ts_block_mode=0, no_half=0, coop_items=coop_items, force_slots=0, nbins=max(n_ir, n_sol))


def _rule(L, call, **rule):
    """(takes the other slot, waves of the grid)"""
    rl = dict(RULE_OK)
    rl.update(rule)
    a = (C.c_int * len(RULE_FIELDS))(*[int(rl[k]) for k in RULE_FIELDS])
    b = (C.c_int * len(LF.IN_FIELDS))(*[int(call[k]) for k in LF.IN_FIELDS])
    out = (C.c_int * 2)(-1, -1)
    L.clima_test_two_in_flight(a, b, out)
    return out[0], out[1]


SMALL = [("nz70 x 100", _call(70, 100)), ("nz230 x 100", _call(230, 100)), ("nz40 x 100", _call(40, 100)),
         ("nz70 x 100, default coop_items", _call(70, 100, coop_items=LF.DEFAULT_COOP_ITEMS))]
LARGE = [("config 2", _call(200, 1000, nzen=8)), ("config 3", _call(200, 1000)), ("config 5", _call(500, 1000, nzen=8)),
         ("102 x 400", _call(102, 400)), ("102 x 400, doubled grid", _call(102, 400, doubled=True))]


def test_grid_waves_of_the_benchmark_shape(hip_lib):
    # 782 opacity tiles + 1 200 half-wave two-stream items, four waves each
    assert _rule(hip_lib, LARGE[0][1]) == (1, 4 * (782 + 1200))


def test_automatic_mode_is_off_for_small_grids(hip_lib):
    for name, call in SMALL:
        on, waves = _rule(hip_lib, call)
        assert on == 0 and 0 < waves <= 8 * CUS, (name, waves)
    for row in LF.ROWS:                               # the 8-bin rows: every launch form, all of them launch-bound
        for kind in ("single0", "single"):
            on, waves = _rule(hip_lib, row.plan_in(kind))
            assert on == 0 and waves <= 8 * CUS, (row, kind, waves)


def test_automatic_mode_is_on_where_the_grid_exceeds_one_residency_round(hip_lib):
    for name, call in LARGE:
        on, waves = _rule(hip_lib, call)
        assert on == 1 and waves > 8 * CUS, (name, waves)
        assert _rule(hip_lib, call, cus=waves // 8 + 1)[0] == 0      # ... and it is the device that decides


def test_modes_one_and_two(hip_lib):
    for name, call in SMALL + LARGE:
        assert _rule(hip_lib, call, mode=1)[0] == 0, name
        assert _rule(hip_lib, call, mode=2)[0] == 1, name


def test_off_whenever_the_call_may_not_keep_its_results_back(hip_lib):
    call = LARGE[0][1]
    for mode in (0, 2):
        for sw, world, comm, prof, cap, ptr in itertools.product((0, 1), (1, 2), (0, 1), (0, 1, 2), (0, 1), (0, 1)):
            want = sw == 1 and world == 1 and not comm and prof != 1 and not cap and not ptr
            got = _rule(hip_lib, call, mode=mode, switch_on=sw, shard_world=world, has_comm=comm, profile=prof, capturing=cap,
                        flux_ptr_taken=ptr)[0]
            assert got == int(want), (mode, sw, world, comm, prof, cap, ptr)


def test_off_after_a_join_and_for_a_timed_launch(hip_lib):
    for mode in (0, 2):
        assert _rule(hip_lib, LARGE[0][1], mode=mode, fields_dirty=1)[0] == 0      # stale fields go up behind a join
        assert _rule(hip_lib, LARGE[0][1], mode=mode, int_pending=1)[0] == 0       # a pending integration reads the current slot
        wide = dict(LARGE[0][1], nbins=200000)                                    # the integration needs the shared partial sums
        assert _rule(hip_lib, wide, mode=mode)[0] == 0
        assert _rule(hip_lib, LARGE[0][1], mode=mode, unjoined=0)[0] == 0
        assert _rule(hip_lib, LARGE[0][1], mode=mode, profile=2, sampled=1)[0] == 0
        assert _rule(hip_lib, LARGE[0][1], mode=mode, profile=2, sampled=0)[0] == 1
