"""A pipelined call's integration stays in its call slot for the next call into that slot (include/clima_radtran_hip.h,
radtran_calls_in_flight_set): what that leaves unchanged, without a device.  The rule function keeps its truth table --
`int_pending = 1` still turns it off, only what the library feeds in there has changed (an integration kept back by a
call that was NOT pipelined) -- and the C surface is the one it was: same entry points, same argument counts, same
number of rule inputs."""
import ctypes as C
import re

import build_inspect
from test_two_in_flight_abi import LARGE, RULE_FIELDS, SMALL, _rule

SURFACE = {"radtran_calls_in_flight_set": 2, "radtran_calls_in_flight_get": 2, "radtran_overlapped_calls_get": 2,
           "clima_test_two_in_flight": 3, "radtran_defer_integration_set": 2, "radtran_defer_integration_get": 2,
           "radtran_merged_integrations_get": 3}


def test_a_pending_integration_still_turns_the_rule_off(hip_lib):
    for name, call in SMALL + LARGE:
        for mode in (0, 2):
            assert _rule(hip_lib, call, mode=mode, int_pending=1)[0] == 0, (name, mode)
        assert _rule(hip_lib, call, mode=2, int_pending=0)[0] == 1, name
        assert _rule(hip_lib, call, mode=1, int_pending=0)[0] == 0, name
    for name, call in LARGE:
        assert _rule(hip_lib, call, mode=0, int_pending=0)[0] == 1, name


def test_the_declared_surface_is_unchanged(hip_lib):
    from clima_amd import lib
    text = build_inspect.header_text()
    assert int(re.search(r"#define\s+CLIMA_TWO_IN_FLIGHT_RULE_N\s+(\d+)", text).group(1)) == len(RULE_FIELDS) == 12
    assert RULE_FIELDS.index("int_pending") == 11
    counts = build_inspect.header_arg_counts()
    for n, nargs in SURFACE.items():
        assert counts[n] == nargs, n
        assert hasattr(hip_lib, n) and len(lib.SIGNATURES[n]) == nargs, n
    # nothing new rides along: every prototype of the header is one the Python signature table already knew
    assert set(counts) <= set(lib.SIGNATURES), sorted(set(counts) - set(lib.SIGNATURES))


def test_counters_of_a_bare_handle(hip_lib):
    L = hip_lib
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    m, s, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.radtran_merged_integrations_get(h, C.byref(m), C.byref(s))
    L.radtran_overlapped_calls_get(h, C.byref(n))
    assert (m.value, s.value, n.value) == (0, 0, 0)
    L.deallocate_radtran(h)
