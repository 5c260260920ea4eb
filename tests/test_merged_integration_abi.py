"""The deferred frequency integration's C surface, without a device: the new entry points are declared, exported and in
the Python signature table, and the eligibility rule (clima_test_defer_allowed: the function the library itself asks)
holds what include/clima_radtran_hip.h says of it."""
import ctypes as C
import itertools
import re

import build_inspect

NEW = ("radtran_defer_integration_set", "radtran_defer_integration_get", "radtran_merged_integrations_get",
       "clima_test_defer_allowed")


def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from clima_amd import lib
    text = build_inspect.header_text()
    for n in NEW:
        assert re.search(r"\bvoid\s+%s\s*\(" % n, text), "%s is not declared" % n
        assert hasattr(hip_lib, n), "library does not export %s" % n
        assert n in lib.SIGNATURES


def test_switch_defaults_on_and_counters_start_at_zero(hip_lib):
    L = hip_lib
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    v, m, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    L.radtran_defer_integration_get(h, C.byref(v))
    assert v.value == 1
    L.radtran_defer_integration_set(h, C.byref(C.c_int(0)))
    L.radtran_defer_integration_get(h, C.byref(v))
    assert v.value == 0
    L.radtran_merged_integrations_get(h, C.byref(m), C.byref(s))
    assert (m.value, s.value) == (0, 0)
    L.deallocate_radtran(h)
    L.radtran_defer_integration_get(None, C.byref(v))      # a null handle: off, nothing counted
    L.radtran_merged_integrations_get(None, C.byref(m), C.byref(s))
    assert (v.value, m.value, s.value) == (0, 0, 0)


def test_eligibility_rule(hip_lib):
    def allowed(switch_on, shard_world, has_comm, profile, capturing, flux_ptr_taken):
        out = C.c_int(-1)
        hip_lib.clima_test_defer_allowed(*[C.byref(C.c_int(int(x))) for x in
                                           (switch_on, shard_world, has_comm, profile, capturing, flux_ptr_taken)], C.byref(out))
        return out.value

    for sw, world, comm, prof, cap, ptr in itertools.product((0, 1), (1, 2, 4), (0, 1), (0, 1, 2), (0, 1), (0, 1)):
        want = sw == 1 and world == 1 and not comm and prof != 1 and not cap and not ptr
        assert allowed(sw, world, comm, prof, cap, ptr) == int(want), (sw, world, comm, prof, cap, ptr)
    assert allowed(1, 1, 0, 2, 0, 0) == 1     # events around the dominant kernel only leave the small kernels free
