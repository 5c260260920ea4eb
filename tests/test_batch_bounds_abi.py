"""The column batches with per-column surface, zenith and stellar scaling (radtran_toa_fluxes_batch_bounds,
radtran_toa_fluxes_batch_bounds_device) as far as they can be held without a GPU: the library exports them and the
pack hooks, the ctypes table declares them with the header's argument counts, the Python methods document `bounds` and
refuse unknown keys and wrong shapes by name before anything is called (the pattern of tests/test_batch_spectra_abi.py).

The argument counts.  Both prototypes are the spectra batches' with five arrays put in front of `nsel`: 20 + 5 and
21 + 5.  They are tied to the spectra batches' counts so that they cannot drift."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NEW = ("radtran_toa_fluxes_batch_bounds", "radtran_toa_fluxes_batch_bounds_device")
HOOKS = ("clima_test_pack_bounds", "clima_test_pack_bounds_host")


def test_library_exports_the_symbols(hip_lib):
    for name in NEW + HOOKS:
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    assert counts["radtran_toa_fluxes_batch_bounds"] == counts["radtran_toa_fluxes_batch_spectra"] + 5 == 25
    assert counts["radtran_toa_fluxes_batch_bounds_device"] == counts["radtran_toa_fluxes_batch_spectra_device"] + 5 == 26
    assert counts["clima_test_pack_bounds"] == counts["clima_test_pack_bounds_host"] == 10
    for name in NEW + HOOKS:
        assert len(lib.SIGNATURES[name]) == counts[name], name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]
    # the batches it extends are declared as before
    assert len(lib.SIGNATURES["radtran_toa_fluxes_batch_spectra"]) == 20
    assert len(lib.SIGNATURES["radtran_toa_fluxes_batch_spectra_device"]) == 21


def test_python_methods_document_the_bounds():
    from clima_amd.radtran import Radtran
    for method in (Radtran.TOA_fluxes_batch, Radtran.TOA_fluxes_batch_tensors):
        assert "`bounds`" in method.__doc__
    for name in Radtran.BOUNDS:      # the five names where the argument is described; the tensors method refers there
        assert name in Radtran.TOA_fluxes_batch.__doc__, name
    assert "as in `TOA_fluxes_batch`" in Radtran.TOA_fluxes_batch_tensors.__doc__.split("`bounds`")[1]


def test_python_keys_and_shapes_are_checked_before_anything_is_called():
    """the five arrays come back in the ABI's order, float64 and C-contiguous, None where not given; an unknown key and a
    wrong shape are refused by name (no handle needed: the method reads BOUNDS alone)"""
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        BOUNDS = Radtran.BOUNDS
    n, dims = 3, (5, 4, 2)       # nw_sol, nw_ir, nzen
    assert Radtran.BOUNDS == ("surface_albedo", "surface_emissivity", "zenith_u", "zenith_weights", "photon_scale_factor")
    got = Radtran._bounds_request(Stub(), {"photon_scale_factor": [1, 2, 3], "surface_albedo": np.ones((3, 5), order="F")}, n, dims)
    assert [a is None for a in got] == [False, True, True, True, False]
    assert got[0].flags.c_contiguous and got[0].dtype == np.float64 and got[4].dtype == np.float64 and got[4].tolist() == [1.0, 2.0, 3.0]
    assert Radtran._bounds_request(Stub(), {}, n, dims) == [None] * 5
    with pytest.raises(ClimaException, match='toa_fluxes_batch_bounds: "albedo" is not one of surface_albedo, surface_emissivity'):
        Radtran._bounds_request(Stub(), {"albedo": np.ones((3, 5))}, n, dims)
    bad = {"surface_albedo": (3, 4), "surface_emissivity": (4, 3), "zenith_u": (3,), "zenith_weights": (2, 3), "photon_scale_factor": (3, 1)}
    want = {"surface_albedo": (3, 5), "surface_emissivity": (3, 4), "zenith_u": (3, 2), "zenith_weights": (3, 2), "photon_scale_factor": (3,)}
    for name, shape in bad.items():
        with pytest.raises(ClimaException, match=re.escape('toa_fluxes_batch_bounds: "%s" has the shape %s, not %s' % (name, shape, want[name]))):
            Radtran._bounds_request(Stub(), {name: np.ones(shape)}, n, dims)
    with pytest.raises(ClimaException, match='"bounds" is not a dict'):
        Radtran._bounds_request(Stub(), [np.ones((3, 5))], n, dims)
    # the device form takes torch tensors as they are, and says so
    with pytest.raises(ClimaException, match='toa_fluxes_batch_bounds_device: "zenith_u" is not a float64 torch tensor'):
        Radtran._bounds_request(Stub(), {"zenith_u": np.ones((3, 2))}, n, dims, tensors=True)


def test_the_bounds_kernels_are_a_code_object_of_their_own_without_scratch_traffic():
    """clima_amd/csrc/kernels_bounds.hip (kernels.hip compiled once more, for the BND instances) holds the 18 + 13 + 2
    BND instances of k_fused, k_twostream_w / _h and k_twostream with k_pack_bounds, and nothing else; kernels.hip's own
    code object, the one tests/test_build_quality.py reads, holds no BND instance.  The BND instances are held to that
    test's bounds: no scratch instruction in the wave forms, at most 16 where the assembly form of the mixing step lives
    (k_fused<0, ...>), none in the other fused grids."""
    from clima_amd import build as B
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    assert "kernels_bounds.hip" in B.SOURCES
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels_bounds.s")
        flags = [f for f in B.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-w", os.path.join(B.CSRC, "kernels_bounds.hip"), "-o", out])
        counts, name = {}, None
        for line in open(out):
            m = re.match(r"^(_ZN5clima\d+k_\w+):", line)       # (the kernels: every one is named k_...)
            if m:
                name = m.group(1)
                counts[name] = 0
            elif name is not None and "scratch_" in line:
                counts[name] += 1
            elif line.startswith(".Lfunc_end"):
                name = None
    bnd = {k: v for k, v in counts.items() if "k_pack_bounds" not in k}
    assert len(counts) == len(bnd) + 1 == 34, sorted(counts)
    assert all(re.search(r"Lb1EEEvNS_", k) for k in bnd), sorted(bnd)
    assert sum("k_fused" in k for k in bnd) == 18 and sum("k_twostream_w" in k for k in bnd) == 8
    assert sum("k_twostream_h" in k for k in bnd) == 5 and sum("k_twostreamI" in k for k in bnd) == 2
    wave = {k: v for k, v in bnd.items() if re.search("k_twostream_w|k_twostream_h", k)}
    assert not any(wave.values()), wave
    assert counts[[k for k in counts if "k_pack_bounds" in k][0]] == 0
    for k, v in bnd.items():
        if "k_fused" in k:
            assert v <= (16 if "k_fusedILi0E" in k else 0), (k, v)
    # ... and the first compilation holds none of them
    main = build_inspect.scratch_counts()
    assert not [k for k in main if "k_pack_bounds" in k or re.search(r"k_(fused|twostream_w|twostream_h)I.*Lb1EEEvNS_", k)]
