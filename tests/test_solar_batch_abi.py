"""radtran_radiate_solar_batch as far as it can be held without a GPU: the library exports the new symbols, the ctypes table
declares them with the header's argument counts, the Python method refuses wrong shapes and unknown spectrum names by name
before anything is called, every instance of k_twostream_sol_batch compiles without scratch traffic (the bound its sibling
k_twostream_ir_batch has in tests/test_build_quality.py: zero), and the bounds batches' code object holds none of them."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NEW = ("radtran_radiate_solar_batch", "radtran_solar_batch_shared_set", "radtran_solar_batch_shared_get", "clima_test_solar_batch")
MORE = ("clima_test_solar_batch_cases_per_block",)


def test_library_exports_the_symbols(hip_lib):
    for name in NEW + MORE:
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    assert [counts[k] for k in NEW + MORE] == [16, 2, 3, 16, 2]
    for name in NEW + MORE:
        assert len(lib.SIGNATURES[name]) == counts[name], name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]


def test_python_shapes_and_names_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        SOLAR_BATCH_SPECTRA = Radtran.SOLAR_BATCH_SPECTRA
    dims = (10, 5)      # nz, nw_sol
    req = lambda *a, **kw: Radtran._solar_batch_request(Stub(), dims, *a, **kw)   # noqa: E731
    assert Radtran.SOLAR_BATCH_SPECTRA == ("fup", "fdn", "amean")
    # a 1-D zenith_u: one angle of weight 1 per case
    n, nzen, u, w, alb, scale, levels, names = req([0.5, 0.6, 0.7], None, None, None, None, ("fup",))
    assert (n, nzen) == (3, 1) and u.shape == w.shape == (3, 1) and np.all(w == 1.0) and alb is None and scale is None
    assert levels is None and names == ()
    n, nzen, u, w, alb, scale, levels, names = req(np.full((3, 2), 0.5, order="F"), np.ones((3, 2)), np.ones((3, 5)), [1, 2, 3], [-1, 0, 10],
                                                    ("amean", "fup"))
    assert (n, nzen) == (3, 2) and u.flags.c_contiguous and alb.dtype == np.float64 and scale.tolist() == [1.0, 2.0, 3.0]
    assert levels.dtype == np.int32 and levels.tolist() == [11, 1, 11] and names == ("fup", "amean")
    bad = {"zenith_weights": (3, 3), "surface_albedo": (3, 4), "photon_scale_factor": (3, 1)}
    want = {"zenith_weights": (3, 2), "surface_albedo": (3, 5), "photon_scale_factor": (3,)}
    for name, shape in bad.items():
        kw = dict(zenith_weights=np.ones((3, 2)), surface_albedo=None, photon_scale_factor=None)
        kw[name] = np.ones(shape)
        with pytest.raises(ClimaException, match=re.escape('radiate_solar_batch: "%s" has the shape %s, not %s' % (name, shape, want[name]))):
            req(np.full((3, 2), 0.5), spectra_levels=None, spectra=(), **kw)
    with pytest.raises(ClimaException, match='"zenith_u" has the shape'):
        req(np.ones((2, 2, 2)), None, None, None, None, ())
    with pytest.raises(ClimaException, match='"zenith_weights" is required'):
        req(np.ones((2, 2)), None, None, None, None, ())
    with pytest.raises(ClimaException, match='radiate_solar_batch: "sol_fup" is not one of fup, fdn, amean'):
        req([0.5], None, None, None, [0], ("sol_fup",))
    with pytest.raises(ClimaException, match=r"spectra_levels\[1\] = 11 is outside -11\.\.10"):
        req([0.5], None, None, None, [0, 11], ("fup",))
    with pytest.raises(ClimaException, match='"spectra_levels" is not a list of integer level indices'):
        req([0.5], None, None, None, [0.5], ("fup",))
    assert "radtran_radiate_solar_batch" in Radtran.radiate_solar_batch.__doc__


def test_every_instance_compiles_without_scratch_traffic():
    """k_twostream_sol_batch<L, 8> for 1..4 slots, <L, 4> for 1..8: held to the bound of k_twostream_ir_batch, zero"""
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = {k: v for k, v in build_inspect.scratch_counts().items() if "k_twostream_sol_batch" in k}
    inst = sorted(tuple(int(x) for x in re.search(r"k_twostream_sol_batchILi(\d+)ELi(\d+)E", k).groups()) for k in counts)
    assert inst == sorted([(L, 4) for L in range(1, 9)] + [(L, 8) for L in range(1, 5)]), inst
    assert not any(counts.values()), counts


def test_the_bounds_code_object_holds_no_instance():
    from clima_amd import build as B
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    assert "solar_batch.inc" in B.DEPS
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels_bounds.s")
        flags = [f for f in B.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.check_call([B.HIPCC] + flags + ["-S", "--cuda-device-only", "-w", os.path.join(B.CSRC, "kernels_bounds.hip"), "-o", out])
        names = re.findall(r"^(_ZN5clima\d+k_\w+):", open(out).read(), flags=re.M)
    assert len(names) == 34 and not [k for k in names if "sol_batch" in k], names
