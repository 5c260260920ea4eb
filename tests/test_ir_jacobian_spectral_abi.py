"""radtran_ir_jacobian_spectral_rows as far as it can be held without a GPU: the library exports the new symbols, the ctypes
table declares them with the header's argument counts, the Python method refuses wrong shapes, unknown parts and levels
outside -(nz+1)..nz by name before anything is called, both kernels of ir_adjoint.inc compile without scratch traffic, and
the file is one of the build's dependencies."""
import re

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NEW = ("radtran_ir_jacobian_spectral_rows", "clima_test_ir_adjoint")
KERNELS = ("k_adjoint_rows", "k_adjoint_sum")


def test_library_exports_the_symbols(hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    assert [counts[k] for k in NEW] == [12, 12]
    for name in NEW:
        assert len(lib.SIGNATURES[name]) == counts[name], name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]


def test_python_shapes_parts_and_levels_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_JACOBIAN_SPECTRAL_PARTS = Radtran.IR_JACOBIAN_SPECTRAL_PARTS
    nz = 10
    req = lambda *a: Radtran._ir_jacobian_spectral_request(Stub(), nz, *a)   # noqa: E731
    assert Radtran.IR_JACOBIAN_SPECTRAL_PARTS == ("up", "dn")
    T = np.linspace(280.0, 200.0, nz)
    Ts, Tc, rows, names = req(288.0, T, (-1,), ("up",))
    assert Ts.shape == (1,) and Tc.dtype == np.float64 and rows.dtype == np.int32 and rows.tolist() == [11] and names == ("up",)
    Ts, Tc, rows, names = req([288.0], T.tolist(), [10, 0, -11, -1, 5, 10], ("dn", "up"))
    assert rows.tolist() == [11, 1, 1, 11, 6, 11] and names == ("up", "dn")
    rows, names = req(288.0, T, 3, "dn")[2:]       # a scalar level, a single name
    assert rows.tolist() == [4] and names == ("dn",)
    with pytest.raises(ClimaException, match=re.escape('ir_jacobian_spectral: "T" has the shape (9,), not (10,)')):
        req(288.0, T[:9], (-1,), ("up",))
    with pytest.raises(ClimaException, match=re.escape('ir_jacobian_spectral: "T" has the shape (10, 1), not (10,)')):
        req(288.0, T[:, None], (-1,), ("up",))
    with pytest.raises(ClimaException, match=re.escape('ir_jacobian_spectral: "T_surface" has the shape (2,), not a scalar')):
        req([288.0, 289.0], T, (-1,), ("up",))
    with pytest.raises(ClimaException, match='ir_jacobian_spectral: "total" is not one of up, dn'):
        req(288.0, T, (-1,), ("up", "total"))
    with pytest.raises(ClimaException, match='"parts" names none of up, dn'):
        req(288.0, T, (-1,), ())
    with pytest.raises(ClimaException, match=r"levels\[1\] = 11 is outside -11\.\.10"):
        req(288.0, T, [0, 11], ("up",))
    with pytest.raises(ClimaException, match=r"levels\[0\] = -12 is outside -11\.\.10"):
        req(288.0, T, [-12], ("up",))
    for bad in ([0.5], [], [[0, 1]]):
        with pytest.raises(ClimaException, match='"levels" is not a non-empty list of integer level indices'):
            req(288.0, T, bad, ("up",))
    assert "radtran_ir_jacobian_spectral_rows" in Radtran.ir_jacobian_spectral.__doc__


def test_both_kernels_compile_without_scratch_traffic():
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = {k: v for k, v in build_inspect.scratch_counts().items() if "k_adjoint" in k}
    assert sorted(re.search(r"k_adjoint_[a-z]+", k).group(0) for k in counts) == sorted(KERNELS), counts
    assert not any(counts.values()), counts


def test_the_file_is_a_dependency_of_the_build():
    from clima_amd import build as B
    assert "ir_adjoint.inc" in B.DEPS
