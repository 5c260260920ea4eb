"""radtran_ir_spectra_batch as far as it can be held without a GPU: the header declares the symbol and the library exports
it, the ctypes table declares it with the header's 15 arguments, the Fortran module binds the name, the Python request
helper refuses wrong shapes, unknown parts and levels outside -(nz+1)..nz by name before anything is called, an
unconstructed handle is refused, both kernels of ir_rows_apply.inc compile without scratch traffic (and the kernels the
build had before them still show the scratch counts they had), and the file is one of the build's dependencies."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NAME = "radtran_ir_spectra_batch"
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_header_declares_and_library_exports_the_symbol(hip_lib):
    assert NAME in header_arg_counts()
    assert hasattr(hip_lib, NAME), "library does not export %s" % NAME


def test_ctypes_table_declares_it_with_the_headers_argument_count(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    assert counts[NAME] == 15
    assert len(lib.SIGNATURES[NAME]) == 15
    assert getattr(hip_lib, NAME).argtypes == lib.SIGNATURES[NAME]


def test_fortran_module_binds_the_name():
    from clima_amd import build as B
    src = open(os.path.join(B.FORTRAN_DIR, "clima_radtran_hip.f90")).read()
    assert 'bind(c, name="%s")' % NAME in src
    assert re.search(r"procedure\s*::\s*ir_spectra_batch\s*=>\s*Radtran_ir_spectra_batch", src)
    m = re.search(r"subroutine Radtran_ir_spectra_batch\(([^)]*)\)", src)
    assert [a.strip() for a in m.group(1).split(",")] == ["self", "T_surface", "T", "spec_level", "err", "ir_fup_a", "ir_fdn_a",
                                                          "fup_n", "fdn_n", "w_up", "w_dn"]


def test_python_shapes_parts_and_levels_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_SPECTRA_BATCH_PARTS = Radtran.IR_SPECTRA_BATCH_PARTS
    nz, n = 10, 3
    req = lambda *a: Radtran._ir_spectra_batch_request(Stub(), nz, *a)   # noqa: E731
    assert Radtran.IR_SPECTRA_BATCH_PARTS == ("up", "dn")
    T = np.linspace(280.0, 200.0, nz)[:, None] + np.arange(n)[None, :]
    Tsfc = np.array([288.0, 289.0, 290.0])
    Ts, Tc, rows, names = req(Tsfc, T, (-1,), ("up",), False)
    assert Ts.shape == (n,) and Tc.shape == (nz, n) and Tc.flags.f_contiguous and Tc.dtype == np.float64
    assert rows.dtype == np.int32 and rows.tolist() == [11] and names == ("up",)
    Ts, Tc, rows, names = req(Tsfc.tolist(), T.tolist(), [10, 0, -11, -1, 5, 10], ("dn", "up"), True)
    assert rows.tolist() == [11, 1, 1, 11, 6, 11] and names == ("up", "dn")
    Ts, Tc, rows, names = req(288.0, T[:, 0], 3, "dn", False)        # one column as a scalar and a vector, a scalar level
    assert Ts.shape == (1,) and Tc.shape == (nz, 1) and rows.tolist() == [4] and names == ("dn",)
    Ts, Tc, rows, names = req(None, None, (-1,), ("up",), True)      # no columns: the weights alone
    assert Ts.shape == (0,) and Tc.shape == (nz, 0)
    with pytest.raises(ClimaException, match="ir_spectra_batch: no columns and weights=False: nothing is asked for"):
        req(None, None, (-1,), ("up",), False)
    with pytest.raises(ClimaException, match=re.escape('ir_spectra_batch: "T" has the shape (9, 3), not (10, 3)')):
        req(Tsfc, T[:9], (-1,), ("up",), False)
    with pytest.raises(ClimaException, match=re.escape('ir_spectra_batch: "T" has the shape (10, 3), not (10, 2)')):
        req(Tsfc[:2], T, (-1,), ("up",), False)
    with pytest.raises(ClimaException, match=re.escape('ir_spectra_batch: "T_surface" has the shape (3, 1), not (ncol,)')):
        req(Tsfc[:, None], T, (-1,), ("up",), False)
    with pytest.raises(ClimaException, match='ir_spectra_batch: "total" is not one of up, dn'):
        req(Tsfc, T, (-1,), ("up", "total"), False)
    with pytest.raises(ClimaException, match='"parts" names none of up, dn'):
        req(Tsfc, T, (-1,), (), False)
    with pytest.raises(ClimaException, match=r"levels\[1\] = 11 is outside -11\.\.10"):
        req(Tsfc, T, [0, 11], ("up",), False)
    with pytest.raises(ClimaException, match=r"levels\[0\] = -12 is outside -11\.\.10"):
        req(Tsfc, T, [-12], ("up",), False)
    for bad in ([0.5], [], [[0, 1]]):
        with pytest.raises(ClimaException, match='"levels" is not a non-empty list of integer level indices'):
            req(Tsfc, T, bad, ("up",), False)
    assert NAME in Radtran.ir_spectra_batch.__doc__


def test_an_unconstructed_handle_is_refused(hip_lib):
    L = hip_lib
    err = C.create_string_buffer(1025)
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    T, Ts, lv, out = np.full((4, 1), 250.0, order="F"), np.array([280.0]), np.array([1], dtype=np.int32), np.full(64, 7.0)
    L.radtran_ir_spectra_batch(h, i(1), Ts.ctypes.data_as(DP), i(4), i(1), T.ctypes.data_as(DP), i(1), lv.ctypes.data_as(IP),
                               out.ctypes.data_as(DP), None, None, None, None, None, err)
    assert err.value.decode() == "Radtran is not constructed"
    assert np.all(out == 7.0)
    L.deallocate_radtran(h)


def test_both_kernels_compile_without_scratch_and_the_others_keep_their_counts():
    """the assembly with ir_rows_apply.inc and, under -DCLIMA_WITHOUT_IR_ROWS_APPLY (kernels.hip leaves the include out),
    without it: the same kernels otherwise, each with the scratch instructions it had"""
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = build_inspect.scratch_counts()
    new = {k: v for k, v in counts.items() if "k_rows_" in k}
    assert sorted(set(re.search(r"k_rows_[a-z]+", k).group(0) for k in new)) == ["k_rows_apply", "k_rows_integrate"], new
    assert len(new) == 9                                         # k_rows_apply<1|2|4|8, 1|4> and k_rows_integrate
    assert not any(new.values()), new
    without = {k: len(hits) for k, (_, hits) in build_inspect.kernel_scratch(("-DCLIMA_WITHOUT_IR_ROWS_APPLY",)).items()}
    assert not any("k_rows_" in k for k in without)
    assert len(without) >= 100
    assert {k: v for k, v in counts.items() if k not in new} == without, "python tools/scratch_report.py"


def test_the_file_is_a_dependency_of_the_build():
    from clima_amd import build as B
    assert "ir_rows_apply.inc" in B.DEPS
    src = open(os.path.join(B.CSRC, "kernels.hip")).read()
    assert src.index('#include "ir_adjoint.inc"') < src.index('#include "ir_rows_apply.inc"')
