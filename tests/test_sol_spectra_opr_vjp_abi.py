"""radtran_sol_spectra_opr_vjp, its device form and clima_test_sol_opr_sens as far as they can be held without a GPU: the
header declares the symbols and the library exports them, the ctypes table declares them with the header's argument counts,
an unconstructed handle is refused by both forms with nothing written, the Python request checkers refuse wrong shapes,
unknown keys and names and levels outside -(nz+1)..nz by name before anything is called, both kernels of sol_opr_sens.inc
compile without scratch traffic, and the file is one of the build's dependencies.  (The refusals that need a constructed
handle -- every argument, by name and value -- are in test_gpu_sol_opr_sens.py; the stored exact derivatives are held by
test_exact_sol_opr_sens_host.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NAMES = {"radtran_sol_spectra_opr_vjp": 13, "radtran_sol_spectra_opr_vjp_device": 14, "clima_test_sol_opr_sens": 25}
KERNELS = ("k_sol_opr_adjoint", "k_sol_opr_sum_g")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_header_declares_and_library_exports_the_symbols(hip_lib):
    for name in NAMES:
        assert name in header_arg_counts()
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    for name, n in NAMES.items():
        assert counts[name] == n, name
        assert len(lib.SIGNATURES[name]) == n, name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]


def test_an_unconstructed_handle_is_refused_and_nothing_is_written(hip_lib):
    L = hip_lib
    err = C.create_string_buffer(1025)
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    p = lambda a: a.ctypes.data_as(DP)   # noqa: E731
    lv = np.array([1], dtype=np.int32)
    g, out = np.ones(64), np.full(64, 7.0)
    L.radtran_sol_spectra_opr_vjp(h, i(1), lv.ctypes.data_as(IP), p(g), None, None, None, None, p(out), None, None, None, err)
    assert err.value.decode() == "Radtran is not constructed"
    a = lambda x: x.ctypes.data   # noqa: E731  (host addresses: the handle is refused before any array is looked at)
    L.radtran_sol_spectra_opr_vjp_device(h, i(1), lv.ctypes.data_as(IP), a(g), None, None, None, None, a(out), None, None, None, None, err)
    assert err.value.decode() == "Radtran is not constructed"
    assert np.all(out == 7.0)
    L.deallocate_radtran(h)


def test_python_shapes_keys_names_and_levels_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        SOL_SPECTRA_OPR_GRADS = Radtran.SOL_SPECTRA_OPR_GRADS
        SOL_SPECTRA_OPR_WRT = Radtran.SOL_SPECTRA_OPR_WRT
    nz, nw_sol = 10, 7
    req = lambda *a: Radtran._sol_spectra_opr_request(Stub(), nz, nw_sol, *a)   # noqa: E731
    assert Radtran.SOL_SPECTRA_OPR_WRT == ("tau", "w0", "g", "albedo")
    assert Radtran.SOL_SPECTRA_OPR_GRADS == ("fup", "fdn", "amean", "fup_n", "fdn_n")
    rows, g, names = req(dict(fup=np.ones((nw_sol, 2)), amean=np.ones((nw_sol, 2)), fdn_n=np.ones(2)), (-1, 0), ("albedo", "g", "tau"))
    assert rows.dtype == np.int32 and rows.tolist() == [11, 1] and names == ("tau", "g", "albedo")
    assert [a is not None for a in g] == [True, False, True, False, True]
    assert all(a.flags.f_contiguous and a.dtype == np.float64 for a in g if a is not None)
    rows, g, names = req(dict(fup_n=[1.0]), 3, "w0")       # a scalar level, a single name
    assert rows.tolist() == [4] and names == ("w0",) and g[3].shape == (1,)
    who = "sol_spectra_opr_vjp: "
    ok = dict(fup=np.ones((nw_sol, 1)))
    with pytest.raises(ClimaException, match=who + '"opacity" is not one of tau, w0, g, albedo'):
        req(ok, (-1,), ("tau", "opacity"))
    with pytest.raises(ClimaException, match=who + '"wrt" names none of tau, w0, g, albedo'):
        req(ok, (-1,), ())
    with pytest.raises(ClimaException, match=who + r"levels\[1\] = 11 is outside -11\.\.10"):
        req(ok, [0, 11], ("tau",))
    for bad in ([0.5], [], [[0, 1]]):
        with pytest.raises(ClimaException, match=who + '"levels" is not a non-empty list of integer level indices'):
            req(ok, bad, ("tau",))
    with pytest.raises(ClimaException, match=who + '"grads" is not a dict'):
        req(np.ones((nw_sol, 1)), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=who + '"total" is not one of fup, fdn, amean, fup_n, fdn_n'):
        req(dict(ok, total=1.0), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, amean, fup_n, fdn_n'):
        req(dict(fup=None), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=re.escape(who + '"amean" has the shape (7, 2), not (7, 1)')):
        req(dict(amean=np.ones((nw_sol, 2))), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=re.escape(who + '"fdn_n" has the shape (1, 2), not (2,)')):
        req(dict(fdn_n=np.ones((1, 2))), (-1, 0), ("tau",))
    for name in ("sol_spectra_opr_vjp", "sol_spectra_opr_vjp_tensors"):
        assert "radtran_sol_spectra_opr_vjp" in getattr(Radtran, name).__doc__


def test_the_tensor_form_refuses_names_levels_dtype_and_layout_before_anything_is_called():
    import torch
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        SOL_SPECTRA_OPR_GRADS = Radtran.SOL_SPECTRA_OPR_GRADS
        SOL_SPECTRA_OPR_WRT = Radtran.SOL_SPECTRA_OPR_WRT
        nz, nw, ngauss = 10, 12, 4
        _ir_tensor_check = Radtran._ir_tensor_check

        class sol:
            freq = np.zeros(8)
    s = Stub()
    call = lambda *a, **k: Radtran.sol_spectra_opr_vjp_tensors(s, *a, **k)   # noqa: E731
    nw_sol = 7
    ok = dict(fup=torch.zeros((1, nw_sol), dtype=torch.float64))
    who = "sol_spectra_opr_vjp_device: "
    with pytest.raises(ClimaException, match=who + '"opacity" is not one of tau, w0, g, albedo'):
        call(ok, wrt=("opacity",))
    with pytest.raises(ClimaException, match=who + r"levels\[0\] = -12 is outside -11\.\.10"):
        call(ok, levels=[-12])
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, amean, fup_n, fdn_n'):
        call({})
    with pytest.raises(ClimaException, match=who + '"amean" is not a float64 torch tensor'):
        call(dict(amean=torch.zeros((1, nw_sol), dtype=torch.float32)))
    with pytest.raises(ClimaException, match=re.escape(who + '"fup" has the shape (7, 1), not (1, 7)')):
        call(dict(fup=torch.zeros((nw_sol, 1), dtype=torch.float64)))
    with pytest.raises(ClimaException, match=who + '"fup" is not C-contiguous'):
        call(dict(fup=torch.zeros((nw_sol, 2), dtype=torch.float64).t()), levels=(0, -1))


def test_both_kernels_compile_without_scratch_traffic():
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = {k: v for k, v in build_inspect.scratch_counts().items() if "k_sol_opr_" in k}
    assert sorted(re.search(r"k_sol_opr_[a-z_]+", k).group(0) for k in counts) == sorted(KERNELS), counts
    assert not any(counts.values()), "python tools/scratch_report.py: %s" % counts


def test_the_file_is_a_dependency_of_the_build():
    from clima_amd import build as B
    assert "sol_opr_sens.inc" in B.DEPS
    src = open(os.path.join(B.CSRC, "kernels.hip")).read()
    assert src.index('#include "ir_opr_sens.inc"') < src.index('#include "sol_opr_sens.inc"') < src.index('#include "ir_rows_apply.inc"')
    inc = open(os.path.join(B.CSRC, "sol_opr_sens.inc")).read()
    assert "atomicAdd" not in inc and "atomic_add" not in inc      # fixed summation orders
