"""radtran_ir_spectra_opr_vjp, its device form and clima_test_ir_opr_sens as far as they can be held without a GPU: the header
declares the symbols and the library exports them, the ctypes table declares them with the header's argument counts, an
unconstructed handle is refused by both forms with nothing written, the Python request checkers refuse wrong shapes,
unknown keys and names and levels outside -(nz+1)..nz by name before anything is called, `grey_sensitivity` gives
hand-computed values (the pinned-w0 cases included), both kernels of ir_opr_sens.inc compile without scratch traffic, the
stored exact derivatives are what the generator gives today, bit for bit, and the file is one of the build's dependencies.
(The refusals that need a constructed handle -- every argument, by name and value -- are in test_gpu_ir_opr_sens.py.)"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NAMES = {"radtran_ir_spectra_opr_vjp": 14, "radtran_ir_spectra_opr_vjp_device": 15, "clima_test_ir_opr_sens": 17}
KERNELS = ("k_opr_adjoint", "k_opr_sum_g")
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
    T, Ts, lv = np.full(4, 250.0), np.array([280.0]), np.array([1], dtype=np.int32)
    g, out = np.ones(64), np.full(64, 7.0)
    L.radtran_ir_spectra_opr_vjp(h, p(Ts), i(4), p(T), i(1), lv.ctypes.data_as(IP), p(g), None, None, None, p(out), None, None, err)
    assert err.value.decode() == "Radtran is not constructed"
    a = lambda x: x.ctypes.data   # noqa: E731  (host addresses: the handle is refused before any array is looked at)
    L.radtran_ir_spectra_opr_vjp_device(h, a(Ts), i(4), a(T), i(1), lv.ctypes.data_as(IP), a(g), None, None, None, a(out), None, None,
                                        None, err)
    assert err.value.decode() == "Radtran is not constructed"
    assert np.all(out == 7.0)
    L.deallocate_radtran(h)


def test_python_shapes_keys_names_and_levels_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_SPECTRA_VJP_GRADS = Radtran.IR_SPECTRA_VJP_GRADS
        IR_SPECTRA_OPR_WRT = Radtran.IR_SPECTRA_OPR_WRT
    nz, nw_ir = 10, 7
    req = lambda *a: Radtran._ir_spectra_opr_request(Stub(), nz, nw_ir, *a)   # noqa: E731
    assert Radtran.IR_SPECTRA_OPR_WRT == ("tau", "w0", "g")
    T = np.linspace(280.0, 200.0, nz)
    Ts, Tc, rows, g, names = req(288.0, T, dict(fup=np.ones((nw_ir, 2)), fdn_n=np.ones(2)), (-1, 0), ("g", "tau"))
    assert Ts.shape == (1,) and Tc.shape == (nz,) and rows.dtype == np.int32 and rows.tolist() == [11, 1] and names == ("tau", "g")
    assert [a is not None for a in g] == [True, False, False, True]
    assert all(a.flags.f_contiguous and a.dtype == np.float64 for a in g if a is not None)
    rows, g, names = req([288.0], T.tolist(), dict(fup_n=[1.0]), 3, "w0")[2:]       # a scalar level, a single name
    assert rows.tolist() == [4] and names == ("w0",) and g[2].shape == (1,)
    who = "ir_spectra_opr_vjp: "
    ok = dict(fup=np.ones((nw_ir, 1)))
    with pytest.raises(ClimaException, match=re.escape(who + '"T" has the shape (9,), not (10,)')):
        req(288.0, T[:9], ok, (-1,), ("tau",))
    with pytest.raises(ClimaException, match=re.escape(who + '"T_surface" has the shape (2,), not a scalar')):
        req([288.0, 289.0], T, ok, (-1,), ("tau",))
    with pytest.raises(ClimaException, match=who + '"opacity" is not one of tau, w0, g'):
        req(288.0, T, ok, (-1,), ("tau", "opacity"))
    with pytest.raises(ClimaException, match=who + '"wrt" names none of tau, w0, g'):
        req(288.0, T, ok, (-1,), ())
    with pytest.raises(ClimaException, match=who + r"levels\[1\] = 11 is outside -11\.\.10"):
        req(288.0, T, ok, [0, 11], ("tau",))
    for bad in ([0.5], [], [[0, 1]]):
        with pytest.raises(ClimaException, match=who + '"levels" is not a non-empty list of integer level indices'):
            req(288.0, T, ok, bad, ("tau",))
    with pytest.raises(ClimaException, match=who + '"grads" is not a dict'):
        req(288.0, T, np.ones((nw_ir, 1)), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=who + '"total" is not one of fup, fdn, fup_n, fdn_n'):
        req(288.0, T, dict(ok, total=1.0), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, fup_n, fdn_n'):
        req(288.0, T, dict(fup=None), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=re.escape(who + '"fup" has the shape (7, 2), not (7, 1)')):
        req(288.0, T, dict(fup=np.ones((nw_ir, 2))), (-1,), ("tau",))
    with pytest.raises(ClimaException, match=re.escape(who + '"fdn_n" has the shape (1, 2), not (2,)')):
        req(288.0, T, dict(fdn_n=np.ones((1, 2))), (-1, 0), ("tau",))
    for name in ("ir_spectra_opr_vjp", "ir_spectra_opr_vjp_tensors"):
        assert "radtran_ir_spectra_opr_vjp" in getattr(Radtran, name).__doc__


def test_the_tensor_form_refuses_names_levels_dtype_and_layout_before_anything_is_called():
    import torch
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_SPECTRA_VJP_GRADS = Radtran.IR_SPECTRA_VJP_GRADS
        IR_SPECTRA_OPR_WRT = Radtran.IR_SPECTRA_OPR_WRT
        nz, nw, ngauss = 10, 12, 4
        _ir_tensor_check = Radtran._ir_tensor_check

        class ir:
            freq = np.zeros(8)
    s = Stub()
    call = lambda *a, **k: Radtran.ir_spectra_opr_vjp_tensors(s, *a, **k)   # noqa: E731
    nz, nw_ir = 10, 7
    Ts, T = torch.full((1,), 280.0, dtype=torch.float64), torch.full((nz,), 250.0, dtype=torch.float64)
    ok = dict(fup=torch.zeros((1, nw_ir), dtype=torch.float64))
    who = "ir_spectra_opr_vjp_device: "
    with pytest.raises(ClimaException, match=who + '"opacity" is not one of tau, w0, g'):
        call(Ts, T, ok, wrt=("opacity",))
    with pytest.raises(ClimaException, match=who + r"levels\[0\] = -12 is outside -11\.\.10"):
        call(Ts, T, ok, levels=[-12])
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, fup_n, fdn_n'):
        call(Ts, T, {})
    with pytest.raises(ClimaException, match=who + '"T" is not a float64 torch tensor'):
        call(Ts, T.float(), ok)
    with pytest.raises(ClimaException, match=re.escape(who + '"T_surface" has the shape (2,), not (1,)')):
        call(torch.full((2,), 280.0, dtype=torch.float64), T, ok)
    with pytest.raises(ClimaException, match=re.escape(who + '"fup" has the shape (7, 1), not (1, 7)')):
        call(Ts, T, dict(fup=torch.zeros((nw_ir, 1), dtype=torch.float64)))
    with pytest.raises(ClimaException, match=who + '"fup" is not C-contiguous'):
        call(Ts, T, dict(fup=torch.zeros((nw_ir, 2), dtype=torch.float64).t()), levels=(0, -1))


def test_grey_sensitivity_against_hand_computed_values():
    from clima_amd.radtran import ClimaException, grey_sensitivity
    tau_min, max_w0 = 1.0e-20, 0.99999
    # (nz, ngauss, nw) = (2, 2, 2): layer 0 ordinary; layer 1, bin 0: g-point 0 at the cap, g-point 1 at tau <= tau_min;
    # layer 1, bin 1: w0 = 0 exactly (free: its derivative in an added scatterer is 1 / tau)
    tau = np.array([[[2.0, 4.0], [0.5, 8.0]], [[1.0, 0.25], [1.0e-20, 0.5]]])
    w0 = np.array([[[0.5, 0.25], [0.125, 0.75]], [[0.99999, 0.0], [0.0, 0.0]]])
    gt = np.array([[[1.0, 2.0], [3.0, 4.0]], [[5.0, 6.0], [7.0, 8.0]]])
    gw = np.array([[[8.0, 16.0], [2.0, 32.0]], [[100.0, 1.0], [100.0, 3.0]]])
    ab, sc = grey_sensitivity((tau, w0, None, None), dict(tau=gt, w0=gw), tau_min, max_w0)
    assert ab.shape == sc.shape == (2, 2)
    # (every number a binary fraction: the sums are exact)
    # layer 0, bin 0: (1 - 8 * 0.5 / 2) + (3 - 2 * 0.125 / 0.5) = -1 + 2.5;   (1 + 8 * 0.5 / 2) + (3 + 2 * 0.875 / 0.5) = 3 + 6.5
    assert ab[0, 0] == 1.5 and sc[0, 0] == 9.5
    # layer 0, bin 1: (2 - 16 * 0.25 / 4) + (4 - 32 * 0.75 / 8) = 1 + 1;   (2 + 16 * 0.75 / 4) + (4 + 32 * 0.25 / 8) = 5 + 5
    assert ab[0, 1] == 2.0 and sc[0, 1] == 10.0
    # layer 1, bin 0: both g-points pinned -> grad_tau alone
    assert ab[1, 0] == 12.0 and sc[1, 0] == 12.0
    # layer 1, bin 1: w0 = 0: absorption leaves w0 at 0, a scatterer raises it by 1 / tau
    assert ab[1, 1] == 14.0 and sc[1, 1] == 10.0 + 14.0
    with pytest.raises(ClimaException, match='grey_sensitivity: "grads" lacks "w0"'):
        grey_sensitivity((tau, w0), dict(tau=gt), tau_min, max_w0)
    with pytest.raises(ClimaException, match='grey_sensitivity: "w0" has the shape'):
        grey_sensitivity((tau, w0), dict(tau=gt, w0=gw[:1]), tau_min, max_w0)


def test_both_kernels_compile_without_scratch_traffic():
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = {k: v for k, v in build_inspect.scratch_counts().items() if "k_opr_" in k}
    assert sorted(re.search(r"k_opr_[a-z_]+", k).group(0) for k in counts) == sorted(KERNELS), counts
    assert not any(counts.values()), "python tools/scratch_report.py: %s" % counts


def test_the_file_is_a_dependency_of_the_build():
    from clima_amd import build as B
    assert "ir_opr_sens.inc" in B.DEPS
    src = open(os.path.join(B.CSRC, "kernels.hip")).read()
    assert src.index('#include "ir_adjoint.inc"') < src.index('#include "ir_opr_sens.inc"') < src.index('#include "ir_rows_apply.inc"')
    inc = open(os.path.join(B.CSRC, "ir_opr_sens.inc")).read()
    assert "atomicAdd" not in inc and "atomic_add" not in inc      # fixed summation orders


def test_the_stored_exact_derivatives_are_what_the_generator_gives():
    """a small column regenerated (mpmath, 80 digits) and held to the stored file bit for bit; the stored file holds every
    column the GPU test runs, with the reference algorithm's error on each"""
    pytest.importorskip("mpmath")
    import ir_opr_sens_cases as K
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import make_exact_ir_opr_sens as G
    E = K.load()
    assert int(E["n"][0]) == K.NCOLUMNS == 2 * len(G.CASES)
    n = 2 * G.CASES.index((3, 0)) + 1                  # nz = 3, variant 0, no hard surface
    c = G.case(3, 0, False, with_ref=False)
    for name, v in c.items():
        assert np.array_equal(E["s%02d_%s" % (n, name)], v), name
    for m in range(K.NCOLUMNS):
        k = "s%02d_" % m
        assert E[k + "e_ref"].shape == (6,) and np.all(np.isfinite(E[k + "e_ref"]))
        assert all(np.all(np.isfinite(E[k + x])) for x in K.NAMES)          # tau = 3e4 included: 0 or tiny, never NaN
