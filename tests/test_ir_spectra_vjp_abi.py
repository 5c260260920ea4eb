"""radtran_ir_spectra_batch_device, radtran_ir_spectra_batch_vjp and radtran_ir_spectra_batch_vjp_device as far as they can
be held without a GPU: the header declares the three symbols and the library exports them, the ctypes table declares them
with the header's argument counts, the Fortran module binds the host gradient, the Python request helpers refuse wrong
shapes, unknown keys and parts by name before anything is called, an unconstructed handle is refused by all three, the
gradient kernel (k_vjp_rows in ir_rows_vjp.inc) compiles without scratch traffic while every other kernel keeps the count it
has without the file (-DCLIMA_WITHOUT_IR_ROWS_VJP), and the file is one of the build's dependencies."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import build_inspect
from build_inspect import header_arg_counts

NAMES = {"radtran_ir_spectra_batch_device": 17, "radtran_ir_spectra_batch_vjp": 16, "radtran_ir_spectra_batch_vjp_device": 17}
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


def test_fortran_module_binds_the_name():
    from clima_amd import build as B
    src = open(os.path.join(B.FORTRAN_DIR, "clima_radtran_hip.f90")).read()
    assert 'bind(c, name="radtran_ir_spectra_batch_vjp")' in src
    assert re.search(r"procedure\s*::\s*ir_spectra_batch_vjp\s*=>\s*Radtran_ir_spectra_batch_vjp", src)
    m = re.search(r"subroutine Radtran_ir_spectra_batch_vjp\(([^)]*)\)", src)
    args = [a.strip() for a in m.group(1).replace("&", "").split(",")]
    assert args == ["self", "T_surface", "T", "grad_T_surface", "grad_T", "err", "w_up", "w_dn", "g_ir_fup_a", "g_ir_fdn_a",
                    "g_fup_n", "g_fdn_n"]


def test_python_shapes_and_keys_are_checked_before_anything_is_called():
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_SPECTRA_VJP_WEIGHTS = Radtran.IR_SPECTRA_VJP_WEIGHTS
        IR_SPECTRA_VJP_GRADS = Radtran.IR_SPECTRA_VJP_GRADS
    nz, n, nw_ir, nsel = 10, 3, 7, 2
    req = lambda *a: Radtran._ir_spectra_vjp_request(Stub(), nz, nw_ir, *a)   # noqa: E731
    assert Radtran.IR_SPECTRA_VJP_WEIGHTS == ("w_up", "w_dn") and Radtran.IR_SPECTRA_VJP_GRADS == ("fup", "fdn", "fup_n", "fdn_n")
    T = np.linspace(280.0, 200.0, nz)[:, None] + np.arange(n)[None, :]
    Tsfc = np.array([288.0, 289.0, 290.0])
    w = dict(w_up=np.ones((nw_ir, nsel, nz + 1)), w_dn=np.ones((nw_ir, nsel, nz + 1)))
    g = dict(fup=np.ones((nw_ir, nsel, n)), fdn_n=np.ones((nsel, n)))
    Ts, Tc, k, ws, gs = req(Tsfc, T, w, g)
    assert Ts.shape == (n,) and Tc.shape == (nz, n) and Tc.flags.f_contiguous and k == nsel
    assert [a is not None for a in ws] == [True, True] and [a is not None for a in gs] == [True, False, False, True]
    assert all(a.flags.f_contiguous and a.dtype == np.float64 for a in ws + gs if a is not None)
    Ts, Tc, k, ws, gs = req(288.0, T[:, 0], dict(w_dn=w["w_dn"]), dict(fdn=np.ones((nw_ir, nsel, 1))))      # one column
    assert Ts.shape == (1,) and Tc.shape == (nz, 1) and ws[0] is None and gs[1].shape == (nw_ir, nsel, 1)
    who = "ir_spectra_vjp: "
    with pytest.raises(ClimaException, match=re.escape(who + '"T" has the shape (9, 3), not (10, 3)')):
        req(Tsfc, T[:9], w, g)
    with pytest.raises(ClimaException, match=re.escape(who + '"T_surface" has the shape (3, 1), not (ncol,)')):
        req(Tsfc[:, None], T, w, g)
    with pytest.raises(ClimaException, match=who + '"w_total" is not one of w_up, w_dn'):
        req(Tsfc, T, dict(w, w_total=1.0), g)
    with pytest.raises(ClimaException, match=who + '"total" is not one of fup, fdn, fup_n, fdn_n'):
        req(Tsfc, T, w, dict(g, total=1.0))
    with pytest.raises(ClimaException, match=who + '"weights" holds none of w_up, w_dn'):
        req(Tsfc, T, {}, g)
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, fup_n, fdn_n'):
        req(Tsfc, T, w, dict(fup=None))
    with pytest.raises(ClimaException, match=who + '"weights" is not a dict'):
        req(Tsfc, T, w["w_up"], g)
    with pytest.raises(ClimaException, match=re.escape(who + '"w_dn" has the shape (7, 2, 10), not (7, nsel, 11)')):
        req(Tsfc, T, dict(w, w_dn=np.ones((nw_ir, nsel, nz))), g)
    with pytest.raises(ClimaException, match=re.escape(who + '"fup" has the shape (7, 2, 4), not (7, 2, 3)')):
        req(Tsfc, T, w, dict(fup=np.ones((nw_ir, nsel, n + 1))))
    with pytest.raises(ClimaException, match=re.escape(who + '"fdn_n" has the shape (3, 2), not (2, 3)')):
        req(Tsfc, T, w, dict(fdn_n=np.ones((n, nsel))))
    with pytest.raises(ClimaException, match=who + '"fdn_n" was given without "w_dn"'):
        req(Tsfc, T, dict(w_up=w["w_up"]), g)
    for name in ("ir_spectra_vjp", "ir_spectra_batch_tensors", "ir_spectra_vjp_tensors", "ir_spectra_torch"):
        assert "radtran_ir_spectra_batch" in getattr(Radtran, name).__doc__ or name == "ir_spectra_torch"


def test_the_tensor_forms_refuse_parts_levels_dtype_and_layout_before_anything_is_called():
    import torch
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        IR_SPECTRA_BATCH_PARTS = Radtran.IR_SPECTRA_BATCH_PARTS
        IR_SPECTRA_VJP_WEIGHTS = Radtran.IR_SPECTRA_VJP_WEIGHTS
        IR_SPECTRA_VJP_GRADS = Radtran.IR_SPECTRA_VJP_GRADS
        nz = 10
        _ir_tensor_check = Radtran._ir_tensor_check

        class ir:
            freq = np.zeros(8)
    s = Stub()
    fwd = lambda *a, **k: Radtran.ir_spectra_batch_tensors(s, *a, **k)   # noqa: E731
    bwd = lambda *a, **k: Radtran.ir_spectra_vjp_tensors(s, *a, **k)     # noqa: E731
    n, nz, nw_ir = 3, 10, 7
    Ts, T = torch.full((n,), 280.0, dtype=torch.float64), torch.full((n, nz), 250.0, dtype=torch.float64)
    who = "ir_spectra_batch_device: "
    with pytest.raises(ClimaException, match=who + '"total" is not one of up, dn'):
        fwd(Ts, T, parts=("total",))
    with pytest.raises(ClimaException, match=who + '"parts" names none of up, dn'):
        fwd(Ts, T, parts=())
    with pytest.raises(ClimaException, match=who + r"levels\[1\] = 11 is outside -11\.\.10"):
        fwd(Ts, T, levels=[0, 11])
    with pytest.raises(ClimaException, match=who + '"T" is not a float64 torch tensor'):
        fwd(Ts, T.float())
    with pytest.raises(ClimaException, match=who + '"T_surface" is not a float64 torch tensor'):
        fwd(Ts.numpy(), T)
    with pytest.raises(ClimaException, match=re.escape(who + '"T" has the shape (10, 3), not (3, 10)')):
        fwd(Ts, T.t().contiguous())
    with pytest.raises(ClimaException, match=who + '"T" is not C-contiguous'):
        fwd(Ts, torch.full((nz, n), 250.0, dtype=torch.float64).t())
    with pytest.raises(ClimaException, match=who + '"weights" lacks "w_up"'):
        fwd(Ts, T, weights=dict(w_dn=torch.zeros((nz + 1, 1, nw_ir), dtype=torch.float64)))
    with pytest.raises(ClimaException, match=re.escape(who + '"w_up" has the shape (11, 2, 7), not (11, 1, 7)')):
        fwd(Ts, T, weights=dict(w_up=torch.zeros((nz + 1, 2, nw_ir), dtype=torch.float64)))
    who = "ir_spectra_batch_vjp_device: "
    w = dict(w_up=torch.zeros((nz + 1, 2, nw_ir), dtype=torch.float64))
    with pytest.raises(ClimaException, match=who + '"grads" holds none of fup, fdn, fup_n, fdn_n'):
        bwd(Ts, T, w, {})
    with pytest.raises(ClimaException, match=who + '"fdn" was given without "w_dn"'):
        bwd(Ts, T, w, dict(fdn=torch.zeros((n, 2, nw_ir), dtype=torch.float64)))
    with pytest.raises(ClimaException, match=who + '"fup" is not a float64 torch tensor'):
        bwd(Ts, T, w, dict(fup=torch.zeros((n, 2, nw_ir), dtype=torch.float32)))
    with pytest.raises(ClimaException, match=who + '"fup_n" is not C-contiguous'):
        bwd(Ts, T, w, dict(fup_n=torch.zeros((2, n), dtype=torch.float64).t()))


def test_an_unconstructed_handle_is_refused(hip_lib):
    L = hip_lib
    err = C.create_string_buffer(1025)
    h = C.c_void_p()
    L.allocate_radtran(C.byref(h))
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    T, Ts, lv = np.full((4, 1), 250.0, order="F"), np.array([280.0]), np.array([1], dtype=np.int32)
    w, g, gT, gTs = np.ones(64 * 5), np.ones(64), np.full(4, 7.0), np.full(1, 7.0)
    p = lambda a: a.ctypes.data_as(DP)   # noqa: E731
    L.radtran_ir_spectra_batch_vjp(h, i(1), p(Ts), i(4), i(1), p(T), i(1), p(w), None, p(g), None, None, None, p(gTs), p(gT), err)
    assert err.value.decode() == "Radtran is not constructed"
    assert np.all(gT == 7.0) and np.all(gTs == 7.0)
    a = lambda x: x.ctypes.data   # noqa: E731  (host addresses: the handle is refused before any array is looked at)
    L.radtran_ir_spectra_batch_vjp_device(h, i(1), a(Ts), i(4), i(1), a(T), i(1), a(w), None, a(g), None, None, None, a(gTs), a(gT),
                                          None, err)
    assert err.value.decode() == "Radtran is not constructed"
    L.radtran_ir_spectra_batch_device(h, i(1), a(Ts), i(4), i(1), a(T), i(1), lv.ctypes.data_as(IP), a(g), None, None, None, None, None,
                                      i(0), None, err)
    assert err.value.decode() == "Radtran is not constructed"
    assert np.all(gT == 7.0) and np.all(g == 1.0)
    L.deallocate_radtran(h)


def test_the_kernel_compiles_without_scratch_and_the_others_keep_their_counts():
    """the assembly with ir_rows_vjp.inc and, under -DCLIMA_WITHOUT_IR_ROWS_VJP (kernels.hip leaves the include out), without
    it: the same kernels otherwise, each with the scratch instructions it had"""
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    counts = build_inspect.scratch_counts()
    new = {k: v for k, v in counts.items() if "k_vjp_rows" in k}
    assert len(new) == 2, new                                    # k_vjp_rows<1|4>
    assert not any(new.values()), new
    without = {k: len(hits) for k, (_, hits) in build_inspect.kernel_scratch(("-DCLIMA_WITHOUT_IR_ROWS_VJP",)).items()}
    assert not any("k_vjp_rows" in k for k in without)
    assert len(without) >= 100
    assert {k: v for k, v in counts.items() if k not in new} == without, "python tools/scratch_report.py"


def test_the_file_is_a_dependency_of_the_build():
    from clima_amd import build as B
    assert "ir_rows_vjp.inc" in B.DEPS
    src = open(os.path.join(B.CSRC, "kernels.hip")).read()
    assert src.index('#include "ir_adjoint.inc"') < src.index('#include "ir_rows_apply.inc"') < src.index('#include "ir_rows_vjp.inc"')
    assert "adjoint_dbdt(" in open(os.path.join(B.CSRC, "ir_rows_vjp.inc")).read()                 # the one dB/dT, not a restatement
    assert open(os.path.join(B.CSRC, "ir_adjoint.inc")).read().count("double adjoint_dbdt(") == 1
