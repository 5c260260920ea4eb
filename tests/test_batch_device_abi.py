"""The device-array column batch (radtran_toa_fluxes_batch_device) as far as it can be held without a GPU: the library
exports it and its test hooks, the ctypes table declares them with the header's argument counts, and its two kernels
compile without scratch traffic (the pattern of tests/test_build_quality.py, for kernels that file's list predates)."""
import re

import pytest

import build_inspect
NEW = ("radtran_toa_fluxes_batch_device", "clima_test_pack_columns", "clima_test_pack_columns_host")


def test_library_exports_the_device_batch_and_its_hooks(hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = build_inspect.header_arg_counts()
    assert counts["radtran_toa_fluxes_batch_device"] == 15      # the host batch's 14 + producer_stream
    assert counts["clima_test_pack_columns"] == counts["clima_test_pack_columns_host"] == 13
    for name in NEW:
        assert len(lib.SIGNATURES[name]) == counts[name], name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]


def test_python_mirror_has_the_tensor_entry():
    from clima_amd.radtran import Radtran
    doc = Radtran.TOA_fluxes_batch_tensors.__doc__
    assert "synchronize()" in doc and "fused_fallbacks" in doc


@pytest.fixture(scope="module")
def scratch_counts():
    """scratch instructions per kernel of kernels.hip, from the gfx950 assembly of the build's own flags"""
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    return build_inspect.scratch_counts()


def test_pack_and_finish_kernels_have_no_scratch_traffic(scratch_counts):
    mine = {k: v for k, v in scratch_counts.items() if re.search(r"k_pack_columns|k_batch_finish", k)}
    assert len(mine) == 2, sorted(mine)
    assert not any(mine.values()), "scratch instructions in: %s (python tools/scratch_report.py)" % mine
