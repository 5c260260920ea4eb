"""The column batches with per-bin spectra (radtran_toa_fluxes_batch_spectra, radtran_toa_fluxes_batch_spectra_device)
as far as they can be held without a GPU: the library exports them, the ctypes table declares them with the header's
argument counts, and the Python methods document the new arguments and check the level indices (the pattern of
tests/test_batch_device_abi.py; that k_batch_spectra has no scratch traffic is what tools/scratch_report.py shows).

The argument counts.  Both prototypes are the plain batches' with six arguments put in front of `producer_stream` /
`err`: nsel, spec_level and the four spectrum arrays.  The plain batches have 14 and 15 arguments
(test_batch_device_abi.py asserts the 15), so these have 20 and 21.  The request for them quoted 21 and 22 beside
the very prototypes it spelled out, which count to 20 and 21: the prototypes are what the Fortran binding, the ctypes
table and every caller are written against, so the count asserted here is theirs, and it is tied to the plain
batches' counts so that it cannot drift."""
import re

import pytest

from build_inspect import header_arg_counts

NEW = ("radtran_toa_fluxes_batch_spectra", "radtran_toa_fluxes_batch_spectra_device")


def test_library_exports_both_symbols(hip_lib):
    for name in NEW:
        assert hasattr(hip_lib, name), "library does not export %s" % name


def test_ctypes_table_declares_them_with_the_headers_argument_counts(hip_lib):
    from clima_amd import lib
    counts = header_arg_counts()
    assert counts["radtran_toa_fluxes_batch_spectra"] == counts["radtran_toa_fluxes_batch"] + 6 == 20
    assert counts["radtran_toa_fluxes_batch_spectra_device"] == counts["radtran_toa_fluxes_batch_device"] + 6 == 21
    for name in NEW:
        assert len(lib.SIGNATURES[name]) == counts[name], name
        assert getattr(hip_lib, name).argtypes == lib.SIGNATURES[name]
    # the plain batches are declared as before
    assert len(lib.SIGNATURES["radtran_toa_fluxes_batch"]) == 14 and len(lib.SIGNATURES["radtran_toa_fluxes_batch_device"]) == 15


def test_python_methods_document_the_spectra():
    from clima_amd.radtran import Radtran
    assert "spectra_levels" in Radtran.TOA_fluxes_batch.__doc__
    doc = Radtran.TOA_fluxes_batch_tensors.__doc__
    assert "spectra_levels" in doc and "synchronize()" in doc


def test_python_level_indices_are_checked_before_anything_is_called():
    """numpy-style indices -(nz+1)..nz become the ABI's 1..nz+1; anything else is refused by name (no handle needed:
    the method reads `nz` alone)"""
    from clima_amd.radtran import ClimaException, Radtran

    class Stub:
        nz = 50
        SPECTRA = Radtran.SPECTRA
    levels, names = Radtran._spectra_request(Stub(), [50, 0, 0, 25, -1, -51], ("sol_fup_a", "ir_fup_a"))
    assert levels.tolist() == [51, 1, 1, 26, 51, 1] and names == ("ir_fup_a", "sol_fup_a")
    for bad in (51, -52):
        with pytest.raises(ClimaException, match=re.escape("spectra_levels[1] = %d is outside -51..50" % bad)):
            Radtran._spectra_request(Stub(), [0, bad], Radtran.SPECTRA)
    with pytest.raises(ClimaException, match='"amean" is not one of'):
        Radtran._spectra_request(Stub(), [0], ("amean",))

