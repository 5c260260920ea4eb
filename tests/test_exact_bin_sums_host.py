"""tests/exact_bin_sums.py held without a GPU: its rational sums against Python-integer sums on the integer inputs and
against plain `Fraction` sums on the real ones, its copies of the integration kernels' layout constants against the
sources, the bin counts of the GPU tests against the thresholds they are named after, the case generators' own conditions
(ranges, order, every sum an exact double), and on the CPU oracle the condition the entry-point tests put on their
handles: every bin's term is at least 1e-8 of a compared row's sum."""
import operator
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import exact_bin_sums as E

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
C_LIGHT_NM = 2.99792458e17


def _source(name):
    return open(os.path.join(ROOT, "clima_amd", "csrc", name)).read()


def test_layout_constants_are_the_sources():
    dev, kern = _source("radtran_dev.h"), _source("kernels.hip")
    assert "constexpr int INT_CHUNK = %d;" % E.INT_CHUNK in dev
    assert "constexpr int INT_LV = %d;" % E.INT_LV in dev
    assert "constexpr int INT_CG = %d;" % E.INT_CG in kern
    assert "constexpr int PREP_AXIS_MAX = %d;" % E.PREP_AXIS_MAX in kern
    assert "return nbins <= 0 ? 1 : (nbins + INT_CHUNK - 1) / INT_CHUNK;" in dev
    assert "return sizeof(double) * (size_t)nchunk * (INT_CHUNK + INT_LV);" in dev
    assert "return integrate_lds_bytes(nchunk) <= 64 * 1024;" in dev and E.ONE_LAUNCH_LDS == 64 * 1024
    assert re.search(r"integrate_lds_bytes\(ip\.nchunk\) \+ sizeof\(double\) \* PREP_AXIS_MAX;", kern)
    assert "integrate_fits_one_launch(ip.nchunk) && lds <= 48 * 1024;" in kern and E.MERGE_LDS == 48 * 1024


def test_bin_counts_sit_on_the_thresholds_they_are_named_after():
    assert [E.chunks(n) for n in (0, 1, 31, 32, 33)] == [1, 1, 1, 1, 2]                       # a chunk
    assert [E.chunks(n) > E.INT_CG for n in (1023, 1024, 1025)] == [False, False, True]       # the loop's second pass
    assert 2 * E.INT_CG < E.chunks(2049) <= 3 * E.INT_CG                                      # ... and third
    assert (E.merges(3392), E.merges(3393)) == (True, False)                                  # the merge's LDS limit
    assert E.lds_bytes(E.chunks(3392)) + 8 * E.PREP_AXIS_MAX <= 48 * 1024 < E.lds_bytes(E.chunks(3393)) + 8 * E.PREP_AXIS_MAX
    assert E.lds_bytes(E.chunks(4096)) == 48 * 1024 < E.lds_bytes(E.chunks(4097))             # k_integrate_one's own 48 KiB
    assert E.lds_bytes(E.chunks(5440)) == 65280 and E.fits_one_launch(5440)
    assert not E.fits_one_launch(5441) and not E.fits_one_launch(5600)
    assert [E.chunks(n) for n in E.BATCH_COUNTS] == [1, 8, 9, 16, 17, 33, 171]                # the eight-wide loop's edges
    for n in (1, 31, 32, 33, 1023, 1024, 1025, 2049, 3392, 3393, 4096, 4097, 5440, 5441, 5600):
        assert n in E.COUNTS and E.LEVELS_OF[n] in E.LEVELS
    assert set(E.LEVELS_OF.values()) == set(E.LEVELS) and E.LEVELS_OF[5600] == 33
    assert E.LEVELS == (2, E.INT_LV, E.INT_LV + 1, 2 * E.INT_LV + 1)
    assert E.UNEQUAL == ((1025, 40), (40, 5441))
    assert E.HANDLE_BINS == (1025, 3393, 5441) and E.HANDLE_NZ + 1 == E.INT_LV + 1
    assert [(E.fits_one_launch(n), E.merges(n)) for n in E.HANDLE_BINS] == [(True, True), (True, False), (False, False)]


def test_bound_factors():
    assert E.chunked_factor(5441) == 32 + 171 + 3
    assert abs(float(E.chunked_factor(5441) * E.U) - 2.29e-14) < 1e-16       # "about 2.3e-14 A at 5441 bins"
    assert E.chunked_factor(1) == 36 and E.sequential_factor(40) == 43


@pytest.mark.parametrize("count", [1, 33, 1025, 5600])
def test_rational_sums_are_the_integer_sums_on_integer_inputs(count):
    rng = E.case_rng(1, count)
    nl = 5
    freq, arrays = E.integer_channel(rng, count, nl)
    a = arrays[0, 0]
    # the generator's own conditions
    assert freq.shape == (count + 1,) and a.shape == (count, nl)
    assert np.all(a == np.floor(a)) and a.min() >= 1 and a.max() < E.INT_VALUE_MAX
    w = freq[:-1] - freq[1:]
    assert np.all(freq == np.floor(freq)) and w.min() >= 1 and w.max() <= E.INT_WIDTH_MAX and freq[-1] >= 1
    assert count * (E.INT_VALUE_MAX - 1) * E.INT_WIDTH_MAX < 2 ** 53      # every partial sum in any order is an exact double
    # plain Python integers, written out
    want = [sum(int(a[l, i]) * (int(freq[l]) - int(freq[l + 1])) for l in range(count)) for i in range(nl)]
    assert E.int_rows(a, freq) == want
    S, A = E.exact_rows(a, freq)
    assert [s.denominator for s in S] == [1] * nl and [int(s) for s in S] == want and A == S
    assert all(float(s) == int(s) for s in S)
    if count > 40:       # an owned range
        lo, n = 7, count - 20
        want = [sum(int(a[l, i]) * (int(freq[l]) - int(freq[l + 1])) for l in range(lo, lo + n)) for i in range(nl)]
        assert E.int_rows(a, freq, lo, n) == want and [int(s) for s in E.exact_rows(a, freq, lo, n)[0]] == want


@pytest.mark.parametrize("signed", [False, True])
def test_rational_sums_are_plain_fraction_sums_on_real_inputs(signed):
    rng = E.case_rng(2, signed)
    count, nl, lo, n = 300, 3, 11, 257
    freq, arrays = E.real_channel(rng, count, nl, signed=signed)
    a = arrays[0, 1]
    assert np.all(np.diff(freq) < 0) and freq.min() >= E.FREQ_RANGE[0] and freq.max() <= E.FREQ_RANGE[1]
    assert (a.min() >= -1.0 and a.max() <= 1.0 and a.min() < 0 < a.max()) if signed else (a.min() >= 0.5 and a.max() <= 1.5)
    w = [Fraction(freq[l]) - Fraction(freq[l + 1]) for l in range(lo, lo + n)]
    assert w == E.exact_widths(freq, lo, n)
    S, A = E.exact_rows(a, freq, lo, n)
    for i in range(nl):
        terms = [Fraction(float(a[lo + k, i])) * w[k] for k in range(n)]
        assert S[i] == sum(terms, Fraction(0)) and A[i] == sum(map(abs, terms), Fraction(0))
    if signed:
        assert all(abs(s) < a_ / 4 for s, a_ in zip(S, A))        # the case the bound on A (not on S) is shown with
    else:
        assert A == S
    # a value one rounding off a sum has a share of the bound that says so
    got = [float(s) for s in S]
    assert max(E.shares(got, S, A, E.chunked_factor(n))) <= 0.5 / E.chunked_factor(n) * 1.0001
    off = [g * (1.0 + 1.0e-9) for g in got]
    assert min(E.shares(off, S, A, E.chunked_factor(n))) > 1.0 or signed


def test_f_total_combination():
    rng = E.case_rng(3)
    rows = [E.given_rows(r) for r in E.integer_rows(rng, 4)]
    S, A = E.exact_f_total(*rows)
    for i in range(4):
        u, d, su, sd = (int(r[0][i]) for r in rows)
        assert S[i] == (sd - su) + (d - u) and A[i] == u + d + su + sd


def test_share_per_bin_sees_a_bin_no_row_would_miss():
    rng = E.case_rng(4)
    freq, arrays = E.real_channel(rng, 50, 3)
    up, dn = arrays[0, 0].copy(), arrays[0, 1].copy()
    assert E.worst_bin_share(up, dn, freq) > 1.0e-6
    up[17], dn[17] = 1.0e-12, 1.0e-12                # a bin whose loss every row would hide
    assert E.worst_bin_share(up, dn, freq) < E.MIN_BIN_SHARE
    dn[17, 2] = 1.0                                  # ... but one row shows it
    assert E.worst_bin_share(up, dn, freq) > 1.0e-6


@pytest.mark.parametrize("nz", [E.HANDLE_NZ, E.HANDLE_NZ_FUSED])
@pytest.mark.parametrize("nbins", E.HANDLE_BINS)
def test_every_bin_of_the_handles_carries_weight_on_the_oracle(O, nbins, nz):
    """The condition of the entry-point tests (they assert it again on the arrays the GPU returns): in each channel every
    bin's term is at least MIN_BIN_SHARE of the exact sum in a row compared, for every column used."""
    t = E.handle_tables(nbins)
    assert len(t.ir_wavl) == len(t.sol_wavl) == nbins + 1 and t.nw == nbins
    freq = C_LIGHT_NM / t.wavl
    worst = {"ir": 1.0, "sol": 1.0}
    for col in E.handle_columns(3, nz):
        ref = O.OracleRadtran(t, nz, 1, 0.3)
        ref.radiate(*col.args())
        for name, w in (("ir", ref.wrk_ir), ("sol", ref.wrk_sol)):
            worst[name] = min(worst[name], E.worst_bin_share(w.fup_a.T, w.fdn_a.T, freq))
    print("\n    %d bins, %d layers: worst bin's largest share of a row's sum: IR %.1e, solar %.1e" % (nbins, nz, worst["ir"], worst["sol"]))
    assert min(worst.values()) >= E.MIN_BIN_SHARE
