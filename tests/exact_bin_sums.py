"""Exact sums over the bins, fup_n(i) = sum_l fup_a(i,l) * (freq(l) - freq(l+1)) (clima_radtran_radiate.f90:184-192), the
bound a kernel's sum is held to, and the seeded inputs of tests/test_gpu_integration_sums.py.  A helper of the tests, not a
test.  It shares nothing with oracle/ and nothing with the kernels.

The reference is rational arithmetic (`fractions.Fraction`) on the doubles as the numbers they are: no float and no numpy
takes part in a sum.  numpy arrays are containers only (`.tolist()` hands out Python floats, `Fraction(float)` is exact).

  exact_rows(a, freq, lo, n) -> (S, A): lists over the levels of
        S(i) = sum over lo <= l < lo + n of a[l][i] * (freq[l] - freq[l+1])          the exact value
        A(i) = sum over the same l of |a[l][i]| * |freq[l] - freq[l+1]|               what the rounding errors scale with
  exact_f_total(ir_up, ir_dn, sol_up, sol_dn) -> (S, A) of f_total_level's combination (sol_dn - sol_up) + (ir_dn - ir_up)
        (clima_radtran.f90:287), each argument an (S, A) pair of rows (or, for a row that is given, (values, |values|))
  int_rows(a, freq, lo, n) -> the same S in Python integers, for inputs that are integers

The bound.  u = 2^-53.  A kernel forms each width with one rounding, adds a chunk of INT_CHUNK = 32 bins by fma (one
rounding each) and the nchunk chunk sums one after the other (one rounding each): a term passes through at most
1 + INT_CHUNK + nchunk roundings, so  |got - S| <= (INT_CHUNK + nchunk + 3) u A  (the 3 cover the second-order terms).
k_rows_integrate rounds the product and adds the n bins one after the other: (n + 3) u A.  f_total adds three roundings
(two differences and their sum) to rows that each hold their own bound: (k + 3) u A with A the sum of the four rows' A.

The layout constants below are radtran_dev.h's and kernels.hip's; tests/test_exact_bin_sums_host.py reads them out of the
sources and compares."""
import operator
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
INT_CHUNK, INT_LV, INT_CG = 32, 16, 32
ONE_LAUNCH_LDS = 64 * 1024          # integrate_fits_one_launch
MERGE_LDS = 48 * 1024               # prep_integrate_merges: the integration's dynamic LDS and prep_block's axis
PREP_AXIS_MAX = 1024


def chunks(nbins):
    """integrate_chunks"""
    return 1 if nbins <= 0 else (nbins + INT_CHUNK - 1) // INT_CHUNK


def lds_bytes(nchunk):
    """integrate_lds_bytes"""
    return 8 * nchunk * (INT_CHUNK + INT_LV)


def fits_one_launch(nbins):
    """integrate_fits_one_launch of the bins of the larger channel"""
    return lds_bytes(chunks(nbins)) <= ONE_LAUNCH_LDS


def merges(nbins):
    """the LDS condition of prep_integrate_merges"""
    return fits_one_launch(nbins) and lds_bytes(chunks(nbins)) + 8 * PREP_AXIS_MAX <= MERGE_LDS


def chunked_factor(nbins):
    """k of the bound k u A for the chunked kernels summing `nbins` owned bins (of the larger channel: nchunk is its)"""
    return INT_CHUNK + chunks(nbins) + 3


def sequential_factor(nbins):
    """... for k_rows_integrate"""
    return nbins + 3


# ------------------------------------------------------------------ the reference
def _columns(a, lo, n):
    """a [bins][levels] (array or nested lists) -> per level the owned bins' values as Python numbers"""
    a = np.asarray(a)
    assert a.ndim == 2
    return [a[lo:lo + n, i].tolist() for i in range(a.shape[1])]


def _scaled(values):
    """Python floats -> (integers p, power of two q) with values[k] == Fraction(p[k], q) exactly: the Fractions of the
    doubles over their common denominator, so that a sum of products is a sum of Python integers"""
    pq = [x.as_integer_ratio() for x in values]
    q = max([d for _, d in pq] + [1])
    return [n * (q // d) for n, d in pq], q


def exact_widths(freq, lo, n):
    f = [Fraction(x) for x in np.asarray(freq, dtype=np.float64)[lo:lo + n + 1].tolist()]
    return [f[k] - f[k + 1] for k in range(n)]


def exact_rows(a, freq, lo=0, n=None):
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0] - lo if n is None else n
    fp, fq = _scaled(np.asarray(freq, dtype=np.float64)[lo:lo + n + 1].tolist())
    w = [fp[k] - fp[k + 1] for k in range(n)]          # the widths over fq
    aw = [abs(x) for x in w]
    S, A = [], []
    for col in _columns(a, lo, n):
        p, q = _scaled(col)
        S.append(Fraction(sum(map(operator.mul, p, w)), q * fq))
        A.append(Fraction(sum(map(operator.mul, map(abs, p), aw)), q * fq))
    return S, A


def given_rows(values):
    """a row that is an input (the solar rows a batch's f_total is formed with): exact as it stands"""
    v = [Fraction(x) for x in np.asarray(values, dtype=np.float64).tolist()]
    return v, [abs(x) for x in v]


def exact_f_total(ir_up, ir_dn, sol_up, sol_dn):
    S = [(sd - su) + (d - u) for u, d, su, sd in zip(ir_up[0], ir_dn[0], sol_up[0], sol_dn[0])]
    A = [a + b + c + d for a, b, c, d in zip(ir_up[1], ir_dn[1], sol_up[1], sol_dn[1])]
    return S, A


def int_rows(a, freq, lo=0, n=None):
    a = np.asarray(a)
    n = a.shape[0] - lo if n is None else n
    f = [int(x) for x in np.asarray(freq)[lo:lo + n + 1].tolist()]
    w = [f[k] - f[k + 1] for k in range(n)]
    return [sum(map(operator.mul, [int(x) for x in col], w)) for col in _columns(a, lo, n)]


def shares(got, S, A, factor):
    """per level |got - S| / (factor u A) as floats (0 where A is 0 and got is S); a share above 1 breaks the bound"""
    out = []
    for g, s, a in zip(np.asarray(got, dtype=np.float64).tolist(), S, A):
        e = abs(Fraction(g) - s)
        out.append(float(e / (factor * U * a)) if a else (0.0 if e == 0 else float("inf")))
    return out


def share_per_bin(a, freq, lo=0, n=None, S=None):
    """per owned bin, over the levels, the LARGEST |term| / |S|: a bin whose loss no level would show has a small one.
    (A condition on inputs, held to 1e-8: the terms are floats, the sums the exact ones -- `S` where they are at hand.)"""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0] - lo if n is None else n
    if S is None:
        S = exact_rows(a, freq, lo, n)[0]
    f = np.asarray(freq, dtype=np.float64)[lo:lo + n + 1]
    terms = np.abs(a[lo:lo + n] * (f[:-1] - f[1:])[:, None])
    s = np.array([abs(float(x)) for x in S])
    return np.max(terms[:, s > 0] / s[s > 0], axis=1, initial=0.0).tolist()


# ------------------------------------------------------------------ the inputs
INT_VALUE_MAX = 2 ** 20      # spectra in [1, 2^20)
INT_WIDTH_MAX = 2 ** 10      # widths in [1, 2^10]
FREQ_RANGE = (1.0e12, 3.0e15)


def integer_channel(rng, nw, nl, ncol=1):
    """freq [nw+1] descending integers, widths in [1, 2^10]; ncol arrays pairs (up, dn) [nw][nl] of integers in [1, 2^20):
    every product, fma and partial sum of them is an integer below 2^53, so ANY order of summation gives the same bits"""
    width = rng.integers(1, INT_WIDTH_MAX + 1, size=nw)
    freq = np.concatenate([np.cumsum(width[::-1])[::-1], [0]]) + int(rng.integers(1, 1000))
    arrays = rng.integers(1, INT_VALUE_MAX, size=(ncol, 2, nw, nl))
    return freq.astype(np.float64), arrays.astype(np.float64)


def real_channel(rng, nw, nl, ncol=1, signed=False):
    """freq [nw+1] sorted uniform reals of the real grid's magnitude, descending and distinct; spectra uniform in
    [0.5, 1.5], or in [-1, 1] where `signed` (there A is far above |S|)"""
    while True:
        freq = np.sort(rng.uniform(*FREQ_RANGE, size=nw + 1))[::-1].copy()
        if np.all(np.diff(freq) < 0):
            break
    arrays = rng.uniform(-1.0, 1.0, size=(ncol, 2, nw, nl)) if signed else rng.uniform(0.5, 1.5, size=(ncol, 2, nw, nl))
    return freq, arrays


def integer_rows(rng, nl, n=4):
    """level rows of integers (a flux_n or flux_part that is given)"""
    return rng.integers(1, 2 ** 40, size=(n, nl)).astype(np.float64)


# bin counts per channel, each at a constant of the code: a chunk | the first wrap of integrate_block's chunk loop (INT_CG
# chunks of INT_CHUNK bins) | its third pass | the merge's LDS limit (48 KiB with prep_block's axis) | 48 KiB of the
# integration's own dynamic LDS, beyond which k_integrate_one runs on more than a launch gets without asking | the largest
# one-launch count | the two-launch form
COUNTS = (1, 31, 32, 33, 1023, 1024, 1025, 2049, 3392, 3393, 4096, 4097, 5440, 5441, 5600)
LEVELS = (2, 16, 17, 33)             # nz + 1: one level group, its edge, two groups, three
UNEQUAL = ((1025, 40), (40, 5441))   # (IR, solar) bins: nchunk is the larger channel's, the other's later chunks are empty
BATCH_COUNTS = (1, 256, 257, 512, 513, 1025, 5441)   # k_integrate_final_b: edges of its eight-wide loop (8 x 32 bins) and beyond


# the level count a bin count is run with on real inputs (integer inputs run all of LEVELS); 5600 x 33 is the largest case
LEVELS_OF = {1: 2, 31: 16, 32: 17, 33: 33, 1023: 16, 1024: 17, 1025: 33, 2049: 17, 3392: 16, 3393: 17, 4096: 16, 4097: 17, 5440: 16, 5441: 17,
             5600: 33}


def case_rng(*key):
    """the generator of a case: seeded by what names it"""
    return np.random.default_rng([20240607] + [int(k) for k in key])


# ------------------------------------------------------------------ the handles of the entry-point tests
HANDLE_BINS = (1025, 3393, 5441)     # second pass of the chunk loop | above the merge's LDS limit | the two-launch form
HANDLE_NZ = 16                       # 17 levels: two level groups
HANDLE_NZ_FUSED = 70                 # 71 levels: five; more than 64 layers: the fused grid, whose prep pass clears nothing
WINDOW_NM = (5.0e3, 1.0e5)           # 5-100 um: every bin carries weight in both channels (the nominal grid's ends do not)
MIN_BIN_SHARE = 1.0e-8               # of a row's sum, in at least one of the rows compared: a lost bin is 1e6 bounds


def handle_tables(nbins):
    """one k-table species on a grid of `nbins` bins over WINDOW_NM, both channels owning every bin"""
    from clima_amd import synthetic as S
    t = S.make_tables(nw=nbins, nP=2, nT=2, nT_cia=2, nrad=2, k_species=("CO2",), cia_pairs=(), pxs_species=(), particles=(),
                      water_continuum=False, sol_frac=1.0, ir_frac=0.0)
    t.wavl = np.geomspace(*WINDOW_NM, nbins + 1)
    t.sol_wavl, t.ir_wavl = t.wavl.copy(), t.wavl.copy()
    t.photons_sol = S.blackbody_photons(t.sol_wavl)
    return t


def handle_columns(n=3, nz=HANDLE_NZ):
    """the columns of the entry-point tests: [0] and [1] alternate in the pipelined calls, all n make the batches"""
    from clima_amd import synthetic as S
    return S.perturbed_columns(n, nz, seed=41, n_particles=0)


def worst_bin_share(up, dn, freq, lo=0, n=None, S_up=None, S_dn=None):
    """the smallest, over the owned bins, of a bin's largest share of a row's sum in `up` and `dn` ([bins][levels] each)"""
    return min(max(a, b) for a, b in zip(share_per_bin(up, freq, lo, n, S_up), share_per_bin(dn, freq, lo, n, S_dn)))
