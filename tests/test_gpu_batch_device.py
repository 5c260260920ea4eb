"""Column batches out of device memory (radtran_toa_fluxes_batch_device, Radtran.TOA_fluxes_batch_tensors): the
contract is the host batch's result on the same columns BIT FOR BIT -- in every launch form --, the column blocks
k_pack_columns builds are the host's pack_column blocks byte for byte, and what the host batch does behind its
synchronise (the repeat after an expired fused hand-off wait, the opacity error) happens at the next synchronize().

Run as a script (`python tests/test_gpu_batch_device.py child`) it is the child process of
test_every_launch_form_in_a_fresh_process: the launch-form switches are read when a handle is made or per call from the
environment, so they get a process of their own."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NZ, NZEN, ALBEDO = 50, 2, 0.3
SRC_PAIR, SRC_EXACT, SRC_LAYER = 1 << 30, 1 << 29, 0xffff


# ------------------------------------------------------------------ helpers (no GPU work at import)
def stacked(cols, np_):
    """The ABI's arrays (column last = C order with the column first) of a list of columns, as numpy arrays"""
    a = dict(T_surface=np.array([float(c["T_surface"]) for c in cols]),
             T=np.stack([np.asarray(c["T"], dtype=np.float64) for c in cols]),
             P=np.stack([np.asarray(c["P"], dtype=np.float64) for c in cols]),
             densities=np.ascontiguousarray(np.stack([np.asarray(c["densities"], dtype=np.float64).T for c in cols])),
             dz=np.stack([np.asarray(c["dz"], dtype=np.float64) for c in cols]))
    if np_ > 0:
        a["pdensities"] = np.ascontiguousarray(np.stack([np.asarray(c["pdensities"], dtype=np.float64).T for c in cols]))
        a["radii"] = np.ascontiguousarray(np.stack([np.asarray(c["radii"], dtype=np.float64).T for c in cols]))
    return a


def tensors(cols, np_):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in stacked(cols, np_).items()}


def device_batch(r, cols, **kw):
    """(ISR, OLR, fluxes) of the device call as numpy arrays, fluxes in the host batch's (nz+1, 5, ncol) order"""
    isr, olr, fl = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, **kw)
    if kw.get("sync") is False:
        r.synchronize()
    return isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0))


def handle_state(r):
    return np.array(r.f_total), np.array(r.wrk_ir.fup_a), np.array(r.wrk_sol.tau_band)


def assert_same_batch(r, cols, **kw):
    """device call == host call on the same handle, results and the state the handle is left in"""
    want = r.TOA_fluxes_batch(cols, return_fluxes=True)
    want_state = handle_state(r)
    got = device_batch(r, cols, **kw)
    for g, w, name in zip(got, want, ("ISR", "OLR", "fluxes")):
        print("%s: largest |device - host| = %.3e" % (name, float(np.max(np.abs(g - w)))))
        np.testing.assert_array_equal(g, w, err_msg=name)
    for g, w, name in zip(handle_state(r), want_state, ("f_total", "wrk_ir.fup_a", "wrk_sol.tau_band")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return got


def doubled(nz_half, n=1, seed=5):
    """columns on AdiabatClimate's doubled radiative grid (2 nz_half + 2 layers, every pair exact)"""
    from clima_amd import synthetic as S
    from clima_amd.atmosphere import copy_atm_to_radiative_grid
    if n == 1:
        return [S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(nz_half)))]
    return [S.Column(copy_atm_to_radiative_grid(c)) for c in S.perturbed_columns(n, nz_half, seed=seed)]


def pack_both(r, cols):
    """(device blocks, host blocks, col_count) of the two test hooks"""
    a = stacked(cols, r.np)
    n = len(cols)
    dp = C.POINTER(C.c_double)

    def d(x):
        return x.ctypes.data_as(dp) if x is not None else None

    cc = C.c_int()
    args = (C.byref(C.c_int(n)), d(a["T_surface"]), d(a["T"]), d(a["P"]), d(a["densities"]), d(a["dz"]),
            C.byref(C.c_int(1 if r.np > 0 else 0)), d(a.get("pdensities")), d(a.get("radii")))
    r._L.clima_test_pack_columns(r._ptr, *args, None, C.byref(cc), r._err)
    r._check()
    out = []
    for fn in (r._L.clima_test_pack_columns, r._L.clima_test_pack_columns_host):
        b = np.full(n * cc.value, np.nan)
        fn(r._ptr, *args, d(b), C.byref(cc), r._err)
        r._check()
        out.append(b)
    return out[0], out[1], cc.value


def meta_of(blocks, cc, nz, c):
    """(nsrc, source list entries, source of every layer) of column c of host-layout blocks"""
    m = blocks[c * cc:(c + 1) * cc][cc - (nz + 1):].view(np.int32)
    return int(m[0]), m[1:1 + nz], m[1 + nz:1 + 2 * nz]


def pair_table_cases(base):
    """base: one column of exact pairs.  Returns columns and what the pair table of each must say."""
    from clima_amd import synthetic as S
    nz = len(base["T"])

    def copy():
        return S.Column({k: (np.array(v, copy=True, order="K") if isinstance(v, np.ndarray) else v) for k, v in base.items()})

    cols, expect = [copy()], [dict(nsrc=nz // 2, not_exact=(), split=())]
    pa, pb, pc = 0, (nz // 2) // 2, nz // 2 - 1          # three different pairs (nz >= 6)
    c = copy()
    c["T"][2 * pa + 1] *= 1.0 + 5e-13                      # within 1e-12: reused, not exact
    c["T"][2 * pb + 1] *= 1.0 + 2e-12                      # beyond: two source layers
    c["densities"][2 * pc + 1, 1] = np.nextafter(c["densities"][2 * pc + 1, 1], np.inf)   # 1 ulp: reused, not exact
    cols.append(c)
    expect.append(dict(nsrc=nz // 2 + 1, not_exact=(2 * pa, 2 * pc), split=(2 * pb,)))
    return cols, expect


def check_pair_tables(r, cols, expect):
    nz = r.nz
    dev, host, cc = pack_both(r, cols)
    for c, e in enumerate(expect):          # the host's table says what the case was built to say ...
        nsrc, srcl, src = meta_of(host, cc, nz, c)
        assert nsrc == e["nsrc"], (c, nsrc, e)
        ent = {int(x) & SRC_LAYER: int(x) for x in srcl[:nsrc]}
        for j in range(0, nz - 1, 2):
            if j in e["split"]:
                assert not ent[j] & SRC_PAIR and ent[j + 1] == j + 1 and src[j + 1] == j + 1
            elif nz % 2 == 0 and e["nsrc"] < nz:
                assert ent[j] & SRC_PAIR and src[j + 1] == j and bool(ent[j] & SRC_EXACT) == (j not in e["not_exact"]), (c, j)
        assert np.all(srcl[nsrc:] == nz - 1)
    assert dev.tobytes() == host.tobytes()    # ... and the device's blocks are the host's, byte for byte


def close_products(na, nb, dza, dzb, contracted):
    """is_close(nb * dzb, na * dza, 1e-12) in float64 (numpy), every operation rounded on its own -- or, `contracted`,
    with the product nb * dzb fused into the difference: the exact product minus the other column, rounded once"""
    from fractions import Fraction
    na, nb, dza, dzb = (np.float64(x) for x in (na, nb, dza, dzb))
    ca, cb = na * dza, nb * dzb
    diff = np.float64(float(Fraction(float(nb)) * Fraction(float(dzb)) - Fraction(float(ca)))) if contracted else cb - ca
    return bool(np.abs(diff) <= np.abs(np.float64(1.0e-12) * max(np.abs(cb), np.abs(ca))))


def ulps(x, k):
    """the float64 k representable numbers above (below: k < 0) the positive x"""
    return (np.array([x], dtype=np.float64).view(np.int64) + k).view(np.float64)[0]


def rounding_cases(n0, dz, walk=400):
    """Densities (na, nb) of one species in the two layers of a pair of thickness dz for which the decision with rounded
    products differs from the one with a contracted product: the first found of each direction, keyed by what the
    rounded decision -- the reference -- says.  na walks upwards from the column's own density n0; for each, nb is
    bisected to the boundary of the rounded decision above na and the 9 neighbours of the boundary are tried."""
    found = {}
    for t in range(walk):
        na = np.float64(n0) * (1.0 + t / 1024.0 + 1.0e-3)
        lo, hi = na, na * (1.0 + 3.0e-12)
        assert close_products(na, lo, dz, dz, False) and not close_products(na, hi, dz, dz, False)
        while ulps(lo, 1) < hi:
            mid = lo + 0.5 * (hi - lo)
            if close_products(na, mid, dz, dz, False):
                lo = mid
            else:
                hi = mid
        for k in range(-4, 5):
            nb = ulps(lo, k)
            want = close_products(na, nb, dz, dz, False)
            if want != close_products(na, nb, dz, dz, True):
                found.setdefault(want, (float(na), float(nb)))
        if len(found) == 2:
            break
    return found


def child_main():
    """both column sets against the host batch, under whatever launch-form switches the environment carries"""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    tables = S.modern_earth_tables(nw=40)
    r = Radtran(tables, NZ, NZEN, ALBEDO)
    assert_same_batch(r, S.perturbed_columns(9, NZ, seed=3))
    cols = doubled(50, 9)
    r2 = Radtran(tables, len(cols[0]["T"]), NZEN, ALBEDO)
    assert_same_batch(r2, cols)
    assert_same_batch(r2, cols, sync=False)
    assert r.fused_fallbacks == 0 and r2.fused_fallbacks == 0
    print("child ok")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main()
    sys.exit(0)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def nine(small_tables):
    """the handle, the 9 columns of test_column_batch_equals_one_call_per_column and the host batch's results"""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    cols = S.perturbed_columns(9, NZ, seed=3)
    r = Radtran(small_tables, NZ, NZEN, ALBEDO)
    want = r.TOA_fluxes_batch(cols, return_fluxes=True)
    return r, cols, want


def test_device_batch_equals_host_batch_byte_for_byte(nine):
    r, cols, want = nine
    got = assert_same_batch(r, cols)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert r.fused_fallbacks == 0


def test_columns_against_the_oracle(O, small_tables, nine):
    from test_gpu_parity import RTOL_TOA
    r, cols, _ = nine
    isr, olr, _ = device_batch(r, cols)
    o = O.OracleRadtran(small_tables, NZ, NZEN, ALBEDO)
    for c in (0, 4, 8):
        isr_o, olr_o = o.TOA_fluxes(*cols[c].args())
        assert abs(olr[c] - olr_o) <= RTOL_TOA * abs(olr_o) and abs(isr[c] - isr_o) <= RTOL_TOA * abs(isr_o)


def test_doubled_columns_in_one_launch_per_chunk(small_tables):
    """102 layers (AdiabatClimate's 50 doubled): the fused grid covers them, so the batch is one launch of each kernel
    per chunk and nothing is fetched before the enqueue; every pair is exact, so half the layers are sources"""
    from clima_amd.radtran import Radtran
    cols = doubled(50, 9)
    r = Radtran(small_tables, len(cols[0]["T"]), NZEN, ALBEDO)
    assert_same_batch(r, cols)
    assert_same_batch(r, cols[:3], sync=False)      # fewer columns than the arenas hold
    assert r.fused_fallbacks == 0


@pytest.mark.parametrize("env", [{"CLIMA_HIP_BATCH_ONE_LAUNCH": "0"}, {"CLIMA_HIP_BATCH_COLS": "4"}], ids=["per_column", "chunks_of_4"])
def test_every_launch_form_in_a_fresh_process(env):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=e, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0 and "child ok" in p.stdout


@pytest.mark.parametrize("nz_half", [2, 24, 299], ids=["nz6", "nz50", "nz600"])
def test_pair_table_is_built_on_the_device_as_on_the_host(small_tables, nz_half):
    from clima_amd.radtran import Radtran
    base = doubled(nz_half)[0]
    nz = len(base["T"])
    assert nz == 2 * nz_half + 2
    cols, expect = pair_table_cases(base)
    if nz == 600:   # a pair split in the block's second pass (pairs 256..299), behind reused ones of the first
        c = cols[1]
        c["P"][2 * 270 + 1] *= 1.0 + 3e-12
        expect[1] = dict(expect[1], nsrc=expect[1]["nsrc"] + 1, split=expect[1]["split"] + (540,))
    r = Radtran(small_tables, nz, NZEN, ALBEDO)
    check_pair_tables(r, cols, expect)
    if nz == 50:
        assert_same_batch(r, cols)


def test_pair_decision_rounds_the_column_products(small_tables):
    """The columns density * dz of the pair decision are rounded before they are compared, on the host and on the
    device alike: cases, found here in exact arithmetic for the column's own layer thicknesses, whose decision flips
    when a product is fused into the difference -- one that is reused only with rounded products, one that is split
    only with them --, in two different pairs of columns of their own.  The reference is the float64 (numpy) decision."""
    from clima_amd.radtran import Radtran
    base = doubled(2)[0]
    nz, sp = len(base["T"]), 1
    assert nz == 6
    cols, expect = [], []
    for reused, pair in ((True, 0), (False, 2)):
        j = 2 * pair + 1
        assert base["dz"][j] == base["dz"][j - 1]
        found = rounding_cases(base["densities"][j, sp], base["dz"][j])
        print("pair %d, dz %r: rounded and contracted decisions differ at %r" % (pair, float(base["dz"][j]), found))
        assert set(found) == {True, False}, "no case of each direction for this dz"
        na, nb = found[reused]
        c = pair_table_cases(base)[0][0]
        c["densities"][j - 1, sp], c["densities"][j, sp] = na, nb
        cols.append(c)
        expect.append(dict(nsrc=nz // 2, not_exact=(j - 1,), split=()) if reused else dict(nsrc=nz // 2 + 1, not_exact=(), split=(j - 1,)))
    r = Radtran(small_tables, nz, NZEN, ALBEDO)
    check_pair_tables(r, cols, expect)


def test_pair_table_of_an_odd_column_has_no_reuse(small_tables):
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    col = S.modern_earth_column(7)
    col["T"][3] = col["T"][2]
    col["P"][3] = col["P"][2]         # (would be close, were the layer count even)
    r = Radtran(small_tables, 7, NZEN, ALBEDO)
    check_pair_tables(r, [col, S.modern_earth_column(7)], [dict(nsrc=7, not_exact=(), split=())] * 2)


def test_pair_table_with_particle_radii():
    """the handle made from the data directory has particle opacities: the radii take part in the decision"""
    from clima_amd.radtran import Radtran
    from expected_tables import DATADIR_C
    base = doubled(3)[0]
    nz = len(base["T"])
    cols, expect = pair_table_cases(base)
    cols[1]["radii"][3, 0] *= 1.0 + 2e-12             # pair (2, 3): two source layers
    cols[0]["radii"][1, 0] *= 1.0 + 5e-13             # pair (0, 1): reused, not exact
    expect[1] = dict(expect[1], nsrc=expect[1]["nsrc"] + 1, split=expect[1]["split"] + (2,))
    expect[0] = dict(expect[0], not_exact=(0,))
    r = Radtran.from_files(os.path.join(DATADIR_C, "settings.yaml"), os.path.join(DATADIR_C, "star.txt"), 3, 0.2, nz, DATADIR_C)
    assert r.np == 1
    check_pair_tables(r, cols, expect)
    assert_same_batch(r, cols)


def test_expired_handoff_is_repaired_at_synchronize():
    """fused_spins = 0: every hand-off wait that is not satisfied at its first poll expires.  The device call returns
    with the batch enqueued; synchronize() finds the flag and runs the batch again through the separate launches into
    the same tensors -- once.

    What the repaired result is held to.  The existing forced-fallback tests (test_gpu_parity.py,
    test_fused_handoff_timeout_is_reissued_unfused and its neighbours) take a handle with fused_spins at its default
    whose `fused` switch is off -- the separate launches, which is what a repeat runs -- and ask for EQUALITY: so does
    this test, and for equality with the host batch on the same fused_spins = 0 handle (the contract).  The FUSED
    result of the default handle is not that reference: the fused grid and the separate launches differ by rounding
    (measured here on the MI355X: ISR 1.8e-14, OLR 1.9e-13 relative, level rows 6.5e-11 of an
    element), and the suite's bound between those two forms is test_fused_and_separate_launch_forms'
    rtol 1e-11 + 1e-9 of the largest level flux; it is asserted too."""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    tables = S.modern_earth_tables(nw=400)   # enough opacity blocks that some two-stream blocks do wait
    nz = 200
    col = S.modern_earth_column(nz)
    warm = S.Column(col)
    warm["T"] = np.asarray(col["T"]) + 3.0
    cols = [col, warm]
    ref = Radtran(tables, nz, 4, 0.2)        # fused_spins at its default
    want_fused = ref.TOA_fluxes_batch(cols, return_fluxes=True)
    assert ref.fused_fallbacks == 0
    ref.fused = False
    want = ref.TOA_fluxes_batch(cols, return_fluxes=True)
    r = Radtran(tables, nz, 4, 0.2)
    r.fused_spins = 0
    t = tensors(cols, r.np)
    n0 = r.fused_fallbacks
    isr, olr, fl = r.TOA_fluxes_batch_tensors(**t, return_fluxes=True, sync=False)
    assert r.fused_fallbacks == n0           # nothing has been looked at yet
    r.synchronize()
    assert r.fused_fallbacks == n0 + 1
    got = (isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0)))
    names = ("ISR", "OLR", "fluxes")
    for g, w, f, name in zip(got, want, want_fused, names):
        print("%s: largest relative difference to the default handle's fused result %.3e, to its separate launches' %.3e"
              % (name, float(np.max(np.abs(g - f) / np.maximum(np.abs(f), 1e-300))), float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))))
    for g, w, name in zip(got, want, names):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for g, f, name in zip(got, want_fused, names):
        np.testing.assert_allclose(g, f, rtol=1e-11, atol=1e-9 * float(np.max(np.abs(want_fused[2]))), err_msg=name)
    r.synchronize()                          # settled: nothing is repeated twice
    assert r.fused_fallbacks == n0 + 1
    np.testing.assert_array_equal(np.array(r.f_total), want[2][:, 4, -1])
    left = handle_state(r) + r.opr()         # what the repaired device batch left in the handle's own buffers
    n1 = r.fused_fallbacks
    host = r.TOA_fluxes_batch(cols, return_fluxes=True)      # the host batch on this handle repeats itself the same way
    assert r.fused_fallbacks == n1 + 1
    for g, h, name in zip(got, host, names):
        np.testing.assert_array_equal(g, h, err_msg=name)
    # ... and leaves the handle holding the same: the last column's rows, spectra and optical properties
    for g, w, name in zip(handle_state(r) + r.opr(), left, ("f_total", "wrk_ir.fup_a", "wrk_sol.tau_band", "tau", "w0", "g", "tau_band")):
        np.testing.assert_array_equal(g, w, err_msg=name)


OPACITY_FAILED = "Opacity computation failed in one or more wavelength bins."


@pytest.mark.parametrize("form", ["per_column", "one_launch"])
def test_opacity_failure_inside_a_batch(small_tables, form):
    """The middle column of three has particle radii outside the Mie grid (the reference's own ierr path, as in
    test_error_behaviour_matches_reference): the host batch reports it in its own call, the device batch at the next
    synchronize() -- once --, no route mistakes it for an expired hand-off wait, and the handle computes the good
    columns afterwards as a fresh handle does.  50 layers run one call per column, the 102 doubled ones one launch
    per chunk."""
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    good = S.perturbed_columns(3, 50) if form == "per_column" else doubled(50, 3)
    bad = list(good)
    bad[1] = S.Column(good[1])
    bad[1]["radii"] = np.asarray(good[1]["radii"]) * 1e6
    r = Radtran(small_tables, len(good[0]["T"]), NZEN, ALBEDO)
    assert r.np == 1
    n0 = r.fused_fallbacks
    fresh = r.TOA_fluxes_batch(good, return_fluxes=True)
    # host route
    with pytest.raises(ClimaException, match=OPACITY_FAILED):
        r.TOA_fluxes_batch(bad, return_fluxes=True)
    for g, w, name in zip(r.TOA_fluxes_batch(good, return_fluxes=True), fresh, ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    # device route, sync=False: reported at synchronize(), once
    t = tensors(bad, r.np)
    out = r.TOA_fluxes_batch_tensors(**t, return_fluxes=True, sync=False)
    with pytest.raises(ClimaException, match=OPACITY_FAILED):
        r.synchronize()
    r.synchronize()
    del out
    for g, w, name in zip(assert_same_batch(r, good), fresh, ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    # device route, sync=True
    with pytest.raises(ClimaException, match=OPACITY_FAILED):
        r.TOA_fluxes_batch_tensors(**t, return_fluxes=True)
    assert_same_batch(r, good, sync=False)
    assert r.fused_fallbacks == n0


def test_inputs_written_on_another_torch_stream(small_tables):
    """The inputs are produced on a side stream, behind work long enough that a call which ignored the order would
    read the zeros the tensors were made with.  102 layers: the batch is enqueued without a look at the device."""
    import torch
    from clima_amd.radtran import Radtran
    cols = doubled(50, 9)
    r = Radtran(small_tables, len(cols[0]["T"]), NZEN, ALBEDO)
    want = r.TOA_fluxes_batch(cols, return_fluxes=True)
    src = tensors(cols, r.np)
    t = {k: torch.zeros_like(v) for k, v in src.items()}
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            a = (a @ a) * 1e-2
        for k in t:
            t[k].copy_(src[k])
        isr, olr, fl = r.TOA_fluxes_batch_tensors(**t, return_fluxes=True, sync=False)
    r.synchronize()
    np.testing.assert_array_equal(isr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(olr.cpu().numpy(), want[1])
    np.testing.assert_array_equal(np.transpose(fl.cpu().numpy(), (2, 1, 0)), want[2])
    assert r.fused_fallbacks == 0


def test_refusals_leave_the_handle_usable(small_tables, nine):
    import torch
    from clima_amd.radtran import ClimaException, Radtran
    r, cols, want = nine
    t = tensors(cols, r.np)
    host = dict(t, T=torch.from_numpy(stacked(cols, r.np)["T"]))               # NumPy-backed, pageable host memory
    with pytest.raises(ClimaException, match='toa_fluxes_batch_device: "T" is not device memory of this handle\'s device'):
        r.TOA_fluxes_batch_tensors(**host)
    strided = dict(t, T=t["T"].t().contiguous().t())                           # right shape, column-major
    with pytest.raises(ClimaException, match='"T" is not C-contiguous'):
        r.TOA_fluxes_batch_tensors(**strided)
    none = {k: v[:0] for k, v in t.items()}
    with pytest.raises(ClimaException, match='"T" has the wrong input dimension.'):
        r.TOA_fluxes_batch_tensors(**none)
    sharded = Radtran(small_tables, NZ, NZEN, ALBEDO)
    sharded.set_bin_shard(0, 2)
    with pytest.raises(ClimaException, match="toa_fluxes_batch is not available on a bin-sharded handle"):
        sharded.TOA_fluxes_batch_tensors(**t)
    isr, olr = r.TOA_fluxes_batch_tensors(**t)                                 # and a normal call afterwards
    np.testing.assert_array_equal(isr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(olr.cpu().numpy(), want[1])
