"""Per-bin spectra of every column out of the column batches (radtran_toa_fluxes_batch_spectra and its device-array
form; Radtran.TOA_fluxes_batch / TOA_fluxes_batch_tensors with `spectra_levels`).  The rows are COPIES of what the
batch's own kernels left in its buffers, taken before the next chunk (or column) overwrites them, so every comparison
with the rows of a column's own TOA_fluxes call, and of one form with another, is an equality; the only bound is the
rounding bound of test 6, which ties the rows to the level fluxes the same batch integrated out of them.

"own-call rows": wrk_ir.fup_a, wrk_ir.fdn_a, wrk_sol.fup_a, wrk_sol.fdn_a after that column's own TOA_fluxes.

Run as a script (`python tests/test_gpu_batch_spectra.py child`) it is the child process of
test_the_arena_is_reused_in_a_fresh_process: the launch-form switches are read from the environment."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from test_gpu_batch_device import doubled, stacked, tensors  # noqa: E402

NZ, NZEN, ALBEDO = 50, 2, 0.3
NAMES = ("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a")
LEVELS = [NZ, 0, 0, 25]          # the top, the ground, a repeat, an interior level


# ------------------------------------------------------------------ helpers (no GPU work at import)
def own_call_rows(r, cols):
    """name -> (nz+1, nw_channel, ncol): the four spectra of every column's own TOA_fluxes call on `r`, every level"""
    out = {name: [] for name in NAMES}
    for c in cols:
        r.TOA_fluxes(*c.args())
        for name in NAMES:
            out[name].append(np.array(getattr(r.wrk_ir if name.startswith("ir") else r.wrk_sol, name.split("_", 1)[1])))
    return {name: np.stack(v, axis=2) for name, v in out.items()}


def assert_rows_equal(spec, own, levels, what=""):
    assert sorted(spec) == sorted(NAMES)
    for name in NAMES:
        assert spec[name].shape == (len(levels),) + own[name].shape[1:], (name, spec[name].shape)
        np.testing.assert_array_equal(spec[name], own[name][levels], err_msg="%s %s" % (what, name))


def device_spectra(r, cols, levels, sync=True, **kw):
    """the tensor form's results in the host form's layout"""
    isr, olr, fl, spec = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, sync=sync, spectra_levels=levels, **kw)
    if not sync:
        r.synchronize()
    return (isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0)),
            {k: np.transpose(v.cpu().numpy(), (1, 2, 0)) for k, v in spec.items()})


def assert_sum_identity(r, fluxes, spec):
    """Test 6.  `spec` holds every level.  The batch's integration (clima_radtran_radiate.f90:184-192 of the reference)
    sums flux[l] * dnu[l] over the channel's bins; numpy sums the same nw products in another order.  Two orders of
    summing nw numbers differ by at most (nw - 1) 2^-53 sum |x| each from the exact sum to first order, and a product
    adds 2^-53 of itself: 2 nw 2^-53 sum |x| between them, doubled here.  Nothing measured enters."""
    worst = 0.0
    for k, name in enumerate(NAMES):
        freq = (r.ir if name.startswith("ir") else r.sol).freq
        dnu = freq[:-1] - freq[1:]
        a = spec[name]                                   # (nz+1, nw, ncol)
        nw = a.shape[1]
        assert a.shape[0] == r.nz + 1 and len(dnu) == nw
        prod = a * dnu[None, :, None]
        got, scale = prod.sum(axis=1), np.abs(prod).sum(axis=1)
        bound = 2.0 * nw * 2.0 ** -52 * scale
        err = np.abs(got - fluxes[:, k, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
        assert np.all(err <= bound), (name, float(np.max(err - bound)))
    print("sum identity: largest error / bound = %.3f" % worst)


def set2():
    """tables, nz and the 9 columns of the one-launch-per-chunk tests"""
    from clima_amd import synthetic as S
    return S.modern_earth_tables(nw=60), 100, S.perturbed_columns(9, nz=100, seed=3)


def child_main():
    """Test 3: the nz = 100 set under whatever launch-form switches the environment carries.  CLIMA_HIP_BATCH_COLS=4: 9
    columns in chunks of 4, 4 and 1, each chunk overwriting the arena of the one before -- the reference is test 2's,
    a second handle with coop_items = 0.  CLIMA_HIP_BATCH_ONE_LAUNCH=0: the columns' calls back to back, each what the
    handle's own TOA_fluxes enqueues (test_column_batch_equals_one_call_per_column), so the second handle is left as
    it is made."""
    from clima_amd.radtran import Radtran
    tables, nz, cols = set2()
    levels = [nz, 0, 0, 25]
    r = Radtran(tables, nz, NZEN, 0.2)
    plain = r.TOA_fluxes_batch(cols, return_fluxes=True)
    isr, olr, fl, spec = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=levels)
    dev = device_spectra(r, cols, levels, sync=False)
    one = Radtran(tables, nz, NZEN, 0.2)
    if os.environ.get("CLIMA_HIP_BATCH_ONE_LAUNCH", "1") != "0":
        one.coop_items = 0
    own = own_call_rows(one, cols)
    assert_rows_equal(spec, own, levels, "host form")
    assert_rows_equal(dev[3], own, levels, "device form")
    for g, d, w, name in zip((isr, olr, fl), dev, plain, ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
        np.testing.assert_array_equal(d, w, err_msg=name)
    print("fused_fallbacks = %d" % r.fused_fallbacks)
    assert r.fused_fallbacks == 0
    print("child ok")


if __name__ == "__main__":
    child_main()
    sys.exit(0)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the two column sets, computed once
@pytest.fixture(scope="module")
def per_column(small_tables):
    """Set 1 (50 layers: one call per column).  The handle, the columns, the own-call rows on the SAME handle, the plain
    batch's results and the state it leaves, then the spectra batch's results and state."""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    from test_gpu_batch_device import handle_state
    cols = S.perturbed_columns(9, NZ, seed=3)
    r = Radtran(small_tables, NZ, NZEN, ALBEDO)
    own = own_call_rows(r, cols)
    plain = r.TOA_fluxes_batch(cols, return_fluxes=True)
    plain_state = handle_state(r)
    got = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=LEVELS)
    got_state = handle_state(r)
    return dict(r=r, cols=cols, own=own, plain=plain, plain_state=plain_state, got=got, got_state=got_state)


@pytest.fixture(scope="module")
def per_chunk():
    """Set 2 (100 layers: one launch per chunk).  Own-call rows on a second handle with coop_items = 0: the batch runs
    the lane-per-item opacity kernel inside the fused grid, so does that call (test_state_after_a_column_batch_is_the_last_columns)."""
    from clima_amd.radtran import Radtran
    tables, nz, cols = set2()
    r = Radtran(tables, nz, NZEN, 0.2)
    one = Radtran(tables, nz, NZEN, 0.2)
    one.coop_items = 0
    own = own_call_rows(one, cols)
    plain = r.TOA_fluxes_batch(cols, return_fluxes=True)
    levels = [nz, 0, 0, 25]
    got = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=levels)
    return dict(r=r, cols=cols, own=own, plain=plain, got=got, levels=levels, nz=nz, tables=tables)


# ------------------------------------------------------------------ tests
def test_one_call_per_column(per_column):
    p = per_column
    assert len(p["got"]) == 4
    assert_rows_equal(p["got"][3], p["own"], LEVELS)
    for g, w, name in zip(p["got"], p["plain"], ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for g, w, name in zip(p["got_state"], p["plain_state"], ("f_total", "wrk_ir.fup_a", "wrk_sol.tau_band")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert p["r"].fused_fallbacks == 0


def test_one_launch_per_chunk(per_chunk):
    p = per_chunk
    assert_rows_equal(p["got"][3], p["own"], p["levels"])
    for g, w, name in zip(p["got"], p["plain"], ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert p["r"].fused_fallbacks == 0


def test_one_launch_per_chunk_paired_layers(small_tables):
    """102 layers of exact pairs (AdiabatClimate's 50 doubled): the last column against what the batch leaves in the
    handle, every column by the sum identity"""
    from clima_amd.radtran import Radtran
    cols = doubled(50, 9)
    nz = len(cols[0]["T"])
    r = Radtran(small_tables, nz, NZEN, ALBEDO)
    plain = r.TOA_fluxes_batch(cols, return_fluxes=True)
    isr, olr, fl, spec = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=np.arange(nz + 1))
    for g, w, name in zip((isr, olr, fl), plain, ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for name in NAMES:
        left = np.array(getattr(r.wrk_ir if name.startswith("ir") else r.wrk_sol, name.split("_", 1)[1]))
        np.testing.assert_array_equal(spec[name][:, :, -1], left, err_msg=name)
    assert_sum_identity(r, fl, spec)
    assert r.fused_fallbacks == 0


@pytest.mark.parametrize("env", [{"CLIMA_HIP_BATCH_COLS": "4"}, {"CLIMA_HIP_BATCH_ONE_LAUNCH": "0"}], ids=["chunks_of_4", "per_column"])
def test_the_arena_is_reused_in_a_fresh_process(env):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=e, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0 and "child ok" in p.stdout and "fused_fallbacks = 0" in p.stdout


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "synchronize_later"])
def test_device_form_equals_host_form(per_column, per_chunk, sync):
    for p, levels in ((per_column, LEVELS), (per_chunk, per_chunk["levels"])):
        dev = device_spectra(p["r"], p["cols"], levels, sync=sync)
        for g, w, name in zip(dev, p["got"], ("ISR", "OLR", "fluxes")):
            np.testing.assert_array_equal(g, w, err_msg=name)
        assert sorted(dev[3]) == sorted(NAMES)
        for name in NAMES:
            np.testing.assert_array_equal(dev[3][name], p["got"][3][name], err_msg=name)
        only = device_spectra(p["r"], p["cols"], levels, sync=sync, spectra=("ir_fup_a",))[3]
        assert list(only) == ["ir_fup_a"]
        np.testing.assert_array_equal(only["ir_fup_a"], p["got"][3]["ir_fup_a"])
        host_only = p["r"].TOA_fluxes_batch(p["cols"], spectra_levels=levels, spectra=("sol_fdn_a",))
        assert len(host_only) == 3 and list(host_only[2]) == ["sol_fdn_a"]
        np.testing.assert_array_equal(host_only[2]["sol_fdn_a"], p["got"][3]["sol_fdn_a"])
        assert p["r"].fused_fallbacks == 0


def test_the_repeat_refills_the_spectra():
    """The setup of test_expired_handoff_is_repaired_at_synchronize: fused_spins = 0, so hand-off waits expire and
    synchronize() runs the batch again through the separate launches -- into the same tensors, the spectra included.
    The reference is the host spectra batch of a default handle whose `fused` switch is off (what a repeat runs)."""
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    tables = S.modern_earth_tables(nw=400)
    nz = 200
    col = S.modern_earth_column(nz)
    warm = S.Column(col)
    warm["T"] = np.asarray(col["T"]) + 3.0
    cols = [col, warm]
    levels = [nz, 0, 0, 100]
    ref = Radtran(tables, nz, 4, 0.2)
    ref.fused = False
    want = ref.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=levels)
    r = Radtran(tables, nz, 4, 0.2)
    r.fused_spins = 0
    n0 = r.fused_fallbacks
    isr, olr, fl, spec = r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), return_fluxes=True, sync=False, spectra_levels=levels)
    assert r.fused_fallbacks == n0           # nothing has been looked at yet
    r.synchronize()
    assert r.fused_fallbacks == n0 + 1
    got = (isr.cpu().numpy(), olr.cpu().numpy(), np.transpose(fl.cpu().numpy(), (2, 1, 0)))
    for g, w, name in zip(got, want, ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert sorted(spec) == sorted(NAMES)
    for name in NAMES:
        np.testing.assert_array_equal(np.transpose(spec[name].cpu().numpy(), (1, 2, 0)), want[3][name], err_msg=name)
    r.synchronize()                          # settled: nothing is repeated twice
    assert r.fused_fallbacks == n0 + 1
    # the host form on the same handle repeats itself the same way, spectra included
    host = r.TOA_fluxes_batch(cols, return_fluxes=True, spectra_levels=levels)
    assert r.fused_fallbacks == n0 + 2
    for name in NAMES:
        np.testing.assert_array_equal(host[3][name], want[3][name], err_msg=name)


def test_the_rows_are_the_ones_that_were_integrated(per_column, per_chunk):
    for p in (per_column, per_chunk):
        r = p["r"]
        isr, olr, fl, spec = r.TOA_fluxes_batch(p["cols"], return_fluxes=True, spectra_levels=np.arange(r.nz + 1))
        np.testing.assert_array_equal(fl, p["plain"][2])
        assert_sum_identity(r, fl, spec)
        # ... and they are the own-call rows, every level
        assert_rows_equal(spec, p["own"], np.arange(r.nz + 1))


def test_refusals_leave_the_handle_usable(small_tables, per_column):
    import torch
    from clima_amd.radtran import ClimaException, Radtran
    p = per_column
    r, cols = p["r"], p["cols"]
    # the ABI's levels are 1..nz+1: 0 and nz+2 through the raw host call, index and value named
    a = stacked(cols, r.np)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def d(x):
        return x.ctypes.data_as(dp) if x is not None else None

    n = len(cols)
    isr, olr = np.empty(n), np.empty(n)
    nw_ir = len(r.ir.freq) - 1

    def raw_host(levels, out):
        lv = np.asarray(levels, dtype=np.int32)
        r._L.radtran_toa_fluxes_batch_spectra(r._ptr, C.byref(C.c_int(n)), d(a["T_surface"]), d(a["T"]), d(a["P"]), d(a["densities"]),
                                              d(a["dz"]), C.byref(C.c_int(1 if r.np > 0 else 0)), d(a.get("pdensities")),
                                              d(a.get("radii")), d(isr), d(olr), None, C.byref(C.c_int(len(lv))),
                                              lv.ctypes.data_as(ip), d(out), None, None, None, r._err)
        r._check()

    buf = np.empty((n, 2, nw_ir))
    with pytest.raises(ClimaException, match=r"spec_level\(2\) = 0 is outside 1\.\.%d" % (NZ + 1)):
        raw_host([NZ + 1, 0], buf)
    with pytest.raises(ClimaException, match=r"spec_level\(1\) = %d is outside 1\.\.%d" % (NZ + 2, NZ + 1)):
        raw_host([NZ + 2, 1], buf)
    with pytest.raises(ClimaException, match=r"nsel must be at least 1 \(nsel = 0\)"):
        r.TOA_fluxes_batch(cols, spectra_levels=[])
    with pytest.raises(ClimaException, match="none of ir_fup, ir_fdn, sol_fup, sol_fdn was given"):
        r.TOA_fluxes_batch(cols, spectra_levels=[0], spectra=())
    with pytest.raises(ClimaException, match="none of ir_fup, ir_fdn, sol_fup, sol_fdn was given"):
        r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), spectra_levels=[0], spectra=())
    with pytest.raises(ClimaException, match=r"spectra_levels\[1\] = %d is outside -%d\.\.%d" % (NZ + 1, NZ + 1, NZ)):
        r.TOA_fluxes_batch(cols, spectra_levels=[0, NZ + 1])
    with pytest.raises(ClimaException, match=r"spectra_levels\[0\] = %d is outside" % (NZ + 1)):
        r.TOA_fluxes_batch_tensors(**tensors(cols, r.np), spectra_levels=[NZ + 1])
    # a host numpy pointer as d_ir_fup through the raw device call
    t = tensors(cols, r.np)
    d_isr, d_olr = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    lv = np.array([NZ + 1, 1], dtype=np.int32)
    torch.cuda.synchronize()
    r._L.radtran_toa_fluxes_batch_spectra_device(r._ptr, C.byref(C.c_int(n)), t["T_surface"].data_ptr(), t["T"].data_ptr(), t["P"].data_ptr(),
                                                 t["densities"].data_ptr(), t["dz"].data_ptr(), C.byref(C.c_int(1 if r.np > 0 else 0)),
                                                 t["pdensities"].data_ptr() if r.np > 0 else None,
                                                 t["radii"].data_ptr() if r.np > 0 else None, d_isr.data_ptr(), d_olr.data_ptr(), None,
                                                 C.byref(C.c_int(2)), lv.ctypes.data_as(ip), buf.ctypes.data, None, None, None, None, r._err)
    with pytest.raises(ClimaException, match='toa_fluxes_batch_device: "ir_fup" is not device memory of this handle\'s device'):
        r._check()
    sharded = Radtran(small_tables, NZ, NZEN, ALBEDO)
    sharded.set_bin_shard(0, 2)
    with pytest.raises(ClimaException, match="toa_fluxes_batch is not available on a bin-sharded handle"):
        sharded.TOA_fluxes_batch(cols, spectra_levels=[0])
    with pytest.raises(ClimaException, match="toa_fluxes_batch is not available on a bin-sharded handle"):
        sharded.TOA_fluxes_batch_tensors(**t, spectra_levels=[0])
    # a plain batch afterwards gives the earlier bits, and so does a spectra batch
    for g, w, name in zip(r.TOA_fluxes_batch(cols, return_fluxes=True), p["plain"], ("ISR", "OLR", "fluxes")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    np.testing.assert_array_equal(r.TOA_fluxes_batch(cols, spectra_levels=LEVELS)[2]["ir_fup_a"], p["got"][3]["ir_fup_a"])


def test_against_the_oracle(O, small_tables, per_column):
    from test_gpu_parity import TOL_SPEC
    p = per_column
    top = LEVELS.index(NZ)
    o = O.OracleRadtran(small_tables, NZ, NZEN, ALBEDO)
    for c in (0, 4, 8):
        o.TOA_fluxes(*p["cols"][c].args())
        want = np.asarray(o.wrk_ir.fup_a)
        a_scale = max(float(np.max(np.abs(want))), float(np.max(np.abs(np.asarray(o.wrk_ir.fdn_a)))), 1e-300)
        err = float(np.max(np.abs(p["got"][3]["ir_fup_a"][top, :, c] - want[-1, :])))
        print("column %d: largest |batch - oracle| of the TOA IR row = %.3e of the channel's scale (bound %.0e)" % (c, err / a_scale, TOL_SPEC))
        assert err <= TOL_SPEC * a_scale
