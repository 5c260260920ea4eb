"""f_total is formed in one place per path (the host's f_total_row from the level rows it fetches; k_batch_finish for
a batch out of device memory), always as f_total_level of radtran_dev.h states it:

    f_total = (sol_dn - sol_up) + (ir_dn - ir_up)        (clima_radtran.f90:287)

Every way of getting an f_total is held to that expression BIT FOR BIT, evaluated in this order in float64 numpy from the
four level rows the same object returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NZ = 10


def expected(ir_up, ir_dn, sol_up, sol_dn):
    rows = [np.asarray(x, dtype=np.float64) for x in (ir_up, ir_dn, sol_up, sol_dn)]
    return (rows[3] - rows[2]) + (rows[1] - rows[0])


def assert_handle(r, what):
    want = expected(r.wrk_ir.fup_n, r.wrk_ir.fdn_n, r.wrk_sol.fup_n, r.wrk_sol.fdn_n)
    got = np.array(r.f_total)
    assert got.shape == (NZ + 1,) and np.all(np.isfinite(got)) and np.any(got != 0.0), what
    np.testing.assert_array_equal(got, want, err_msg=what)
    return got


@pytest.fixture(scope="module")
def handle(hip_lib, small_tables):
    from clima_amd.radtran import Radtran
    return Radtran(small_tables, NZ, 2, 0.3)


@pytest.fixture(scope="module")
def column():
    from clima_amd import synthetic as S
    return S.modern_earth_column(NZ)


def test_synchronous_radiate(handle, column):
    handle.radiate(*column.args())
    assert_handle(handle, "radiate")


def test_resident_call(handle, column):
    handle.upload_column(*column.args())
    handle.radiate_resident()
    assert_handle(handle, "upload_column + radiate_resident")


def test_after_radiation_enhancement(handle, column):
    handle.radiate(*column.args())
    before = assert_handle(handle, "radiate")
    sol = np.array(handle.wrk_sol.fdn_n)
    handle.apply_radiation_enhancement(1.7)
    np.testing.assert_array_equal(np.array(handle.wrk_sol.fdn_n), sol * 1.7)     # the rows were scaled ...
    after = assert_handle(handle, "apply_radiation_enhancement(1.7)")            # ... and f_total follows them
    assert np.any(after != before)


def test_every_column_of_a_host_batch(handle):
    from clima_amd import synthetic as S
    cols = S.perturbed_columns(3, NZ, seed=3)
    _, _, fl = handle.TOA_fluxes_batch(cols, return_fluxes=True)
    assert fl.shape == (NZ + 1, 5, 3)
    for c in range(3):
        np.testing.assert_array_equal(fl[:, 4, c], expected(*(fl[:, a, c] for a in range(4))), err_msg="column %d" % c)
    np.testing.assert_array_equal(assert_handle(handle, "the handle after the batch"), fl[:, 4, -1])


def test_every_column_of_a_device_batch(handle):
    from clima_amd import synthetic as S
    from test_gpu_batch_device import tensors
    cols = S.perturbed_columns(3, NZ, seed=3)
    _, _, fl = handle.TOA_fluxes_batch_tensors(**tensors(cols, handle.np), return_fluxes=True)
    fl = fl.cpu().numpy()                       # (ncol, 5, nz+1)
    assert fl.shape == (3, 5, NZ + 1)
    for c in range(3):
        np.testing.assert_array_equal(fl[c, 4], expected(*fl[c, :4]), err_msg="column %d" % c)
    np.testing.assert_array_equal(assert_handle(handle, "the handle after the batch"), fl[-1, 4])


def test_one_rank_communicator(hip_lib, small_tables, column):
    """there the slot behind the four rows carries the step's status word on the device"""
    from clima_amd.radtran import Radtran
    r = Radtran(small_tables, NZ, 2, 0.3)
    r.comm_init_rank(1, 0, Radtran.comm_unique_id())
    r.radiate(*column.args())
    assert_handle(r, "radiate on a one-rank communicator")
    r.upload_column(*column.args())
    r.radiate_resident()
    assert_handle(r, "resident call on a one-rank communicator")
    r.comm_destroy()
