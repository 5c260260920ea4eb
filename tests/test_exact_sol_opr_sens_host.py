"""The exact solar optical-property derivatives without a GPU: two of the stored columns regenerated (mpmath, 80 digits) and
held to tests/golden/exact_sol_opr_sens_0.npz bit for bit, the stored file's coverage, and the float64 restatement's forward
values held to exact_two_stream.exact_solar_sum (the restatement is the yardstick e_ref is measured with: it has to be
two_stream_solar)."""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("mpmath")
import exact_sol_opr_sens as X  # noqa: E402
import sol_opr_sens_cases as K  # noqa: E402
from exact_two_stream import exact_solar_sum  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_exact_sol_opr_sens as G  # noqa: E402


@pytest.fixture(scope="module")
def stored():
    return K.load()


@pytest.mark.parametrize("n", [1, 4])        # nz = 1 at the w0 cap over a perfect reflector; nz = 3 with four zenith angles
def test_a_stored_column_is_what_the_generator_gives(stored, n):
    c = G.case(n, with_ref=False)
    for name, v in c.items():
        assert np.array_equal(stored["s%02d_%s" % (n, name)], v), name


def test_the_stored_file_holds_what_the_gpu_test_needs(stored):
    E = stored
    assert int(E["n"][0]) == K.NCOLUMNS == len(G.CASES) and K.NAMES == X.NAMES
    nzs, rs, nzen = set(), set(), set()
    feats = dict(neg_g=False, w0_zero=False, cap=False, tau0=False, thick=False, grazing=False, near=False, uneven=False)
    for m in range(K.NCOLUMNS):
        k = "s%02d_" % m
        tau, w0, g, zu, zw = (E[k + x] for x in ("tau", "w0", "g", "zen_u", "zen_w"))
        nz = len(tau)
        nzs.add(nz); rs.add(float(E[k + "rsfc"][0])); nzen.add(len(zu))
        lv = E[k + "levels"].tolist()
        assert lv[0] == 0 and lv[-1] == nz and (nz < 3 or len(lv) == 4)
        assert E[k + "e_ref"].shape == (12,) and np.all(np.isfinite(E[k + "e_ref"]))
        for x in K.NAMES:
            assert E[k + x].shape == ((len(lv),) if x.endswith("rsfc") else (len(lv), nz)) and np.all(np.isfinite(E[k + x])), (k, x)
        assert np.all(E[k + "dn_tau"][0] == 0.0) and np.all(E[k + "dn_rsfc"][0] == 0.0)       # fdn at the top is u0
        feats["neg_g"] |= bool(np.any(g < 0)); feats["w0_zero"] |= bool(np.all(w0 == 0)); feats["cap"] |= bool(np.any(w0 == 0.99999))
        feats["tau0"] |= bool(np.any(tau == 0)); feats["thick"] |= bool(np.any(tau == 3.0e4)); feats["grazing"] |= bool(np.any(zu == 0.05))
        feats["uneven"] |= len(zu) == 4 and len(set(zw.tolist())) == 4
        lam = G.lam_of(w0, g)
        feats["near"] |= bool(np.any(np.abs(np.abs(lam[:, None] * zu[None, :] - 1.0) - 1.0e-3) < 1.0e-5))
    assert {1, 2, 63, 64, 65, 129} <= nzs and {0.0, 1.0} <= rs and {1, 4} <= nzen
    assert all(feats.values()), feats


@pytest.mark.parametrize("n", [0, 4, 6, 8])
def test_the_restatement_is_two_stream_solar(stored, n):
    """its forward values against the 50-digit sums: 1e-12 of each array's largest value (float64 rounding of a 2nz-row
    solve; column 6 divides by lambda^2 - 1/u0^2 = 2e-3 / u0^2 and gets 1e3 times that)"""
    k = "s%02d_" % n
    a = tuple(stored[k + x] for x in ("tau", "w0", "g", "zen_u", "zen_w")) + (float(stored[k + "rsfc"][0]),)
    (fup, fdn, am), _ = X.restated_solar(*a)
    e_am, e_up, e_dn = exact_solar_sum(*a)
    tol = 1.0e-9 if n == 6 else 1.0e-12
    for got, ex in ((fup, e_up), (fdn, e_dn), (am, e_am)):
        assert np.max(np.abs(got.detach().numpy() - ex)) <= tol * np.max(np.abs(ex))
