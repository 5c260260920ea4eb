"""What tests/test_gpu_sol_opr_sens.py and tools/gpu_sol_opr_sens.py share: the stored exact derivatives
(tests/golden/exact_sol_opr_sens_*.npz, made by tests/golden/make_exact_sol_opr_sens.py), the hook, and the measure.  No
mpmath here.  A helper, not a test.

The criterion is exact_two_stream_cases': kernel error <= max(FLOOR x scale, MARGIN x e_ref), per column and per derivative
array (up / dn / am x tau / w0 / g / rsfc): scale the array's largest exact magnitude, e_ref the stored error of the
reference algorithm's float64 restatement on that array.  An array that is identically zero must come back as zeros."""
import ctypes as C
import glob
import os

import numpy as np

from exact_two_stream_cases import DP, FLOOR, IP, MARGIN, weights
from ir_opr_sens_cases import OprRecord

HERE = os.path.dirname(os.path.abspath(__file__))
QUANTITIES = ("up", "dn", "am")
PARAMS = ("tau", "w0", "g", "rsfc")
NAMES = tuple("%s_%s" % (q, p) for q in QUANTITIES for p in PARAMS)
NCOLUMNS = 14


def load():
    d = {}
    for p in sorted(glob.glob(os.path.join(HERE, "golden", "exact_sol_opr_sens_*.npz"))):
        with np.load(p) as z:
            d.update({k: z[k] for k in z.files})
    return d


def _i(v):
    return C.byref(C.c_int(int(v)))


def _p(a):
    return a.ctypes.data_as(DP)


def sol_opr_sens(L, tau, w0, g, zen_u, zen_w, rsfc, ng, levels):
    """clima_test_sol_opr_sens -> ({name: (nrow, nz), or (nrow,) for rsfc}, error text)"""
    tau, w0, g, zu, zw = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g, zen_u, zen_w))
    rs = np.array([float(np.ravel(rsfc)[0])])
    nz, nr = len(tau), len(levels)
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    out = {k: np.full((nr,) if k.endswith("rsfc") else (nr, nz), np.nan) for k in NAMES}
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_sol_opr_sens(_i(nz), _i(ng), _p(tau), _p(w0), _p(g), _p(wb), _i(len(zu)), _p(zu), _p(zw), _p(rs), _i(nr),
                              lv.ctypes.data_as(IP), *[_p(out[k]) for k in NAMES], err)
    return out, err.value.decode()


def run(L, E, ng):
    """every stored column -> (records, columns run, names of the identically-zero arrays that did not come back as zeros)"""
    recs, ran, nonzero = [], 0, []
    for n in range(int(E["n"][0])):
        k = "s%02d_" % n
        tau, lv = E[k + "tau"], E[k + "levels"]
        out, err = sol_opr_sens(L, tau, E[k + "w0"], E[k + "g"], E[k + "zen_u"], E[k + "zen_w"], E[k + "rsfc"], ng, lv)
        assert err == "", (k, err)
        for i, name in enumerate(NAMES):
            x = E[k + name]
            e = np.max(np.abs(out[name] - x))
            if not np.any(x != 0.0) and not np.all(out[name] == 0.0):
                nonzero.append(k + name)
            recs.append(OprRecord("sol_opr_sens", "ng %d" % ng, "nz %d nzen %d rsfc %g" % (len(tau), len(E[k + "zen_u"]), E[k + "rsfc"][0]),
                                  "s%02d" % n, name, e if np.isfinite(e) else np.inf, E[k + "e_ref"][i], np.max(np.abs(x))))
        ran += 1
    return recs, ran, nonzero


def worst_ratios(recs):
    """{parameter: the largest err / allowed} over the records"""
    out = {}
    for r in recs:
        p = r.quantity.split("_")[1]
        allowed = max(FLOOR * r.scale, MARGIN * r.e_ref)
        ratio = r.err / allowed if allowed > 0 else (0.0 if r.err == 0 else np.inf)
        out[p] = max(out.get(p, 0.0), ratio)
    return out
