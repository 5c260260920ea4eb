"""What tests/test_gpu_ir_opr_sens.py and tools/gpu_ir_opr_sens.py share: the stored exact derivatives
(tests/golden/exact_ir_opr_sens_*.npz, made by tests/golden/make_exact_ir_opr_sens.py), the hook, and the measure.  No
mpmath here.  A helper, not a test.

The criterion is exact_two_stream_cases': kernel error <= max(FLOOR x scale, 10 x e_ref), per column and per derivative
array (up / dn x tau / w0 / g): scale the array's largest exact magnitude, e_ref the stored error of the reference
algorithm's float64 restatement on that array."""
import ctypes as C
import glob
import os

import numpy as np

from exact_two_stream_cases import DP, FLOOR, IP, MARGIN, Record, weights

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("up_tau", "up_w0", "up_g", "dn_tau", "dn_w0", "dn_g")
NCOLUMNS = 14


class OprRecord(Record):
    """a Record whose scale may be 0 (a derivative array that is identically zero: the kernel must give zeros too)"""

    def __repr__(self):
        s = self.scale if self.scale > 0 else 1.0
        return "%s %s | %s %s | %s: kernel %.2e, reference %.2e of the scale %.2e (allowed %.2e)" % (
            self.hook, self.form, self.name, self.group, self.quantity, self.err / s, self.e_ref / s, self.scale,
            max(FLOOR * self.scale, MARGIN * self.e_ref) / s)


def load():
    d = {}
    for p in sorted(glob.glob(os.path.join(HERE, "golden", "exact_ir_opr_sens_*.npz"))):
        with np.load(p) as z:
            d.update({k: z[k] for k in z.files})
    return d


def _i(v):
    return C.byref(C.c_int(int(v)))


def _p(a):
    return a.ctypes.data_as(DP)


def ir_opr_sens(L, tau, w0, g, bplanck, ir_par, ng, levels):
    """clima_test_ir_opr_sens -> ({name: (nrow, nz)}, error text)"""
    tau, w0, g, bp, par = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g, bplanck, ir_par))
    nz, nr = len(tau), len(levels)
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    out = {k: np.full((nr, nz), np.nan) for k in NAMES}
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_ir_opr_sens(_i(nz), _i(ng), _p(tau), _p(w0), _p(g), _p(bp), _p(par), _p(wb), _i(nr), lv.ctypes.data_as(IP),
                             *[_p(out[k]) for k in NAMES], err)
    return out, err.value.decode()


def run(L, E, ng):
    """every stored column -> (records, columns run)"""
    recs, ran = [], 0
    for n in range(int(E["n"][0])):
        k = "s%02d_" % n
        tau, par, lv = E[k + "tau"], E[k + "ir_par"], E[k + "levels"]
        out, err = ir_opr_sens(L, tau, E[k + "w0"], E[k + "g"], E[k + "bplanck"], par, ng, lv)
        assert err == "", (k, err)
        for i, name in enumerate(NAMES):
            x = E[k + name]
            e = np.max(np.abs(out[name] - x))
            if name.startswith("dn") and 0 in lv.tolist():
                assert np.all(out[name][lv.tolist().index(0)] == 0.0), (k, name)      # fdn(level 0) = 0: exact zeros
            recs.append(OprRecord("ir_opr_sens", "ng %d" % ng, "nz %d hard %d" % (len(tau), int(par[1])), "s%02d" % n, name,
                               e if np.isfinite(e) else np.inf, E[k + "e_ref"][i], np.max(np.abs(x))))
        ran += 1
    return recs, ran


def worst_ratios(recs):
    """{parameter: the largest err / allowed} over the records"""
    out = {}
    for r in recs:
        p = r.quantity.split("_")[1]
        allowed = max(FLOOR * r.scale, MARGIN * r.e_ref)
        ratio = r.err / allowed if allowed > 0 else (0.0 if r.err == 0 else np.inf)
        out[p] = max(out.get(p, 0.0), ratio)
    return out
