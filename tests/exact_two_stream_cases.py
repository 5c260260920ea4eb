"""What tests/test_gpu_exact_two_stream.py, tools/gpu_exact_two_stream.py and the fixture's generator share: the stored
exact values (tests/golden/exact_two_stream_*.npz, made by tests/golden/make_exact_two_stream.py), the reference
algorithm's TRUE error on each column, the four hooks, and the measure.  No mpmath here.  A helper, not a test.

The measure (the project's, tests/test_gpu_golden.py::_check): the up and down fluxes of a channel on their common
scale, the largest exact flux of the two; amean on its own; a unit-response matrix pair on its largest entry; a change
of the fluxes through dB at level k on |dB| times that largest entry.

The criterion: kernel error <= max(FLOOR * scale, 10 * e_ref).  e_ref is what the reference algorithm itself is off by
on that quantity of that column: the largest of |golden - exact| (where the reference's own output is stored),
|oracle - exact| and |oracle compiled with FMA contraction - exact|.  FLOOR is test_gpu_golden.TOL, the factor 10 the
project's margin over a yardstick; neither is tuned here.
"""
import ctypes as C
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-10                       # test_gpu_golden.TOL (asserted equal by the tests)
MARGIN = 10.0
WBIN8 = np.array([0.0625, 0.125, 0.1875, 0.125, 0.0625, 0.25, 0.125, 0.0625])      # test_gpu_golden._run's
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
VARIANTS = ("", "fma")


def _load(pattern):
    d = {}
    for p in sorted(glob.glob(os.path.join(HERE, "golden", pattern))):
        with np.load(p) as z:
            d.update({k: z[k] for k in z.files})
    return d


def load_golden():
    return _load("twostream_golden_*.npz")


def load_exact():
    return _load("exact_two_stream_*.npz")


def weights(ng):
    return WBIN8 if ng == 8 else np.full(ng, 1.0 / ng) if ng > 1 else np.ones(1)


def allowed(err, scale, e_ref):
    return err <= max(FLOOR * scale, MARGIN * e_ref)


# ------------------------------------------------------------------------------------------------ columns

class Column:
    """One column with its exact outputs: a golden case (inputs from the golden archive, `gold` the reference's own
    outputs) or a new edge column (inputs from the exact archive, gold None)."""

    def __init__(self, name, group, src, k, exact, gold, paired):
        self.name, self.group, self.paired, self.key = name, group, paired, k
        self.tau, self.w0, self.g, self.bp = (np.ascontiguousarray(src[k + x], dtype=np.float64) for x in ("tau", "w0", "g", "bplanck"))
        self.ir_par, self.sol_par = np.ascontiguousarray(src[k + "ir_par"], dtype=np.float64), np.ascontiguousarray(src[k + "sol_par"], dtype=np.float64)
        self.nz = len(self.tau)
        names = ("ir_fup", "ir_fdn", "sol_fup", "sol_fdn", "sol_amean")
        self.exact = {x: exact[k + x] for x in names}
        self.gold = None if gold is None else {x: gold[k + x] for x in names}
        self._ref = None

    def scales(self):
        e = self.exact
        return {"ir": max(np.max(np.abs(e["ir_fup"])), np.max(np.abs(e["ir_fdn"]))),
                "sol": max(np.max(np.abs(e["sol_fup"])), np.max(np.abs(e["sol_fdn"]))),
                "amean": np.max(np.abs(e["sol_amean"]))}

    def errors(self, out):
        """out: the five arrays in the hook's order (None where not computed) -> {quantity: absolute error}"""
        e, r = self.exact, {}
        if out[0] is not None:
            r["ir"] = max(np.max(np.abs(out[0] - e["ir_fup"])), np.max(np.abs(out[1] - e["ir_fdn"])))
        if out[2] is not None:
            r["sol"] = max(np.max(np.abs(out[2] - e["sol_fup"])), np.max(np.abs(out[3] - e["sol_fdn"])))
            r["amean"] = np.max(np.abs(out[4] - e["sol_amean"]))
        return {k: float(v) if np.isfinite(v) else np.inf for k, v in r.items()}

    def ref_errors(self, O):
        """{quantity: e_ref, absolute}; computed once"""
        if self._ref is None:
            em, hs, tmin = self.ir_par
            u0, rs = self.sol_par
            outs = [] if self.gold is None else [[self.gold[x] for x in ("ir_fup", "ir_fdn", "sol_fup", "sol_fdn", "sol_amean")]]
            for v in VARIANTS:
                a = O.two_stream_ir(self.tau, self.w0, self.g, em, bool(hs), tmin, self.bp, variant=v)
                b = O.two_stream_solar(self.tau, self.w0, self.g, u0, rs, variant=v)
                outs.append([a[0], a[1], b[2], b[3], b[0]])
            self.ref_finite = all(np.all(np.isfinite(x)) for o in outs for x in o)
            assert self.ref_finite, "the reference algorithm is not finite on %s: no yardstick" % self.name
            errs = [self.errors(o) for o in outs]
            self._ref = {q: max(e[q] for e in errs) for q in ("ir", "sol", "amean")}
        return self._ref


def golden_group(n, paired_first):
    if n in (21, 33):
        return "golden c%02d" % n
    return "golden stress 0-35" if n < 36 else "golden smooth 36-%d" % (paired_first - 1) if n < paired_first else "golden paired %d-" % paired_first


def columns(G, E):
    """every golden case and every new edge column"""
    first = int(G["paired_first"][0])
    cols = [Column("c%02d" % n, golden_group(n, first), G, "c%02d_" % n, E, G, n >= first) for n in range(int(G["ncases"][0]))]
    for n in range(int(E["edge_n"][0])):
        kind = str(E["edge_kind"][n])
        paired = bool(E["edge_paired"][n])
        cols.append(Column("e%02d %s%s" % (n, kind, " paired" if paired else ""), "edge mixed" if kind.startswith("mixed") else "edge resonant " + kind[4:7],
                           E, "e%02d_" % n, E, None, paired))
    return cols


# ------------------------------------------------------------------------------------------------ the hooks

def _i(v):
    return C.byref(C.c_int(int(v)))


def _p(a):
    return a.ctypes.data_as(DP)


def two_stream(L, col, form, slots, ng=8):
    """clima_test_two_stream -> (the five arrays, error text)"""
    out = [np.full(col.nz + 1, np.nan) for _ in range(5)]
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_two_stream(_i(col.nz), _i(ng), _i(form), _i(slots), _p(col.tau), _p(col.w0), _p(col.g), _p(col.bp),
                            _p(col.ir_par), _p(col.sol_par), _p(wb), *[_p(o) for o in out], err)
    return out, err.value.decode()


def solar_batch(L, tau, w0, g, ng, force_nw, zen_u, zen_w, rsfc):
    """clima_test_solar_batch: zen_u, zen_w (ncol, nzen), rsfc (ncol) -> (fup, fdn, amean (ncol, nz+1) TOA-first, error text)"""
    tau, w0, g = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g))
    zen_u, zen_w, rsfc = (np.ascontiguousarray(a, dtype=np.float64) for a in (zen_u, zen_w, rsfc))
    n, nzen = zen_u.shape
    nz = len(tau)
    out = [np.full((n, nz + 1), np.nan) for _ in range(3)]
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_solar_batch(_i(nz), _i(ng), _i(force_nw), _p(tau), _p(w0), _p(g), _p(wb), _i(n), _i(nzen), _p(zen_u), _p(zen_w),
                             _p(rsfc), *[_p(o) for o in out], err)
    return out, err.value.decode()


def ir_adjoint(L, tau, w0, g, ir_par, ng, levels):
    """clima_test_ir_adjoint -> (dfup, dfdn (nrow, nz+1), error text)"""
    tau, w0, g, par = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g, ir_par))
    nz, nr = len(tau), len(levels)
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    up, dn = np.full((nr, nz + 1), np.nan), np.full((nr, nz + 1), np.nan)
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_ir_adjoint(_i(nz), _i(ng), _p(tau), _p(w0), _p(g), _p(par), _p(wb), _i(nr), lv.ctypes.data_as(IP), _p(up), _p(dn), err)
    return up, dn, err.value.decode()


def ir_response(L, tau, w0, g, ir_par, ng, dev_k, dev_db):
    """clima_test_ir_response -> (up, dn (ndev, nz+1), error text)"""
    tau, w0, g, par = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w0, g, ir_par))
    nz, nd = len(tau), len(dev_k)
    kk, db = np.ascontiguousarray(dev_k, dtype=np.int32), np.ascontiguousarray(dev_db, dtype=np.float64)
    up, dn = np.full((nd, nz + 1), np.nan), np.full((nd, nz + 1), np.nan)
    err = C.create_string_buffer(1025)
    wb = weights(ng)
    L.clima_test_ir_response(_i(nz), _i(ng), _p(tau), _p(w0), _p(g), _p(par), _p(wb), _i(nd), kk.ctypes.data_as(IP), _p(db), _p(up), _p(dn), err)
    return up, dn, err.value.decode()


# ------------------------------------------------------------------------------------------------ shape rules
# (the launchers' own: clima_test_two_stream answers "does not cover the requested shape" outside them)

def fits(col, form, slots, ng=8):
    nz = col.nz
    if form in (0, 3, 6):
        return slots == 0 or (nz + 63) // 64 <= slots <= 8
    if form == 1:
        return True
    if form == 2:
        return ng == 8 and 2 <= slots <= 8 and (nz + 63) // 64 <= slots
    if form == 4:
        return ng == 8 and 3 <= slots <= 7 and (nz + 31) // 32 <= slots
    if form == 5:
        return ng == 8 and col.paired and nz % 2 == 0 and slots % 2 == 0 and 2 * ((nz // 2 + 63) // 64) <= slots <= 8
    raise ValueError(form)


def natural_slots(col):
    return max(1, (col.nz + 63) // 64)


# ------------------------------------------------------------------------------------------------ records

class Record:
    """One measured quantity of one run: err, e_ref absolute; ok by the criterion."""

    def __init__(self, hook, form, group, name, quantity, err, e_ref, scale):
        self.hook, self.form, self.group, self.name, self.quantity = hook, form, group, name, quantity
        self.err, self.e_ref, self.scale = float(err), float(e_ref), float(scale)
        self.ok = bool(allowed(self.err, self.scale, self.e_ref))

    def __repr__(self):
        return "%s %s | %s | %s: kernel %.2e, reference %.2e of the scale (allowed %.2e)" % (
            self.hook, self.form, self.name, self.quantity, self.err / self.scale, self.e_ref / self.scale,
            max(FLOOR, MARGIN * self.e_ref / self.scale))


def run_two_stream(L, O, cols, form, slots, ng=8, skip_512=False):
    """every column that the form's shape rule admits -> (records, columns run).  slots None: each column's own count."""
    recs, ran = [], 0
    sol = form not in (3, 6)
    for col in cols:
        s = natural_slots(col) if slots is None else slots
        if not fits(col, form, s, ng) or (skip_512 and col.nz >= 512):
            continue
        out, err = two_stream(L, col, form, s, ng)
        assert err == "", (col.name, form, s, err)
        assert out[1][0] == 0.0, col.name                  # fdn(1) = 0, twostream.f90:289
        if not sol:
            out[2] = out[3] = out[4] = None
        e, r, sc = col.errors(out), col.ref_errors(O), col.scales()
        tag = "form %d slots %s ng %d" % (form, "own" if slots is None else slots, ng)
        recs += [Record("two_stream", tag, col.group, col.name, q, e[q], r[q], sc[q]) for q in e]
        ran += 1
    return recs, ran


def run_solar_batch_columns(L, O, cols, ng, force_nw, copies=2):
    """every column as a batch of `copies` cases of its own (u0, Rsfc): each case against exact"""
    recs, ran = [], 0
    for col in cols:
        zu = np.full((copies, 1), col.sol_par[0])
        out, err = solar_batch(L, col.tau, col.w0, col.g, ng, force_nw, zu, np.ones_like(zu), np.full(copies, col.sol_par[1]))
        assert err == "", (col.name, err)
        r, sc = col.ref_errors(O), col.scales()
        for c in range(copies):
            e = col.errors([None, None, out[0][c], out[1][c], out[2][c]])
            tag = "ng %d force_nw %d" % (ng, force_nw)
            recs += [Record("solar_batch", tag, col.group, "%s case %d" % (col.name, c), q, e[q], r[q], sc[q]) for q in e]
        ran += 1
    return recs, ran


def multi_ref_errors(O, E, k):
    """per case (e_ref fluxes, e_ref amean), absolute: sum_z w_z oracle(u_z) of both compilations against exact"""
    tau, w0, g = E[k + "tau"], E[k + "w0"], E[k + "g"]
    out, finite = [], True
    for c in range(len(E[k + "rsfc"])):
        e_fl = e_am = 0.0
        for v in VARIANTS:
            acc = [np.zeros(len(tau) + 1, dtype=np.longdouble) for _ in range(3)]
            for u, w in zip(E[k + "zen_u"][c], E[k + "zen_w"][c]):
                b = O.two_stream_solar(tau, w0, g, float(u), float(E[k + "rsfc"][c]), variant=v)
                finite = finite and all(np.all(np.isfinite(x)) for x in (b[0], b[2], b[3]))
                for a, x in zip(acc, (b[0], b[2], b[3])):
                    a += np.longdouble(w) * x
            acc = [np.asarray(a, dtype=np.float64) for a in acc]
            e_fl = max(e_fl, np.max(np.abs(acc[1] - E[k + "fup"][c])), np.max(np.abs(acc[2] - E[k + "fdn"][c])))
            e_am = max(e_am, np.max(np.abs(acc[0] - E[k + "amean"][c])))
        out.append((float(e_fl), float(e_am)))
    return out, finite


def run_solar_batch_multi(L, O, E, ng, force_nw, cache):
    recs, ran = [], 0
    for m in range(int(E["multi_n"][0])):
        k = "m%02d_" % m
        if k not in cache:
            cache[k] = multi_ref_errors(O, E, k)[0]
        out, err = solar_batch(L, E[k + "tau"], E[k + "w0"], E[k + "g"], ng, force_nw, E[k + "zen_u"], E[k + "zen_w"], E[k + "rsfc"])
        assert err == "", (k, err)
        nzen = E[k + "zen_u"].shape[1]
        for c in range(len(E[k + "rsfc"])):
            s = max(np.max(np.abs(E[k + "fup"][c])), np.max(np.abs(E[k + "fdn"][c])))
            e = max(np.max(np.abs(out[0][c] - E[k + "fup"][c])), np.max(np.abs(out[1][c] - E[k + "fdn"][c])))
            ea = np.max(np.abs(out[2][c] - E[k + "amean"][c]))
            tag, name = "ng %d force_nw %d" % (ng, force_nw), "m%02d nz %d nzen %d case %d" % (m, len(E[k + "tau"]), nzen, c)
            group = "multi-angle nzen %d%s" % (nzen, ", first angle near resonance" if c == 0 else "")
            recs.append(Record("solar_batch", tag, group, name, "sol", e if np.isfinite(e) else np.inf, cache[k][c][0], s))
            recs.append(Record("solar_batch", tag, group, name, "amean", ea if np.isfinite(ea) else np.inf, cache[k][c][1], np.max(np.abs(E[k + "amean"][c]))))
            ran += 1
    return recs, ran


class _Variant:
    """the oracle's two_stream_ir of one compilation, as ir_jacobian_spectral_oracle.unit_responses calls it"""

    def __init__(self, O, v):
        self.O, self.v = O, v

    def two_stream_ir(self, *a):
        return self.O.two_stream_ir(*a, variant=self.v)


def oracle_unit_responses(O, tau, w0, g, ir_par, ks=None):
    """[(up, dn)] of the oracle's two compilations: [level, k], only the columns `ks` when given"""
    import ir_jacobian_spectral_oracle as JS
    em, hs, tmin = (float(x) for x in ir_par)
    return [JS.unit_responses(_Variant(O, v), np.ascontiguousarray(tau)[:, None], np.ascontiguousarray(w0)[:, None], np.ascontiguousarray(g),
                              np.ones(1), em, bool(hs), tmin, ks) for v in VARIANTS]


def adjoint_levels(nz):
    return sorted(set([0, (nz + 1) // 2, nz]))        # the top, mid-column, the surface


def run_adjoint(L, O, E, ng, cache):
    recs, ran = [], 0
    for u in range(int(E["unit_n"][0])):
        k = "u%02d_" % u
        tau, par = E[k + "tau"], E[k + "ir_par"]
        nz = len(tau)
        lv = adjoint_levels(nz)
        if k not in cache:
            cache[k] = oracle_unit_responses(O, tau, E[k + "w0"], E[k + "g"], par)
        xu, xd = E[k + "up"], E[k + "dn"]
        scale = max(np.max(np.abs(xu)), np.max(np.abs(xd)))
        e_ref = max(max(np.max(np.abs(a[lv] - xu[lv])), np.max(np.abs(b[lv] - xd[lv]))) for a, b in cache[k])
        up, dn, err = ir_adjoint(L, tau, E[k + "w0"], E[k + "g"], par, ng, lv)
        assert err == "", (k, err)
        e = max(np.max(np.abs(up - xu[lv])), np.max(np.abs(dn - xd[lv])))
        recs.append(Record("ir_adjoint", "ng %d" % ng, "unit matrices", "u%02d nz %d hard %d" % (u, nz, int(par[1])), "rows",
                           e if np.isfinite(e) else np.inf, e_ref, scale))
        ran += 1
    return recs, ran


def changed_profile(G, r, j):
    kb = "c%02d_" % int(G[r + "base"][0])
    bp = np.array(G[kb + "bplanck"], dtype=np.float64)
    bp[G[r + "c%d_k" % j]] = G[r + "c%d_b" % j]
    return kb, bp


def run_response_golden(L, O, G, E, ng, cache):
    """the golden response cases: exact base + the response form's changes against the exact fluxes of the changed
    profile.  The two sides are not alike here: the kernel's figure holds the error of the change alone (the base is
    exact), e_ref the reference's error of a full solve of the changed profile, its base included.  On these columns
    e_ref is 3e-12 of the scale and the FLOOR decides; the change itself is held on its own scale by
    run_response_deviations."""
    recs, ran = [], 0
    first = int(G["paired_first"][0])
    for m in range(int(G["nresp"][0])):
        r = "r%02d_" % m
        base = int(G[r + "base"][0])
        kb = "c%02d_" % base
        tau, w0, g, par, bp = (G[kb + x] for x in ("tau", "w0", "g", "ir_par", "bplanck"))
        cols, devs = [], []
        for j in range(int(G[r + "ncol"][0])):
            ks, bs = G[r + "c%d_k" % j], G[r + "c%d_b" % j]
            mine = []
            for kk in sorted(set(int(x) for x in ks)):          # (a level may be listed twice: one changed value)
                mine.append(len(devs))
                devs.append((kk, float(bs[list(ks).index(kk)] - bp[kk])))
            cols.append(mine)
        up, dn, err = ir_response(L, tau, w0, g, par, ng, [d[0] for d in devs], [d[1] for d in devs])
        assert err == "", (r, err)
        f0u, f0d = E[kb + "ir_fup"], E[kb + "ir_fdn"]
        scale = max(np.max(np.abs(f0u)), np.max(np.abs(f0d)))
        for j, mine in enumerate(cols):
            xu, xd = E[r + "c%d_fup" % j], E[r + "c%d_fdn" % j]
            key = r + "c%d" % j
            if key not in cache:
                _, bp2 = changed_profile(G, r, j)
                e_ref = max(np.max(np.abs(G[key + "_fup"] - xu)), np.max(np.abs(G[key + "_fdn"] - xd)))
                for v in VARIANTS:
                    a = O.two_stream_ir(tau, w0, g, float(par[0]), bool(par[1]), float(par[2]), bp2, variant=v)
                    e_ref = max(e_ref, np.max(np.abs(a[0] - xu)), np.max(np.abs(a[1] - xd)))
                cache[key] = float(e_ref)
            e = max(np.max(np.abs(f0u + up[mine].sum(axis=0) - xu)), np.max(np.abs(f0d + dn[mine].sum(axis=0) - xd)))
            recs.append(Record("ir_response", "ng %d" % ng, "golden response, base %s" % ("smooth" if base < first else "paired"),
                               "r%02d (c%02d) column %d" % (m, base, j), "changed fluxes", e if np.isfinite(e) else np.inf, cache[key], scale))
        ran += 1
    return recs, ran


def run_response_deviations(L, O, E, ng, cache):
    """the edge columns' deviation lists: each change on its own against dB x the exact unit response"""
    recs, ran = [], 0
    for n in range(int(E["edge_n"][0])):
        k = "e%02d_" % n
        if k + "dev_k" not in E or len(E[k + "tau"]) < 4:      # (the response form takes 4 layers or more)
            continue
        tau, w0, g, par = (E[k + x] for x in ("tau", "w0", "g", "ir_par"))
        ks = sorted(set(int(x) for x in E[k + "dev_k"][0]))
        if k not in cache:
            cache[k] = oracle_unit_responses(O, tau, w0, g, par, ks)
        umax = float(E[k + "dev_umax"][0])
        for s in range(2):
            dk, db = E[k + "dev_k"][s], E[k + "dev_db"][s]
            up, dn, err = ir_response(L, tau, w0, g, par, ng, dk, db)
            assert err == "", (k, err)
            for j, (kk, d) in enumerate(zip(dk, db)):
                xu, xd = E[k + "dev_up"][s, j], E[k + "dev_dn"][s, j]
                e_ref = max(max(np.max(np.abs(d * a[:, kk] - xu)), np.max(np.abs(d * b[:, kk] - xd))) for a, b in cache[k])
                e = max(np.max(np.abs(up[j] - xu)), np.max(np.abs(dn[j] - xd)))
                recs.append(Record("ir_response", "ng %d" % ng, "edge mixed, dB %s" % ("3 %" if s == 0 else "1e-4"),
                                   "e%02d nz %d level %d" % (n, len(tau), kk), "change", e if np.isfinite(e) else np.inf, e_ref, abs(d) * umax))
        ran += 1
    return recs, ran


def failures(recs):
    return [r for r in recs if not r.ok]
