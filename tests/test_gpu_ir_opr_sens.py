"""The gradient of the IR spectra in the stored optical properties on the GPU: clima_test_ir_opr_sens (k_opr_adjoint and
k_opr_sum_g of clima_amd/csrc/ir_opr_sens.inc, one launch of the production kernels) column by column against exact
derivatives, and radtran_ir_spectra_opr_vjp / _device as a whole call.

Exact: tests/exact_ir_opr_sens.py (mpmath, 80 digits, central differences with h = 1e-30, rounded once) -- stored for the
hook's columns (tests/golden/exact_ir_opr_sens_0.npz), computed live per (bin, g-point) from `opr()` for the whole call and
composed over the g-points and the bins in mpmath.  The criterion is exact_two_stream_cases': kernel error <= max(FLOOR x
scale, 10 x e_ref) per column and derivative array, e_ref the error of the reference algorithm's float64 restatement
(autograd) on that array.  No column is left out; every test asserts how many it ran.

Measured on an MI355X (tools/gpu_ir_opr_sens.py; profiles/ir_opr_sens.txt is its output, column by column): on the fourteen
columns, at 1 and at 8 g-points alike, the largest kernel error over the allowed error is 1.2e-4 for d/dtau, 0.38 for
d/dw0 and 0.39 for d/dg.
"""
import ctypes as C

import numpy as np
import pytest

import closed_forms as CF
import exact_ir_opr_sens as X
import exact_two_stream_cases as K2
import ir_opr_sens_cases as K

pytestmark = pytest.mark.gpu
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
GRADS = ("fup", "fdn", "fup_n", "fdn_n")


# ------------------------------------------------------------------ the hook, column by column

@pytest.mark.parametrize("ng", [1, 8])
def test_hook_columns_against_exact(hip_lib, ng):
    """nz 1, 3, 33, 65 at both surface forms: rows at the top, mid-column and the surface; w0 = 0 exactly and 0.99999,
    negative g, a thin layer next to one just above ir_tau_min, tau = 3e4 (make_exact_ir_opr_sens.py lists them)"""
    import test_gpu_golden
    assert K2.FLOOR == test_gpu_golden.TOL                      # the floor is the project's
    E = K.load()
    recs, ran = K.run(hip_lib, E, ng)
    assert ran == K.NCOLUMNS == 14 and len(recs) == 6 * ran
    for r in recs:
        print(("ok   " if r.ok else "FAIL ") + repr(r))
    print("worst error / allowed per parameter:", K.worst_ratios(recs))
    bad = K2.failures(recs)
    assert not bad, bad


def test_hook_results_do_not_depend_on_the_g_point_count_beyond_rounding(hip_lib):
    """the same column at 1 and at 8 g-points (weights summing to 1): the sums over the g-points agree to rounding"""
    E = K.load()
    k = "s06_"
    args = (E[k + "tau"], E[k + "w0"], E[k + "g"], E[k + "bplanck"], E[k + "ir_par"])
    a, e1 = K.ir_opr_sens(hip_lib, *args, 1, E[k + "levels"])
    b, e8 = K.ir_opr_sens(hip_lib, *args, 8, E[k + "levels"])
    assert e1 == "" and e8 == ""
    for name in K.NAMES:
        assert np.allclose(a[name], b[name], rtol=0, atol=8 * np.finfo(float).eps * np.max(np.abs(a[name]))), name


# ------------------------------------------------------------------ the whole call

class Small:
    """nz = 4, ng = 4, a handful of IR bins, particles on (w0 > 0), a hard surface with a per-bin emissivity"""
    NZ, LEVELS = 4, (-1, 2, 0)

    def __init__(self, hard=True):
        from clima_amd import synthetic as S
        self.tables = S.make_tables(**dict(CF._SMALL, **dict(CF._DUSTY, nw=8, ng=4, seed=431)))
        col = CF._column(nz=self.NZ, P_scale=CF.DUSTY_P_SCALE)
        col["pdensities"] = np.asfortranarray(col["pdensities"] * CF.DUSTY_PARTICLES)
        col["radii"] = np.asfortranarray(col["radii"] * CF.DUSTY_RADII)
        self.col, self.hard = col, hard
        self.nw_ir = len(self.tables.ir_wavl) - 1
        self.emissivity = np.linspace(0.6, 1.0, self.nw_ir)
        self.rad = self.handle()
        self.rad.radiate(*col.args())
        self.opr = tuple(np.array(a) for a in self.rad.opr())
        self.start = CF._channel_bins(self.tables, self.tables.ir_wavl)[0]
        self.nsel = len(self.LEVELS)
        self.lv_toa = [self.NZ - (v % (self.NZ + 1)) for v in self.LEVELS]      # ground-first numpy index -> TOA-first level
        self._columns = None

    def handle(self, custom=None):
        from clima_amd.radtran import Radtran
        r = Radtran(self.tables, self.NZ, 1, 0.3)
        r.has_hard_surface = self.hard
        r.ir_tau_min = 1.0e-6
        r.surface_emissivity = self.emissivity
        if custom is not None:
            r.set_custom_optical_properties(*custom)
        return r

    def columns(self):
        """-> per (bin, g-point): (exact, restated) dicts of (nsel, nz) arrays in mpmath / float64, the g-point weights and
        the bins' widths in mpmath; computed once"""
        if self._columns is None:
            self._columns = self._make_columns()
        return self._columns

    def _make_columns(self):
        import mpmath
        tau, w0, g = self.opr[:3]
        nz = self.NZ
        T, Ts = self.col["T"], self.col["T_surface"]
        with mpmath.workdps(X.DPS):
            wg = [CF._mp(w) for w in self.tables.ktables[0]["weights"]]
            freq = CF._freq_mp(self.tables.ir_wavl)
            out = []
            for l in range(self.nw_ir):
                nu = (freq[l] + freq[l + 1]) / 2
                B = [CF.planck(nu, float(T[nz - 1 - i])) for i in range(nz)] + [CF.planck(nu, float(Ts))]
                Bf = [float(b) for b in B]
                row = []
                for i in range(len(wg)):
                    a = (tau[:, i, self.start + l], w0[:, i, self.start + l], g[:, self.start + l], self.emissivity[l], self.hard, 1.0e-6)
                    row.append((X.opr_sens_mp(*a, B, self.lv_toa), X.restated_opr_sens(*a, Bf, self.lv_toa)))
                out.append(row)
            return out, wg, [freq[l] - freq[l + 1] for l in range(self.nw_ir)]


@pytest.fixture(scope="module")
def small():
    return Small()


def _compose(s, cols, wg, width, cot):
    """the gradients of loss = sum over l, a, direction of cot[direction](l, a) x flux, composed in mpmath from the
    per-column derivatives (and, the same way in float64, from the restatement's) -> exact, restated: {name: array in
    opr()'s shape restricted to the IR bins}"""
    import mpmath
    nz, ng, nsel = s.NZ, len(wg), s.nsel
    ex = {"tau": np.zeros((nz, ng, s.nw_ir)), "w0": np.zeros((nz, ng, s.nw_ir)), "g": np.zeros((nz, s.nw_ir))}
    rs = {k: np.zeros_like(v) for k, v in ex.items()}
    with mpmath.workdps(X.DPS):
        for l in range(s.nw_ir):
            for n in range(nz):
                gsum, gsum_r = mpmath.mpf(0), 0.0
                for i in range(ng):
                    e, r = cols[l][i]
                    for p in ("tau", "w0", "g"):
                        v, vr = mpmath.mpf(0), 0.0
                        for a in range(nsel):
                            for d in ("up", "dn"):
                                c = cot(d, l, a, width[l])
                                v += c * e["%s_%s" % (d, p)][a][n]
                                vr += float(c) * r["%s_%s" % (d, p)][a][n]
                        if p == "g":
                            gsum += wg[i] * v
                            gsum_r += float(wg[i]) * vr
                        else:
                            ex[p][n, i, l], rs[p][n, i, l] = float(wg[i] * v), float(wg[i]) * vr
                ex["g"][n, l], rs["g"][n, l] = float(gsum), gsum_r
    return ex, rs


def _hold(s, got, ex, rs, what):
    """per bin and parameter: error <= max(FLOOR x scale, 10 x e_ref); zeros outside the IR channel"""
    ran, worst = 0, {}
    sl = slice(s.start, s.start + s.nw_ir)
    for p in ("tau", "w0", "g"):
        full = got[p]
        outside = np.ones(full.shape[-1], dtype=bool)
        outside[sl] = False
        assert np.all(full[..., outside] == 0.0), (what, p)
        for l in range(s.nw_ir):
            a, x, r = full[..., s.start + l], ex[p][..., l], rs[p][..., l]
            scale, err, e_ref = np.max(np.abs(x)), np.max(np.abs(a - x)), np.max(np.abs(r - x))
            allowed = max(K2.FLOOR * scale, K2.MARGIN * e_ref)
            print("%s bin %d d/d%s: kernel %.2e, reference %.2e of the scale %.2e" % (what, l, p, err / scale, e_ref / scale, scale))
            assert np.isfinite(err) and err <= allowed, (what, p, l, err / scale, e_ref / scale)
            worst[p] = max(worst.get(p, 0.0), err / allowed)
            ran += 1
    assert ran == 3 * s.nw_ir
    return worst


def test_whole_call_against_exact_derivatives(small):
    s = small
    assert s.nw_ir >= 3 and np.any(s.opr[1][:, :, s.start:s.start + s.nw_ir] > 0.1)        # scattering is on in the IR bins
    cols, wg, width = s.columns()
    # unit cotangents on every spectrum, then on the sums over the bins
    grads = dict(fup=np.ones((s.nw_ir, s.nsel)), fdn=np.ones((s.nw_ir, s.nsel)))
    got = s.rad.ir_spectra_opr_vjp(s.col["T_surface"], s.col["T"], grads, s.LEVELS)
    ex, rs = _compose(s, cols, wg, width, lambda d, l, a, wd: 1)
    print(_hold(s, got, ex, rs, "spectra"))
    grads = dict(fup_n=np.ones(s.nsel), fdn_n=np.ones(s.nsel))
    got = s.rad.ir_spectra_opr_vjp(s.col["T_surface"], s.col["T"], grads, s.LEVELS)
    ex, rs = _compose(s, cols, wg, width, lambda d, l, a, wd: wd)
    print(_hold(s, got, ex, rs, "sums"))
    # only what is asked for comes back, and it is the same
    one = s.rad.ir_spectra_opr_vjp(s.col["T_surface"], s.col["T"], grads, s.LEVELS, wrt="w0")
    assert list(one) == ["w0"] and one["w0"].tobytes() == got["w0"].tobytes()


def _state(r):
    out = {"f_total": np.array(r.f_total)}
    for name, w in (("ir", r.wrk_ir), ("sol", r.wrk_sol)):
        for k in ("fup_a", "fdn_a", "fup_n", "fdn_n"):
            out["%s_%s" % (name, k)] = np.array(getattr(w, k))
    for k, a in zip(("tau", "w0", "g", "tau_band"), r.opr()):
        out["opr_" + k] = np.array(a)
    return out


def test_whole_call_contract(small):
    """host and device forms agree bit for bit, two calls agree bit for bit, zero cotangents give exact zeros, fdn at the top
    gives exactly 0, the handle's rows, spectra and optical properties are unchanged, the gradient is linear in the
    cotangents, and the temperature gradient for the same cotangents is what it was"""
    import torch
    s, r = small, small.rad
    Ts, T = s.col["T_surface"], s.col["T"]
    rng = np.random.default_rng(5)
    g1 = {k: rng.uniform(-1.0, 1.0, (s.nsel,) if k.endswith("_n") else (s.nw_ir, s.nsel)) for k in GRADS}
    g1["fup_n"] *= 1e-12
    g1["fdn_n"] *= 1e-12                           # (the widths are 1e12 Hz: both kinds of cotangent weigh the same)
    g2 = {k: rng.uniform(-1.0, 1.0, v.shape) * (1e-12 if k.endswith("_n") else 1.0) for k, v in g1.items()}
    w = r.ir_spectra_batch(None, None, s.LEVELS, ("up", "dn"), weights=True)
    w = {k: w[k] for k in ("w_up", "w_dn")}
    gT = lambda: r.ir_spectra_vjp(Ts, T, w, {k: v[..., None] for k, v in g1.items()})   # noqa: E731
    before, gT_before = _state(r), gT()
    a = r.ir_spectra_opr_vjp(Ts, T, g1, s.LEVELS)
    b = r.ir_spectra_opr_vjp(Ts, T, g1, s.LEVELS)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")   # noqa: E731
    d = r.ir_spectra_opr_vjp_tensors(dev([Ts]), dev(T), {k: dev(v.T) for k, v in g1.items()}, s.LEVELS, sync=True)
    for k in ("tau", "w0", "g"):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert np.ascontiguousarray(d[k].cpu().numpy().T).tobytes() == np.ascontiguousarray(a[k]).tobytes(), k
        assert np.all(np.isfinite(a[k])) and np.any(a[k] != 0.0)
    after = _state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    gT_after = gT()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(gT_before, gT_after))
    z = r.ir_spectra_opr_vjp(Ts, T, {k: np.zeros_like(v) for k, v in g1.items()}, s.LEVELS)
    assert all(np.all(z[k] == 0.0) for k in z)
    top = r.ir_spectra_opr_vjp(Ts, T, dict(fdn=np.ones((s.nw_ir, 1)), fdn_n=np.ones(1)), (-1,))
    assert all(np.all(top[k] == 0.0) for k in top)
    # linear in the cotangents, exactly where floating point is: a factor 2 on every cotangent doubles every element bit
    # for bit (the cotangents enter one right-hand side and the direct terms, all linear; a power of two rounds nowhere),
    # and cotangents on two disjoint sets of bins give, added, the result of their sum bit for bit (a bin's gradient reads
    # its own cotangents alone; the other call leaves exact zeros there)
    twice = r.ir_spectra_opr_vjp(Ts, T, {k: 2.0 * v for k, v in g1.items()}, s.LEVELS)
    lo, hi = {k: v.copy() for k, v in g1.items() if not k.endswith("_n")}, {k: v.copy() for k, v in g1.items() if not k.endswith("_n")}
    for k in lo:
        lo[k][s.nw_ir // 2:, :] = 0.0
        hi[k][:s.nw_ir // 2, :] = 0.0
    spec = r.ir_spectra_opr_vjp(Ts, T, {k: lo[k] + hi[k] for k in lo}, s.LEVELS)
    part_lo, part_hi = r.ir_spectra_opr_vjp(Ts, T, lo, s.LEVELS), r.ir_spectra_opr_vjp(Ts, T, hi, s.LEVELS)
    for k in ("tau", "w0", "g"):
        assert twice[k].tobytes() == (2.0 * a[k]).tobytes(), k
        assert np.array_equal(part_lo[k] + part_hi[k], spec[k]) and np.any(part_lo[k] != 0.0) and np.any(part_hi[k] != 0.0), k
    # ... and additive within a bin to the accuracy of the results: g1 + g2 against the sum of the two results.  Each of
    # the three is the same linear map of its cotangents in float64, and is held by the accuracy tests to max(FLOOR x scale, 10 x e_ref) -- here on the scale of
    # the TERMS it adds up (they cancel): per bin and parameter, scale = the largest element of  sum over (level, direction)
    # of |cotangent| x |the gradient of that unit cotangent|,  e_ref = the same sum over the reference restatement's errors
    # on those unit gradients.  Three results: three times that bound.
    c = r.ir_spectra_opr_vjp(Ts, T, g2, s.LEVELS)
    both = r.ir_spectra_opr_vjp(Ts, T, {k: g1[k] + g2[k] for k in g1}, s.LEVELS)
    width = np.abs(np.diff(np.asarray(r.ir.freq, dtype=float)))
    sl = slice(s.start, s.start + s.nw_ir)
    cols, wg, width_mp = s.columns()
    terms = {k: np.zeros_like(a[k][..., sl]) for k in a}
    e_terms = {k: np.zeros_like(a[k][..., sl]) for k in a}
    for ai in range(s.nsel):
        for d in ("up", "dn"):
            unit = np.zeros((s.nw_ir, s.nsel))
            unit[:, ai] = 1.0
            G = r.ir_spectra_opr_vjp(Ts, T, {"f" + d: unit}, s.LEVELS)
            ex, rs = _compose(s, cols, wg, width_mp, lambda dd, l, a_, wd: 1 if (dd == d and a_ == ai) else 0)
            mag = (np.abs(g1["f" + d][:, ai]) + np.abs(g2["f" + d][:, ai])
                   + (abs(g1["f%s_n" % d][ai]) + abs(g2["f%s_n" % d][ai])) * width)
            for k in terms:
                terms[k] += mag * np.abs(G[k][..., sl])
                e_terms[k] += mag * np.abs(rs[k] - ex[k])
    for k in ("tau", "w0", "g"):
        flat = lambda x: x.reshape(-1, x.shape[-1]).max(axis=0)   # noqa: E731
        scale, e_ref = flat(terms[k]), flat(e_terms[k])
        diff = flat(np.abs(both[k] - (a[k] + c[k])))
        allowed = 3.0 * np.maximum(K2.FLOOR * scale, K2.MARGIN * e_ref)
        print("linearity d/d%s: largest difference / allowed per bin %s" % (k, np.array2string(diff[sl] / allowed, precision=2)))
        assert np.all(scale > 0) and np.all(diff[sl] <= allowed), k
        assert np.all(np.delete(diff, np.arange(sl.start, sl.stop)) == 0.0), k


def test_wiring_through_the_opacity_step(small):
    """A uniform grey absorber through set_custom_optical_properties (dtau_dz = c0, w0 = 0): the central difference of
    fup_a at the top over c0 (1 +- 1e-5) equals sum_n dz_n x the grey absorption sensitivity of `grey_sensitivity`, within
    1e-6 of the spectrum's largest derivative (truncation 1e-10, rounding eps / 1e-5 = 2e-11: three orders of margin,
    and any slip in layer order, bin order or g-weights is orders above it)"""
    from clima_amd.radtran import grey_sensitivity
    s = small
    sl = slice(s.start, s.start + s.nw_ir)
    dz = np.asarray(s.col["dz"], dtype=float)
    c0 = float(np.median(s.opr[0][:, :, sl])) / float(dz[0])          # the added depth is comparable to the layers' own
    wv, P = np.array([50.0, 5.0e6]), np.array([1.0e8, 1.0e-6])
    custom = lambda c: (wv, P, np.full((2, 2), c), np.zeros((2, 2)), np.zeros((2, 2)))   # noqa: E731
    r = s.handle(custom(c0))
    r.radiate(*s.col.args(), compute_solar=False)
    opr = tuple(np.array(a) for a in r.opr())
    assert np.median(opr[0][:, :, sl]) > 1.5 * np.median(s.opr[0][:, :, sl])
    grads = r.ir_spectra_opr_vjp(s.col["T_surface"], s.col["T"], dict(fup=np.ones((s.nw_ir, 1))), (-1,), ("tau", "w0"))
    ab, _ = grey_sensitivity(opr, grads, 1.0e-20, 0.99999)
    pred = (dz[::-1, None] * ab[:, sl]).sum(axis=0)                   # opr() is TOA-first, dz ground-first
    top = []
    for f in (1.0 + 1.0e-5, 1.0 - 1.0e-5):
        r.set_custom_optical_properties(*custom(c0 * f))
        r.radiate(*s.col.args(), compute_solar=False)
        top.append(np.array(r.wrk_ir.fup_a)[-1, :].copy())
    fd = (top[0] - top[1]) / (2.0e-5 * c0)
    print("wiring: largest |fd - pred| / largest |pred| = %.2e" % (np.max(np.abs(fd - pred)) / np.max(np.abs(pred))))
    assert np.max(np.abs(pred)) > 0 and np.max(np.abs(fd - pred)) <= 1.0e-6 * np.max(np.abs(pred))


def test_whole_call_without_a_hard_surface():
    """the no-hard-surface form of the whole call against exact, on the same small case"""
    s = Small(hard=False)
    cols, wg, width = s.columns()
    grads = dict(fup=np.ones((s.nw_ir, s.nsel)), fdn=np.ones((s.nw_ir, s.nsel)))
    got = s.rad.ir_spectra_opr_vjp(s.col["T_surface"], s.col["T"], grads, s.LEVELS)
    ex, rs = _compose(s, cols, wg, width, lambda d, l, a, wd: 1)
    print(_hold(s, got, ex, rs, "no hard surface"))


# ------------------------------------------------------------------ refusals on a constructed handle

def test_refusals_name_the_argument_and_write_nothing(small, hip_lib):
    import torch
    s, r, L = small, small.rad, hip_lib
    nz, nl, nw_ir = s.NZ, s.NZ + 1, s.nw_ir
    err = C.create_string_buffer(1025)
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    host = dict(Ts=np.array([float(s.col["T_surface"])]), T=np.ascontiguousarray(s.col["T"], dtype=np.float64), fup=np.ones((nw_ir, 2)),
                fdn=np.ones((nw_ir, 2)), fup_n=np.ones(2), fdn_n=np.ones(2), tau=np.full(s.opr[0].size, 7.0), w0=np.full(s.opr[0].size, 7.0),
                g=np.full(s.opr[2].size, 7.0))
    dev = {k: torch.tensor(v, dtype=torch.float64, device="cuda") for k, v in host.items()}
    lv = np.array([nl, 1], dtype=np.int32)
    before = _state(r)

    def call(form, dim=nz, nsel=2, level=lv, skip=(), swap=None, handle=None):
        src = host if form == "host" else dev

        def p(k):
            if k in skip:
                return None
            a = host[k] if k == swap else src[k]
            if form == "host":
                return a.ctypes.data_as(DP)
            return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        args = [handle or r._ptr, p("Ts"), i(dim), p("T"), i(nsel), level.ctypes.data_as(IP) if level is not None else None, p("fup"), p("fdn"),
                p("fup_n"), p("fdn_n"), p("tau"), p("w0"), p("g")]
        if form == "host":
            L.radtran_ir_spectra_opr_vjp(*args, err)
        else:
            L.radtran_ir_spectra_opr_vjp_device(*args, None, err)
        return err.value.decode()

    for form, who in (("host", "ir_spectra_opr_vjp: "), ("device", "ir_spectra_opr_vjp_device: ")):
        assert call(form, dim=nz - 1) == who + '"T" has the dimension %d, not nz = %d' % (nz - 1, nz)
        assert call(form, nsel=0) == who + "nsel must be at least 1 (nsel = 0)"
        assert call(form, level=None) == who + '"spec_level" is a required argument'
        assert call(form, level=np.array([1, nl + 1], dtype=np.int32)) == who + "spec_level(2) = %d is outside 1..%d" % (nl + 1, nl)
        assert call(form, level=np.array([0, 1], dtype=np.int32)) == who + "spec_level(1) = 0 is outside 1..%d" % nl
        assert call(form, skip=GRADS) == who + "none of g_ir_fup, g_ir_fdn, g_fup_n, g_fdn_n was given"
        assert call(form, skip=("tau", "w0", "g")) == who + "none of grad_tau, grad_w0, grad_g was given"
        assert call(form, skip=("T",)) == who + '"T" is a required argument'
        assert call(form, skip=("Ts",)) == who + '"T_surface" is a required argument'
    for name, arg in (("T", "T"), ("T_surface", "Ts"), ("g_ir_fup", "fup"), ("g_fdn_n", "fdn_n"), ("grad_tau", "tau"), ("grad_g", "g")):
        assert call("device", swap=arg) == 'ir_spectra_opr_vjp_device: "%s" is not device memory of this handle\'s device' % name
    good = host["T"].copy()
    host["T"][2] = -5.0
    assert call("host").startswith("ir_spectra_opr_vjp: temperatures must be finite and positive (T(3) = -5.0")
    host["T"][:] = good
    host["Ts"][0] = float("nan")
    assert call("host").startswith("ir_spectra_opr_vjp: temperatures must be finite and positive (T_surface = nan")
    host["Ts"][0] = float(s.col["T_surface"])
    sh = s.handle()
    sh.radiate(*s.col.args())
    sh.set_bin_shard(0, 2)
    fresh = s.handle()
    for form, who in (("host", "ir_spectra_opr_vjp"), ("device", "ir_spectra_opr_vjp_device")):
        assert call(form, handle=sh._ptr) == who + ": needs the whole spectrum (a bin shard of 2)"
        assert call(form, handle=fresh._ptr) == who + " needs opacities: call radiate with compute_opacity first"
    r.synchronize()
    assert all(np.all(host[k] == 7.0) and bool((dev[k] == 7.0).all()) for k in ("tau", "w0", "g"))      # nothing was written
    after = _state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert call("host") == "" and call("device") == ""                # the handle is usable afterwards
    r.synchronize()
    assert not np.any(host["tau"] == 7.0) and not bool((dev["tau"] == 7.0).any())
    assert dev["tau"].cpu().numpy().tobytes() == host["tau"].tobytes()
