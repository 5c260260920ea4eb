"""The gradient of the solar spectra in the stored optical properties and the surface albedo on the GPU:
clima_test_sol_opr_sens (k_sol_opr_adjoint and k_sol_opr_sum_g of clima_amd/csrc/sol_opr_sens.inc, one launch of the
production kernels) column by column against exact derivatives, and radtran_sol_spectra_opr_vjp / _device as a whole call.

Exact: tests/exact_sol_opr_sens.py (mpmath, 80 digits, central differences with h = 1e-30, rounded once) -- stored for the
hook's columns (tests/golden/exact_sol_opr_sens_0.npz), computed live per (bin, g-point) from `opr()` and the handle's
fields for the whole call and composed over the levels, the g-points and the unit factors in mpmath.  The criterion is
exact_two_stream_cases': kernel error <= max(FLOOR x scale, MARGIN x e_ref) per column and derivative array, e_ref the error
of the reference algorithm's float64 restatement (autograd) on that array.  No column is left out; every test asserts how
many it ran.

Measured on an MI355X (tools/gpu_sol_opr_sens.py; profiles/sol_opr_sens.txt is its output): on the fourteen columns, at 1
and at 8 g-points alike, the largest kernel error over the allowed error is 4.4e-3 for d/dtau, 0.42 for d/dw0, 0.42 for
d/dg and 1.7e-4 for d/drsfc; all 21 identically-zero arrays come back as zeros.  (d fdn / d rsfc of the two columns without
any scattering, s02 (nz 2) and s09 (nz 33), is among them: there the kernel solves the surface row's lambda from the upward
cotangents alone, sol_opr_sens.inc's step 2.  Solved from the whole right-hand side it is the rounding of a sum that
cancels: the kernel then gave 4.9e-17 on s02 and 4.2e-24 on s09, the reference's float64 restatement gives 2.0e-17 and
6.4e-25, the `reference` column of the profile.)
"""
import ctypes as C

import numpy as np
import pytest

import closed_forms as CF
import exact_sol_opr_sens as X
import exact_two_stream_cases as K2
import sol_opr_sens_cases as K

pytestmark = pytest.mark.gpu
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
GRADS = ("fup", "fdn", "amean", "fup_n", "fdn_n")
WRT = ("tau", "w0", "g", "albedo")


# ------------------------------------------------------------------ the hook, column by column

@pytest.fixture(scope="module")
def hook_runs(hip_lib):
    E = K.load()
    return {ng: K.run(hip_lib, E, ng) for ng in (1, 8)}


@pytest.mark.parametrize("ng", [1, 8])
def test_hook_columns_against_exact(hook_runs, ng):
    """nz 1 .. 129 (segments of 64 crossed), Rsfc 0 and 1, negative g, w0 = 0 throughout and at the cap, tau = 0 and 3e4, 1
    and 4 zenith angles, a grazing angle, |lambda u0 - 1| = 1e-3 (make_exact_sol_opr_sens.py lists them)"""
    import test_gpu_golden
    assert K2.FLOOR == test_gpu_golden.TOL and K2.MARGIN == 10.0
    recs, ran, _ = hook_runs[ng]
    assert ran == K.NCOLUMNS == 14 and len(recs) == 12 * ran
    for r in recs:
        print(("ok   " if r.ok else "FAIL ") + repr(r))
    print("worst error / allowed per parameter:", K.worst_ratios(recs))
    bad = K2.failures(recs)
    assert not bad, bad


@pytest.mark.parametrize("ng", [1, 8])
def test_hook_identically_zero_arrays_come_back_as_zeros(hook_runs, ng):
    """an array whose exact derivative is 0 everywhere (fdn at the top, d/dg without scattering, fup over a black surface
    without scattering, the surface under an opaque layer ...) must be zeros, not small numbers"""
    E = K.load()
    zero = [k for k in E if k[4:] in K.NAMES and not np.any(E[k] != 0.0)]
    assert len(zero) >= 20                       # (the set is not empty: the columns above make many)
    _, _, nonzero = hook_runs[ng]
    print("identically-zero arrays: %d, not zeros from the kernel: %s" % (len(zero), nonzero))
    assert not nonzero, nonzero


def test_hook_results_do_not_depend_on_the_g_point_count_beyond_rounding(hip_lib):
    E = K.load()
    k = "s07_"
    args = tuple(E[k + x] for x in ("tau", "w0", "g", "zen_u", "zen_w", "rsfc"))
    a, e1 = K.sol_opr_sens(hip_lib, *args, 1, E[k + "levels"])
    b, e8 = K.sol_opr_sens(hip_lib, *args, 8, E[k + "levels"])
    assert e1 == "" and e8 == ""
    for name in K.NAMES:
        assert np.allclose(a[name], b[name], rtol=0, atol=8 * np.finfo(float).eps * np.max(np.abs(a[name]))), name


# ------------------------------------------------------------------ the whole call

class Small:
    """nz = 8, ng = 4, a handful of solar bins, Rayleigh scattering by every species over one weak k-species (closed_forms'
    "rayleigh" kind: light reaches the ground and w0 runs up to the cap), two zenith angles, a per-bin albedo.  (The dusty
    column of test_gpu_ir_opr_sens.py's fixture is opaque in the solar bins: every derivative underflows there.)"""
    NZ, NZEN, LEVELS = 8, 2, (-1, 3, 0)

    def __init__(self):
        from clima_amd import synthetic as S
        self.tables = S.make_tables(**dict(CF._SMALL, **dict(CF._RAYLEIGH, nw=8, ng=4, seed=431)))
        col = CF._column(nz=self.NZ, n_particles=0)
        self.col = col
        self.nw_sol = len(self.tables.sol_wavl) - 1
        self.albedo = np.linspace(0.05, 0.8, self.nw_sol)
        self.rad = self.handle()
        self.rad.radiate(*col.args())
        self.opr = tuple(np.array(a) for a in self.rad.opr())
        self.start = CF._channel_bins(self.tables, self.tables.sol_wavl)[0]
        self.nsel = len(self.LEVELS)
        self.lv_toa = [self.NZ - (v % (self.NZ + 1)) for v in self.LEVELS]      # ground-first numpy index -> TOA-first level
        self.zen_u, self.zen_w = np.array(self.rad.zenith_u), np.array(self.rad.zenith_weights)
        self._columns = None

    def handle(self):
        from clima_amd.radtran import Radtran
        r = Radtran(self.tables, self.NZ, self.NZEN, 0.3)
        r.surface_albedo = self.albedo
        r.photon_scale_factor = 0.75
        return r

    def columns(self):
        """-> per (bin, g-point): (exact, restated) dicts in mpmath / float64, the g-point weights, the bins' widths and
        the two unit factors (of fup / fdn, of amean) per bin in mpmath; computed once"""
        if self._columns is None:
            self._columns = self._make_columns()
        return self._columns

    def _make_columns(self):
        import mpmath
        tau, w0, g = self.opr[:3]
        t, r = self.tables, self.rad
        with mpmath.workdps(X.DPS):
            wg = [CF._mp(w) for w in t.ktables[0]["weights"]]
            freq = CF._freq_mp(t.sol_wavl)
            c, h = mpmath.mpf(CF.C_LIGHT), mpmath.mpf(CF.PLANK)
            out, fs, fa = [], [], []
            for l in range(self.nw_sol):
                row = []
                for i in range(len(wg)):
                    a = (tau[:, i, self.start + l], w0[:, i, self.start + l], g[:, self.start + l], self.zen_u, self.zen_w, self.albedo[l])
                    row.append((X.sol_opr_sens_mp(*a, self.lv_toa), X.restated_sol_opr_sens(*a, self.lv_toa)))
                out.append(row)
                scale = CF._mp(t.photons_sol[l]) * CF._mp(r.photon_scale_factor) * CF._mp(r.diurnal_fac)      # radiate.f90:169-171
                avg_freq = (freq[l] + freq[l + 1]) / 2
                avg_wavl = mpmath.mpf("1e9") * c / avg_freq
                fs.append(scale)                                                                          # :173-178
                fa.append(scale * (avg_freq / avg_wavl) * (avg_wavl / (h * c * mpmath.mpf("1e16"))) * (CF._mp(t.sol_wavl[l + 1]) - CF._mp(t.sol_wavl[l])))
            return out, wg, [freq[l] - freq[l + 1] for l in range(self.nw_sol)], fs, fa


@pytest.fixture(scope="module")
def small():
    return Small()


def _compose(s, grads):
    """the gradients of loss = sum over l, a of the cotangents x the call's outputs, composed in mpmath from the per-column
    derivatives (and, the same way in float64, from the restatement's) -> exact, restated: {name: array in opr()'s shape
    restricted to the solar bins, "albedo": (nw_sol,)}"""
    import mpmath
    cols, wg, width, fs, fa = s.columns()
    nz, ng, nsel, nw = s.NZ, len(wg), s.nsel, s.nw_sol
    ex = {"tau": np.zeros((nz, ng, nw)), "w0": np.zeros((nz, ng, nw)), "g": np.zeros((nz, nw)), "albedo": np.zeros(nw)}
    rs = {k: np.zeros_like(v) for k, v in ex.items()}
    zero = np.zeros((nw, nsel))
    gs = {k: np.asarray(grads.get(k, zero), dtype=np.float64) for k in ("fup", "fdn", "amean")}
    gn = {k: np.asarray(grads.get(k, np.zeros(nsel)), dtype=np.float64) for k in ("fup_n", "fdn_n")}
    with mpmath.workdps(X.DPS):
        for l in range(nw):
            # the cotangent of each of the three per-(bin, g-point) functions at level a, in mpmath
            cot = [{"up": (CF._mp(gs["fup"][l, a]) + CF._mp(gn["fup_n"][a]) * width[l]) * fs[l],
                    "dn": (CF._mp(gs["fdn"][l, a]) + CF._mp(gn["fdn_n"][a]) * width[l]) * fs[l],
                    "am": CF._mp(gs["amean"][l, a]) * fa[l]} for a in range(nsel)]

            def total(e, r, p, n):
                v, vr = mpmath.mpf(0), 0.0
                for a in range(nsel):
                    for q in X.QUANTITIES:
                        x, xr = e["%s_%s" % (q, p)][a], r["%s_%s" % (q, p)][a]
                        v += cot[a][q] * (x if n is None else x[n])
                        vr += float(cot[a][q]) * float(xr if n is None else xr[n])
                return v, vr
            asum, asum_r = mpmath.mpf(0), 0.0
            for i in range(ng):
                e, r = cols[l][i]
                v, vr = total(e, r, "rsfc", None)
                asum += wg[i] * v
                asum_r += float(wg[i]) * vr
            ex["albedo"][l], rs["albedo"][l] = float(asum), asum_r
            for n in range(nz):
                gsum, gsum_r = mpmath.mpf(0), 0.0
                for i in range(ng):
                    e, r = cols[l][i]
                    for p in ("tau", "w0", "g"):
                        v, vr = total(e, r, p, n)
                        if p == "g":
                            gsum += wg[i] * v
                            gsum_r += float(wg[i]) * vr
                        else:
                            ex[p][n, i, l], rs[p][n, i, l] = float(wg[i] * v), float(wg[i]) * vr
                ex["g"][n, l], rs["g"][n, l] = float(gsum), gsum_r
    return ex, rs


def _hold(s, got, ex, rs, what):
    """per bin and parameter: error <= max(FLOOR x scale, MARGIN x e_ref); zeros outside the solar channel"""
    ran, worst = 0, {}
    sl = slice(s.start, s.start + s.nw_sol)
    for p in WRT:
        full = got[p]
        if p != "albedo":
            outside = np.ones(full.shape[-1], dtype=bool)
            outside[sl] = False
            assert np.all(full[..., outside] == 0.0), (what, p)
        for l in range(s.nw_sol):
            a = full[l] if p == "albedo" else full[..., s.start + l]
            x, r = ex[p][..., l], rs[p][..., l]
            scale, err, e_ref = np.max(np.abs(x)), np.max(np.abs(a - x)), np.max(np.abs(r - x))
            allowed = max(K2.FLOOR * scale, K2.MARGIN * e_ref)
            print("%s bin %d d/d%s: kernel %.2e, reference %.2e of the scale %.2e" % (what, l, p, err / scale, e_ref / scale, scale))
            assert np.isfinite(err) and err <= allowed, (what, p, l, err / scale, e_ref / scale)
            worst[p] = max(worst.get(p, 0.0), err / allowed)
            ran += 1
    assert ran == 4 * s.nw_sol
    return worst


def _random_grads(s, seed):
    """random cotangents on all five quantities; those of the sums weigh what the spectra's do (the widths are ~1e14 Hz)"""
    rng = np.random.default_rng(seed)
    g = {k: rng.uniform(-1.0, 1.0, (s.nsel,) if k.endswith("_n") else (s.nw_sol, s.nsel)) for k in GRADS}
    width = np.abs(np.diff(np.asarray(s.rad.sol.freq, dtype=float)))
    g["fup_n"] /= np.max(width)
    g["fdn_n"] /= np.max(width)
    return g


def test_whole_call_against_exact_derivatives(small):
    s = small
    assert s.nw_sol >= 3 and np.any(s.opr[1][:, :, s.start:s.start + s.nw_sol] > 0.1)        # scattering is on in the solar bins
    grads = _random_grads(s, 11)
    got = s.rad.sol_spectra_opr_vjp(grads, s.LEVELS)
    ex, rs = _compose(s, grads)
    print(_hold(s, got, ex, rs, "all five"))
    # only what is asked for comes back, and it is the same
    one = s.rad.sol_spectra_opr_vjp(grads, s.LEVELS, wrt=("albedo", "w0"))
    assert list(one) == ["w0", "albedo"] and all(one[k].tobytes() == got[k].tobytes() for k in one)


def test_directional_check_against_the_librarys_own_forward(small):
    """central differences of radiate_solar_batch in the albedo along a random direction against grad_albedo . d_albedo.  The
    difference quotient's own error is measured against the exact directional derivative first; ten times that is allowed."""
    s, r = small, small.rad
    grads = {k: v for k, v in _random_grads(s, 12).items() if not k.endswith("_n")}
    rng = np.random.default_rng(13)
    da = rng.uniform(-1.0, 1.0, s.nw_sol)
    eps = 1.0e-4
    lv = list(s.LEVELS)
    spec = r.radiate_solar_batch(np.tile(s.zen_u, (2, 1)), np.tile(s.zen_w, (2, 1)), np.stack([s.albedo + eps * da, s.albedo - eps * da]),
                                 spectra_levels=lv)[3]
    loss = [sum(float(np.sum(grads[k].T * spec[k][:, :, c])) for k in ("fup", "fdn", "amean")) for c in (0, 1)]
    fd = (loss[0] - loss[1]) / (2.0 * eps)
    got = float(np.dot(r.sol_spectra_opr_vjp(grads, s.LEVELS, wrt="albedo")["albedo"], da))
    exact = float(np.dot(_compose(s, grads)[0]["albedo"], da))
    e_q = abs(fd - exact)
    print("directional: fd %.12e, exact %.12e, call %.12e; quotient's own error %.2e, |fd - call| %.2e" % (fd, exact, got, e_q, abs(fd - got)))
    assert exact != 0.0 and fd != 0.0 and abs(fd - exact) < 1.0e-3 * abs(exact)      # (the quotient sees the albedo at all)
    assert abs(fd - got) <= 10.0 * e_q


def _state(r):
    out = {"f_total": np.array(r.f_total)}
    for name, w in (("ir", r.wrk_ir), ("sol", r.wrk_sol)):
        for k in ("fup_a", "fdn_a", "fup_n", "fdn_n"):
            out["%s_%s" % (name, k)] = np.array(getattr(w, k))
    out["sol_amean"] = np.array(r.wrk_sol.amean)
    for k, a in zip(("tau", "w0", "g", "tau_band"), r.opr()):
        out["opr_" + k] = np.array(a)
    return out


def test_whole_call_contract(small):
    import torch
    s, r = small, small.rad
    g1 = _random_grads(s, 5)
    before = _state(r)
    a = r.sol_spectra_opr_vjp(g1, s.LEVELS)
    b = r.sol_spectra_opr_vjp(g1, s.LEVELS)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")   # noqa: E731
    d = r.sol_spectra_opr_vjp_tensors({k: dev(v.T) for k, v in g1.items()}, s.LEVELS, sync=True)
    for k in WRT:
        assert a[k].tobytes() == b[k].tobytes(), k                                  # bitwise repeat
        assert np.ascontiguousarray(d[k].cpu().numpy().T).tobytes() == np.ascontiguousarray(a[k]).tobytes(), k   # host = device
        assert np.all(np.isfinite(a[k])) and np.any(a[k] != 0.0)
    after = _state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k                         # the handle's state is unchanged
    z = r.sol_spectra_opr_vjp({k: np.zeros_like(v) for k, v in g1.items()}, s.LEVELS)
    assert all(np.all(z[k] == 0.0) for k in z)                                      # zero cotangents: exact zeros
    top = r.sol_spectra_opr_vjp(dict(fdn=np.ones((s.nw_sol, 1)), fdn_n=np.ones(1)), (-1,))
    assert all(np.all(top[k] == 0.0) for k in top)                                  # fdn at level nz+1 is u0
    # a cotangent on one bin leaves the others exactly zero
    one = {k: np.zeros_like(v) for k, v in g1.items() if not k.endswith("_n")}
    for k in one:
        one[k][1, :] = g1[k][1, :]
    o = r.sol_spectra_opr_vjp(one, s.LEVELS)
    keep = s.start + 1
    for k in ("tau", "w0", "g"):
        assert np.any(o[k][..., keep] != 0.0) and np.all(np.delete(o[k], keep, axis=-1) == 0.0), k
    assert o["albedo"][1] != 0.0 and np.all(np.delete(o["albedo"], 1) == 0.0)
    # levels in any order and with repeats equal the summed cotangents: (2, -1, 2) with c1, c2, c3 against (-1, 2) with c2, c1 + c3
    c = [np.random.default_rng(20 + j).uniform(-1.0, 1.0, s.nw_sol) for j in range(3)]
    rep = r.sol_spectra_opr_vjp(dict(fup=np.stack(c, axis=1)), (2, -1, 2))
    summed = r.sol_spectra_opr_vjp(dict(fup=np.stack([c[1], c[0] + c[2]], axis=1)), (-1, 2))
    for k in WRT:
        scale = np.max(np.abs(summed[k]))
        assert np.max(np.abs(rep[k] - summed[k])) <= 64 * np.finfo(float).eps * scale, k      # (the sum of two cotangents rounds once more)
    # g_fup_n equals g_sol_fup = g_n x width, bit for bit
    width = np.asarray(r.sol.freq, dtype=float)[:-1] - np.asarray(r.sol.freq, dtype=float)[1:]
    gn = np.array([0.3, -1.7, 0.9])
    assert len(gn) == s.nsel
    by_n = r.sol_spectra_opr_vjp(dict(fup_n=gn, fdn_n=0.5 * gn), s.LEVELS)
    by_s = r.sol_spectra_opr_vjp(dict(fup=width[:, None] * gn[None, :], fdn=width[:, None] * (0.5 * gn)[None, :]), s.LEVELS)
    for k in WRT:
        assert by_n[k].tobytes() == by_s[k].tobytes(), k


def test_the_call_works_with_a_deferred_integration_pending(small):
    """A pipelined `radiate_resident` keeps its integration back (`defer_integration`), and with `calls_in_flight = 2` the
    second of two such calls runs on the other slot, not yet joined: the gradient call settles both first.  Per setting a
    handle that defers and one that does not: the gradient is the settled handle's bit for bit, and after `synchronize` the
    two handles hold the same rows and spectra, which are the ones a plain `radiate` leaves."""
    from test_gpu_merged_integration import _assert_same_state
    s = small
    g1 = _random_grads(s, 6)
    ref = s.rad.sol_spectra_opr_vjp(g1, s.LEVELS)
    want = _state(s.rad)
    for in_flight in (1, 2):
        pair = []
        for defer in (True, False):
            h = s.handle()
            h.defer_integration = defer
            h.calls_in_flight = in_flight
            for _ in range(in_flight):
                h.upload_column(*s.col.args())
                h.radiate_resident()
            # (two in flight, which takes deferral: the second call took the other slot and nobody has joined it yet)
            assert h.overlapped_calls == (in_flight - 1 if defer else 0), (in_flight, defer)
            got = h.sol_spectra_opr_vjp(g1, s.LEVELS)
            for k in WRT:
                assert got[k].tobytes() == ref[k].tobytes(), (in_flight, defer, k)
            h.synchronize()
            pair.append(h)
        _assert_same_state(pair[0], pair[1], "deferring against not, the solar gradient in between (in flight: %d)" % in_flight)
        for h in pair:
            for k, v in _state(h).items():
                assert v.tobytes() == want[k].tobytes(), (in_flight, k)


# ------------------------------------------------------------------ refusals on a constructed handle

def test_refusals_name_the_argument_and_write_nothing(small, hip_lib):
    import torch
    s, r, L = small, small.rad, hip_lib
    nl, nw_sol = s.NZ + 1, s.nw_sol
    err = C.create_string_buffer(1025)
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    nan = float("nan")
    host = dict(fup=np.ones((nw_sol, 2)), fdn=np.ones((nw_sol, 2)), amean=np.ones((nw_sol, 2)), fup_n=np.ones(2), fdn_n=np.ones(2),
                tau=np.full(s.opr[0].size, nan), w0=np.full(s.opr[0].size, nan), g=np.full(s.opr[2].size, nan), albedo=np.full(nw_sol, nan))
    dev = {k: torch.tensor(v, dtype=torch.float64, device="cuda") for k, v in host.items()}
    lv = np.array([nl, 1], dtype=np.int32)
    before = _state(r)
    OUT = ("tau", "w0", "g", "albedo")

    def call(form, nsel=2, level=lv, skip=(), swap=None, handle=None):
        src = host if form == "host" else dev

        def p(k):
            if k in skip:
                return None
            a = host[k] if k == swap else src[k]
            if form == "host":
                return a.ctypes.data_as(DP)
            return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        args = [handle or r._ptr, i(nsel), level.ctypes.data_as(IP) if level is not None else None] + [p(k) for k in GRADS + OUT]
        if form == "host":
            L.radtran_sol_spectra_opr_vjp(*args, err)
        else:
            L.radtran_sol_spectra_opr_vjp_device(*args, None, err)
        return err.value.decode()

    for form, who in (("host", "sol_spectra_opr_vjp: "), ("device", "sol_spectra_opr_vjp_device: ")):
        assert call(form, nsel=0) == who + "nsel must be at least 1 (nsel = 0)"
        assert call(form, level=None) == who + '"spec_level" is a required argument'
        assert call(form, level=np.array([1, nl + 1], dtype=np.int32)) == who + "spec_level(2) = %d is outside 1..%d" % (nl + 1, nl)
        assert call(form, level=np.array([0, 1], dtype=np.int32)) == who + "spec_level(1) = 0 is outside 1..%d" % nl
        assert call(form, skip=GRADS) == who + "none of g_sol_fup, g_sol_fdn, g_sol_amean, g_fup_n, g_fdn_n was given"
        assert call(form, skip=OUT) == who + "none of grad_tau, grad_w0, grad_g, grad_albedo was given"
    for name, arg in (("g_sol_fup", "fup"), ("g_sol_amean", "amean"), ("g_fdn_n", "fdn_n"), ("grad_tau", "tau"), ("grad_g", "g"),
                      ("grad_albedo", "albedo")):
        assert call("device", swap=arg) == 'sol_spectra_opr_vjp_device: "%s" is not device memory of this handle\'s device' % name
    sh = s.handle()
    sh.radiate(*s.col.args())
    sh.set_bin_shard(0, 2)
    fresh = s.handle()
    for form, who in (("host", "sol_spectra_opr_vjp"), ("device", "sol_spectra_opr_vjp_device")):
        assert call(form, handle=sh._ptr) == who + ": needs the whole spectrum (a bin shard of 2)"
        assert call(form, handle=fresh._ptr) == who + " needs opacities: call radiate with compute_opacity first"
    # a handle without solar bins cannot be made: the constructor refuses tables whose solar channel is empty, so the
    # call's own refusal of such a handle (sol_opr_handle_refused, ahead of the opacity check) stays a guard that no caller
    # can reach; the work buffer's bound needs ~60 million (bin, g-point, layer) triples on a handle with opacities and is
    # not run either, as the IR call's is not
    from clima_amd import synthetic as S
    from clima_amd.radtran import ClimaException, Radtran
    with pytest.raises(ClimaException, match="channels need at least one bin"):
        Radtran(S.make_tables(**dict(CF._SMALL, **dict(CF._RAYLEIGH, nw=8, ng=4, seed=431, sol_frac=0.0))), s.NZ, s.NZEN, 0.3)
    r.synchronize()
    assert all(np.all(np.isnan(host[k])) and bool(torch.isnan(dev[k]).all()) for k in OUT)      # nothing was written
    after = _state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert call("host") == "" and call("device") == ""                # the handle is usable afterwards
    r.synchronize()
    assert not np.any(np.isnan(host["tau"])) and not bool(torch.isnan(dev["tau"]).any())
    assert all(dev[k].cpu().numpy().tobytes() == host[k].tobytes() for k in OUT)
