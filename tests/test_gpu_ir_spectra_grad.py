"""The differentiable IR spectra: radtran_ir_spectra_batch_device (device arrays, the weights kept by the caller),
radtran_ir_spectra_batch_vjp / _vjp_device (the temperature gradient, clima_amd/csrc/ir_rows_vjp.inc) and the torch op on top
of them.  Held to the host batch bit for bit (1, 2), to an fsum contraction of a 40-digit dB/dT (3), to the library's own
spectral Jacobian (4), to itself (5: exact zeros, independence of the other columns, repeatable, host = device, the handle
untouched), to torch's gradcheck and stream ordering (6), to its refusals (7) and to the Fortran binding (8).

Error metric of the gradient: |got - want| of a (j, c) over the sum of |terms| of that (j, c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ir_jacobian_spectral_oracle as JS
import ir_spectra_vjp_oracle as VO

pytestmark = pytest.mark.gpu

# The gradient kernel alone against math.fsum of G w dB/dT (test 3), over sum |terms|.  Each term is a product of three
# factors good to a few ulps each (G: one FMA; w: given; dB/dT: an exp, an expm1, two divisions), the sum adds
# ceil(n_ir / 64) FMAs and 7 additions per lane, so a few 1e-16 are expected and anything above 1e-13 -- the ceiling the
# project gives the apply kernel -- is a defect.  The bound is 5 x the worst measured on an MI355X (the project's convention).
# Measured, test 3: MEASURED_VJP_CASES below.
MEASURED_VJP = 8.63e-16
TOL_VJP = 5.0 * MEASURED_VJP
assert MEASURED_VJP <= 1.0e-13

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _tables(which):
    from clima_amd import synthetic as S
    return S.modern_earth_tables(nw=40 if which == "small" else which)


def _handle(tables, nz, hard=True, radiate=True):
    from clima_amd import synthetic as S
    from clima_amd.radtran import Radtran
    r = Radtran(tables, nz, 2, 0.3)
    r.has_hard_surface = hard
    r.surface_emissivity = np.linspace(0.65, 1.0, len(r.surface_emissivity))
    col = S.modern_earth_column(nz)
    if radiate:
        r.radiate(*col.args())
    return r, col


def _levels(nz, nsel):
    """numpy-style, ground-first: the top alone; or the top, the ground and the top again"""
    return [nz] if nsel == 1 else [nz, 0, nz]


def _profiles(col, nz, n, seed):
    """T_surface (n), T (nz, n) Fortran-ordered: the profile, then random 150-350 K columns"""
    rng = np.random.default_rng(seed)
    T = rng.uniform(150.0, 350.0, (nz, n))
    Ts = rng.uniform(150.0, 350.0, n)
    T[:, 0], Ts[0] = np.asarray(col["T"], dtype=float), float(col["T_surface"])
    return Ts, np.asfortranarray(T)


def _dev(a):
    """a host array in ir_spectra_batch's layout (column last, Fortran order) as the tensor forms take it (column first, C)"""
    import torch
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(*reversed(range(a.ndim))))).cuda()


def _same_bits(t, host):
    a = t.cpu().numpy()
    return a.transpose(*reversed(range(a.ndim))).tobytes() == np.asarray(host).tobytes()


# ------------------------------------------------------------------ 1
FORWARD_CASES = [("small", 1, 1, True, ("up",), 1), ("small", 5, 5, False, ("dn",), 3), ("small", 63, 16, True, ("up", "dn"), 3),
                 ("small", 64, 17, False, ("up", "dn"), 3), ("small", 65, 21, True, ("up", "dn"), 1), ("small", 130, 5, False, ("up",), 3),
                 (106, 33, 17, True, ("up", "dn"), 3), (108, 33, 21, False, ("dn", "up"), 3)]


@pytest.mark.parametrize("which,nz,n,hard,parts,nsel", FORWARD_CASES)
def test_01_the_device_forward_is_the_host_batch_bit_for_bit(hip_lib, which, nz, n, hard, parts, nsel):
    import torch
    r, col = _handle(_tables(which), nz, hard)
    lv = _levels(nz, nsel)
    Ts, T = _profiles(col, nz, n, nz + n)
    host = r.ir_spectra_batch(Ts, T, levels=lv, parts=parts, fluxes=True, weights=True)
    dTs, dT = _dev(Ts), _dev(T)
    first = r.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=parts, fluxes=True, return_weights=True, sync=True)
    assert sorted(first) == sorted(host)
    for k in host:
        assert first[k].is_contiguous() and _same_bits(first[k], host[k]), (k, "weights_given = 0")
    w = {k: v for k, v in first.items() if k.startswith("w_")}
    again = r.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=parts, fluxes=True, weights=w, sync=True)
    assert sorted(again) == sorted(k for k in host if not k.startswith("w_"))
    for k in again:
        assert _same_bits(again[k], host[k]), (k, "weights_given = 1")
    # the weights left in the handle (no w_* asked for), and a sum asked for without its spectrum (staged in the handle)
    plain = r.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=parts, sync=True)
    for k in plain:
        assert _same_bits(plain[k], host[k]), (k, "no weights returned")
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    rows = np.array([v + 1 for v in lv], dtype=np.int32)
    err = C.create_string_buffer(1025)
    for given in (0, 1):
        sums = {k: torch.full((n, len(lv)), 7.0, dtype=torch.float64, device="cuda") for k in ("fup_n", "fdn_n") if k in host}
        spec = torch.full((n, len(lv), host["f" + parts[0]].shape[0]), 7.0, dtype=torch.float64, device="cuda")
        a = lambda d, k: d[k].data_ptr() if k in d else None   # noqa: E731
        both = len(sums) == 2      # both directions: the up spectrum given, the down one staged
        hip_lib.radtran_ir_spectra_batch_device(r._ptr, i(n), dTs.data_ptr(), i(nz), i(n), dT.data_ptr(), i(len(lv)), rows.ctypes.data_as(IP),
                                                spec.data_ptr() if both else None, None, a(sums, "fup_n"), a(sums, "fdn_n"),
                                                a(w, "w_up") if given else None, a(w, "w_dn") if given else None, i(given), None, err)
        assert err.value.decode() == ""
        r.synchronize()
        for k in sums:
            assert _same_bits(sums[k], host[k]), (k, "sums without spectra", given)
        if both:
            assert _same_bits(spec, host["fup"])


# ------------------------------------------------------------------ 2
def test_02_the_weights_outlive_the_opacities_they_came_from(small_tables):
    from clima_amd import synthetic as S
    nz, n = 33, 5
    r, col = _handle(small_tables, nz, True)
    lv = _levels(nz, 3)
    Ts, T = _profiles(col, nz, n, 2)
    dTs, dT = _dev(Ts), _dev(T)
    kw = dict(levels=lv, parts=("up", "dn"), fluxes=True)
    first = r.ir_spectra_batch_tensors(dTs, dT, return_weights=True, sync=True, **kw)
    w = {k: first[k].clone() for k in ("w_up", "w_dn")}
    other = S.Column(col, T=np.asarray(col["T"], dtype=float) - 15.0, densities=np.asarray(col["densities"], dtype=float) * 1.5)
    r.radiate(*other.args())                                       # another column's opacities on the handle
    reused = r.ir_spectra_batch_tensors(dTs, dT, weights=w, sync=True, **kw)
    fresh = r.ir_spectra_batch_tensors(dTs, dT, sync=True, **kw)
    for k in reused:
        assert _same_bits(reused[k], first[k].cpu().numpy().transpose(*reversed(range(first[k].dim())))), k
    assert not _same_bits(fresh["fup"], first["fup"].cpu().numpy().transpose(2, 1, 0))
    assert all(w[k].equal(first[k]) for k in w)                   # inputs with weights_given = 1: not written


# ------------------------------------------------------------------ 3
# (tables, nz, ncol, nsel, parts): worst error over sum |terms| measured on an MI355X
MEASURED_VJP_CASES = {("small", 5, 5, 3, ("up", "dn")): 1.54e-16, ("small", 65, 17, 1, ("up",)): 8.63e-16,
                      (106, 4, 16, 3, ("dn",)): 1.84e-16, (108, 7, 21, 3, ("up", "dn")): 1.70e-16}


@pytest.mark.parametrize("which,nz,n,nsel,parts", list(MEASURED_VJP_CASES))
def test_03_the_gradient_kernel_alone(which, nz, n, nsel, parts):
    """random signed weights and cotangents through the host form, on a handle that never computed opacities, against fsum
    of a 40-digit dB/dT; columns of 150 K and the highest-frequency bins included (dB/dT underflows there)"""
    tables = _tables(which)
    r, col = _handle(tables, nz, True, radiate=False)
    rng = np.random.default_rng(nz * 100 + n)
    Ts, T = _profiles(col, nz, n, nz)
    T[:, 1], Ts[1] = 150.0, 150.0
    ir_start, freq, ir_freq = JS.channel(tables)
    df = JS.dfreq(tables)
    nw_ir = len(df)
    avg = np.array([0.5 * (freq[ir_start + l] + freq[ir_start + l + 1]) for l in range(nw_ir)])
    w = {"w_" + p: np.asfortranarray(rng.uniform(-1.0, 1.0, (nw_ir, nsel, nz + 1))) for p in parts}
    g = {}
    for p in parts:
        g["f" + p] = np.asfortranarray(rng.uniform(-1.0, 1.0, (nw_ir, nsel, n)))
        g["f%s_n" % p] = np.asfortranarray(rng.uniform(-1.0, 1.0, (nsel, n)) / np.max(np.abs(df)))
    gTs, gT = r.ir_spectra_vjp(Ts, T, w, g)
    assert gTs.shape == (n,) and gT.shape == (nz, n) and np.all(np.isfinite(gTs)) and np.all(np.isfinite(gT))
    wTs, wT, sa = VO.vjp(avg, df, Ts, T, w, g)
    assert np.all(sa > 0.0)
    e = max(float(np.max(np.abs(gTs - wTs) / sa[0])), float(np.max(np.abs(gT - wT) / sa[1:])))
    print("%s nz %d ncol %d nsel %d %s: %.2e of sum |terms| [%.1e]" % (which, nz, n, nsel, "+".join(parts), e, TOL_VJP))
    assert e <= TOL_VJP


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("nz,hard", [(40, True), (5, False)])
def test_04_against_the_librarys_own_jacobian(small_tables, nz, hard):
    """sum over l, a of g(l, a) jac_up_a(l, a, j) from ir_jacobian_spectral at the same T; test_07 of
    test_gpu_ir_spectra_batch holds w dB/dT to 1e-12 of the row's largest entry, so the contraction is held to the sum over
    the terms of |g| times that bound.  The cotangent of a sum the same way, with g = dfreq."""
    r, col = _handle(small_tables, nz, hard)
    lv = _levels(nz, 3)
    Ts, T = float(col["T_surface"]), np.asarray(col["T"], dtype=float)
    w = r.ir_spectra_batch(None, None, levels=lv, parts=("up", "dn"), weights=True)
    jac = r.ir_jacobian_spectral(Ts, T, levels=lv, parts=("up", "dn"))
    df = JS.dfreq(small_tables)
    nw_ir = len(df)
    rng = np.random.default_rng(nz)
    g = {"fup": rng.uniform(-1.0, 1.0, (nw_ir, 3, 1)), "fdn": rng.uniform(-1.0, 1.0, (nw_ir, 3, 1))}
    for grads, G in ((g, {"up": g["fup"][:, :, 0], "dn": g["fdn"][:, :, 0]}),
                     ({"fup_n": np.ones((3, 1)), "fdn_n": np.ones((3, 1))}, {"up": np.repeat(df[:, None], 3, 1), "dn": np.repeat(df[:, None], 3, 1)})):
        gTs, gT = r.ir_spectra_vjp(Ts, T, w, grads)
        got = np.concatenate([gTs, gT[:, 0]])
        want, bound = np.zeros(nz + 1), 0.0
        for name in ("up", "dn"):
            want += np.einsum("la,laj->j", G[name], jac[name])
            bound += float(np.sum(np.abs(G[name]) * 1e-12 * np.maximum(np.max(np.abs(jac[name]), axis=2), 1e-300)))
        print("nz %d hard %s %s: worst %.2e [%.1e], largest entry %.2e" % (nz, hard, "+".join(grads), np.max(np.abs(got - want)), bound, np.max(np.abs(want))))
        assert np.max(np.abs(want)) > 1e3 * bound
        assert np.all(np.abs(got - want) <= bound)


# ------------------------------------------------------------------ 5
def test_05_exact_properties(small_tables):
    nz, n, nsel = 33, 21, 3
    r, col = _handle(small_tables, nz, True)
    lv = _levels(nz, nsel)
    Ts, T = _profiles(col, nz, n, 5)
    w = r.ir_spectra_batch(None, None, levels=lv, parts=("up", "dn"), weights=True)
    nw_ir = w["w_up"].shape[0]
    rng = np.random.default_rng(55)
    g = dict(fup=np.asfortranarray(rng.uniform(-1.0, 1.0, (nw_ir, nsel, n))), fdn=np.asfortranarray(rng.uniform(-1.0, 1.0, (nw_ir, nsel, n))),
             fup_n=np.asfortranarray(rng.uniform(-1e-12, 1e-12, (nsel, n))), fdn_n=np.asfortranarray(rng.uniform(-1e-12, 1e-12, (nsel, n))))
    gTs, gT = r.ir_spectra_vjp(Ts, T, w, g)
    assert np.all(gTs != 0.0) and np.all(gT != 0.0)
    # all-zero cotangents; a dn cotangent at the top of the atmosphere alone (its weights are the constant 0)
    zTs, zT = r.ir_spectra_vjp(Ts, T, w, {k: np.zeros_like(v) for k, v in g.items()})
    assert np.all(zTs == 0.0) and np.all(zT == 0.0)
    top = r.ir_spectra_batch(None, None, levels=[nz], parts=("dn",), weights=True)
    zTs, zT = r.ir_spectra_vjp(Ts, T, top, dict(fdn=np.asfortranarray(g["fdn"][:, :1, :]), fdn_n=np.asfortranarray(g["fdn_n"][:1, :])))
    assert np.all(zTs == 0.0) and np.all(zT == 0.0)
    # two calls; the device form
    aTs, aT = r.ir_spectra_vjp(Ts, T, w, g)
    assert aTs.tobytes() == gTs.tobytes() and aT.tobytes() == gT.tobytes()
    dw, dg = {k: _dev(v) for k, v in w.items()}, {k: _dev(v) for k, v in g.items()}
    dTs, dT = r.ir_spectra_vjp_tensors(_dev(Ts), _dev(T), dw, dg, sync=True)
    assert _same_bits(dTs, gTs) and _same_bits(dT, gT)
    # a column alone, and inside other batches in other positions (21 and 16 columns: tiles of 4 with and without a tail;
    # 5 and 1: tiles of 1)
    pick = lambda idx: (Ts[idx], np.asfortranarray(T[:, idx]), {k: np.asfortranarray(v[..., idx]) for k, v in g.items()})   # noqa: E731
    for c in (0, 3, 16, 20):
        for idx in ([c], [1, 2, c, 4, 5], list(range(1, 16)) + [c], [c] + list(range(20))):
            sTs, sT, sg = pick(idx)
            oTs, oT = r.ir_spectra_vjp(sTs, sT, w, sg)
            at = idx.index(c)
            assert oTs[at] == gTs[c] and oT[:, at].tobytes() == gT[:, c].tobytes(), (c, len(idx))
    # a direction whose cotangents are absent is not read: its weights may be given or not
    up = {k: v for k, v in g.items() if "up" in k}
    bTs, bT = r.ir_spectra_vjp(Ts, T, w, up)
    cTs, cT = r.ir_spectra_vjp(Ts, T, dict(w_up=w["w_up"]), up)
    assert bTs.tobytes() == cTs.tobytes() and bT.tobytes() == cT.tobytes() and bT.tobytes() != gT.tobytes()


def test_05_the_handle_afterwards(small_tables):
    from test_gpu_batch_bounds import fields_of
    from test_gpu_entry_points import left_state
    from test_gpu_merged_integration import _assert_same_state
    from clima_amd.radtran import Radtran
    nz, n = 20, 5
    r, col = _handle(small_tables, nz, True)
    lv = _levels(nz, 3)
    Ts, T = _profiles(col, nz, n, 8)
    dTs, dT = _dev(Ts), _dev(T)
    before, fields, opr = left_state(r), fields_of(r), [np.array(a) for a in r.opr()]

    def three(h):
        out = h.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=("up", "dn"), fluxes=True, return_weights=True, sync=True)
        w = {k: out.pop(k) for k in ("w_up", "w_dn")}
        g = {k: v.clone() for k, v in out.items()}
        dev = h.ir_spectra_vjp_tensors(dTs, dT, w, g, sync=True)
        host = h.ir_spectra_vjp(Ts, T, {k: v.cpu().numpy().transpose(2, 1, 0) for k, v in w.items()},
                                {k: v.cpu().numpy().transpose(*reversed(range(v.dim()))) for k, v in g.items()})
        assert _same_bits(dev[0], host[0]) and _same_bits(dev[1], host[1])
        return host
    first = three(r)
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    for k, v in fields_of(r).items():
        assert v.tobytes() == fields[k].tobytes(), k
    for a, b in zip(r.opr(), opr):
        assert np.array(a).tobytes() == b.tobytes()
    # a pending deferred integration is settled first, and correctly
    pair = []
    for defer in (True, False):
        h = Radtran(small_tables, nz, 2, 0.3)
        h.surface_emissivity = np.asarray(r.surface_emissivity, dtype=float)
        h.defer_integration = defer
        h.upload_column(*col.args())
        h.radiate_resident()
        got = three(h)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), defer
        h.synchronize()
        pair.append(h)
    _assert_same_state(pair[0], pair[1], "deferring against not, the spectra's gradient in between")


# ------------------------------------------------------------------ 6
def test_06_torch_backward_matches_the_jacobian_contraction(small_tables):
    import torch
    nz, n = 12, 3
    r, col = _handle(small_tables, nz, True)
    lv = _levels(nz, 3)
    Ts, T = _profiles(col, nz, n, 6)
    T = np.asfortranarray(np.asarray(col["T"], dtype=float)[:, None] + np.arange(n)[None, :] * 3.0)
    Ts = float(col["T_surface"]) + np.arange(n) * 2.0
    for reuse in (False, True):
        weights = None
        if reuse:
            out = r.ir_spectra_batch_tensors(_dev(Ts), _dev(T), levels=lv, parts=("up", "dn"), return_weights=True, sync=True)
            weights = {k: out[k] for k in ("w_up", "w_dn")}
        tTs, tT = _dev(Ts).requires_grad_(True), _dev(T).requires_grad_(True)
        out = r.ir_spectra_torch(tTs, tT, levels=lv, parts=("up", "dn"), weights=weights)
        assert sorted(out) == ["fdn", "fup"] and out["fup"].shape == (n, 3, len(JS.dfreq(small_tables)))
        (out["fup"].sum() + out["fdn"].sum()).backward()
        r.synchronize()
        got = np.concatenate([tTs.grad.cpu().numpy()[None, :], tT.grad.cpu().numpy().T])      # (nz+1, n)
        for c in range(n):
            jac = r.ir_jacobian_spectral(Ts[c], T[:, c], levels=lv, parts=("up", "dn"))
            want = jac["up"].sum(axis=(0, 1)) + jac["dn"].sum(axis=(0, 1))
            bound = sum(float(np.sum(1e-12 * np.max(np.abs(jac[k]), axis=2))) for k in ("up", "dn"))
            assert np.max(np.abs(want)) > 1e3 * bound
            assert np.all(np.abs(got[:, c] - want) <= bound), (reuse, c)


def test_06_gradcheck(small_tables):
    import torch
    nz, n = 4, 2
    r, col = _handle(small_tables, nz, True)
    Ts, T = _profiles(col, nz, n, 4)
    T[:, 1], Ts[1] = np.linspace(260.0, 210.0, nz), 275.0
    tTs, tT = _dev(Ts).requires_grad_(True), _dev(T).requires_grad_(True)
    kw = dict(levels=[nz, 0], parts=("up", "dn"), fluxes=True)
    base = r.ir_spectra_batch_tensors(tTs.detach(), tT.detach(), sync=True, **kw)
    gen = torch.Generator(device="cpu").manual_seed(3)
    # scalar weights that bring every output element to O(1) (the spectra are per Hz): 1 / its value where that is not 0
    scale = {k: (torch.where(v != 0.0, 1.0 / v, torch.zeros_like(v)) * (0.5 + torch.rand(v.shape, generator=gen, dtype=torch.float64).cuda()))
             for k, v in base.items()}

    def loss(a, b):
        out = r.ir_spectra_torch(a, b, **kw)
        return sum((out[k] * scale[k]).sum() for k in sorted(out))
    for weights in (None, "reused"):
        if weights:
            w = r.ir_spectra_batch_tensors(tTs.detach(), tT.detach(), return_weights=True, sync=True, **kw)
            kw["weights"] = {k: w[k] for k in ("w_up", "w_dn")}
        loss(tTs, tT).backward()
        assert float(tT.grad.abs().max()) > 1e-2 and float(tTs.grad.abs().max()) > 1e-2      # (well above gradcheck's atol)
        tTs.grad = tT.grad = None
        assert torch.autograd.gradcheck(loss, (tTs, tT))


def test_06_a_side_stream_without_a_host_sync(small_tables):
    import torch
    nz, n = 33, 256
    r, col = _handle(small_tables, nz, True)
    Ts, T = _profiles(col, nz, n, 9)
    want = r.ir_spectra_batch_tensors(_dev(Ts), _dev(T), fluxes=True, sync=True)
    want_sum = want["fup"].sum(dim=(1, 2)) + want["fup_n"].sum(dim=1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    hTs, hT = torch.from_numpy(Ts).pin_memory(), torch.from_numpy(np.ascontiguousarray(T.T)).pin_memory()
    with torch.cuda.stream(side):
        dTs, dT = hTs.to("cuda", non_blocking=True), hT.to("cuda", non_blocking=True)
        dT = dT + 0.0                                               # the inputs are still being produced when the call is made
        got = r.ir_spectra_batch_tensors(dTs, dT, fluxes=True, sync=False)
        got_sum = got["fup"].sum(dim=(1, 2)) + got["fup_n"].sum(dim=1)      # a torch reduction right behind, on the same stream
        grad = r.ir_spectra_vjp_tensors(dTs, dT, {"w_up": r.ir_spectra_batch_tensors(dTs, dT, return_weights=True)["w_up"]},
                                        {"fup": got["fup"]})[1].sum()
    side.synchronize()
    r.synchronize()
    assert got_sum.equal(want_sum)
    assert bool(torch.isfinite(grad)) and float(grad) != 0.0


def test_06_two_enqueued_calls_keep_their_own_levels(small_tables):
    """Two calls that only enqueue, with different `levels`, right behind each other on a handle whose producer stream is
    still busy: each computes its weights for its own levels (a staging block the calls share would be rewritten by
    the second call before the first one's copy has run)"""
    import torch
    nz, n = 33, 3
    r, col = _handle(small_tables, nz, True)
    Ts, T = _profiles(col, nz, n, 12)
    dTs, dT = _dev(Ts), _dev(T)
    asked = ((-1,), (0,))
    want = [r.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=("up", "dn"), sync=True) for lv in asked]
    assert not want[0]["fup"].equal(want[1]["fup"])
    torch.cuda.synchronize()
    torch.cuda._sleep(50_000_000)          # tens of milliseconds of the current stream (half a second on a 100 MHz counter)
    got = [r.ir_spectra_batch_tensors(dTs, dT, levels=lv, parts=("up", "dn"), sync=False) for lv in asked]
    torch.cuda.synchronize()
    r.synchronize()
    for lv, w, g in zip(asked, want, got):
        assert sorted(g) == sorted(w) == ["fdn", "fup"]
        for k in w:
            assert g[k].cpu().numpy().tobytes() == w[k].cpu().numpy().tobytes(), (lv, k)


# ------------------------------------------------------------------ 7
def test_07_refusals(hip_lib, small_tables):
    import torch
    from clima_amd.radtran import ClimaException, Radtran
    from test_gpu_entry_points import left_state
    L = hip_lib
    nz, n, nsel = 10, 3, 2
    nl = nz + 1
    r, col = _handle(small_tables, nz, True)
    nw_ir = len(JS.dfreq(small_tables))
    Ts, T = _profiles(col, nz, n, 7)
    err = C.create_string_buffer(1025)
    i = lambda v: C.byref(C.c_int(v))   # noqa: E731
    new = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")   # noqa: E731
    dev = dict(Ts=_dev(Ts), T=_dev(T), w_up=new(nl, nsel, nw_ir), w_dn=new(nl, nsel, nw_ir), fup=new(n, nsel, nw_ir), fdn=new(n, nsel, nw_ir),
               fup_n=new(n, nsel), fdn_n=new(n, nsel), gTs=new(n), gT=new(n, nz))
    host = {k: v.cpu().numpy().copy() for k, v in dev.items()}
    lv = np.array([nl, 1], dtype=np.int32)
    before = left_state(r)

    def vjp(form, ncol=n, dim1=nz, dim2=n, nsel=nsel, skip=(), swap=None, handle=None):
        """the gradient form `form` ("host" / "device") with the argument names in `skip` NULL; swap: a name given as a HOST
        pointer to the device form"""
        src = host if form == "host" else dev
        def p(k):
            if k in skip:
                return None
            a = host[k] if k == swap else src[k]
            if form == "host":
                return a.ctypes.data_as(DP)
            return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        args = [handle or r._ptr, i(ncol), p("Ts"), i(dim1), i(dim2), p("T"), i(nsel), p("w_up"), p("w_dn"), p("fup"), p("fdn"), p("fup_n"),
                p("fdn_n"), p("gTs"), p("gT")]
        if form == "host":
            L.radtran_ir_spectra_batch_vjp(*args, err)
        else:
            L.radtran_ir_spectra_batch_vjp_device(*args, None, err)
        return err.value.decode()

    for form, who in (("host", "ir_spectra_batch_vjp: "), ("device", "ir_spectra_batch_vjp_device: ")):
        assert vjp(form, skip=("w_dn",)) == who + '"g_ir_fdn" was given without "w_dn"'
        assert vjp(form, skip=("w_up", "fup")) == who + '"g_fup_n" was given without "w_up"'
        assert vjp(form, skip=("w_up", "w_dn")) == who + "neither w_up nor w_dn was given"
        assert vjp(form, skip=("fup", "fdn", "fup_n", "fdn_n")) == who + "none of g_ir_fup, g_ir_fdn, g_fup_n, g_fdn_n was given"
        assert vjp(form, skip=("gT",)) == who + '"grad_T" is a required argument'
        assert vjp(form, skip=("gTs",)) == who + '"grad_T_surface" is a required argument'
        assert vjp(form, skip=("T",)) == who + '"T" is a required argument (ncol = 3)'
        assert vjp(form, dim1=nz - 1) == '"T" has the wrong input dimension.'
        assert vjp(form, dim2=n + 1) == '"T" has the wrong input dimension.'
        assert vjp(form, nsel=0) == who + "nsel must be at least 1 (nsel = 0)"
        assert vjp(form, ncol=0, dim2=0) == who + "ncol must be at least 1 (ncol = 0)"
    for name, arg in (("T", "T"), ("T_surface", "Ts"), ("w_dn", "w_dn"), ("g_ir_fup", "fup"), ("g_fdn_n", "fdn_n"), ("grad_T", "gT")):
        assert vjp("device", swap=arg) == 'ir_spectra_batch_vjp_device: "%s" is not device memory of this handle\'s device' % name
    bad = host["T"].copy()
    host["T"][2, 3] = -5.0                                          # C (ncol, nz): column 3, layer 4
    assert vjp("host").startswith("ir_spectra_batch_vjp: temperatures must be finite and positive (T(4, 3) = -5.0")
    host["T"][:] = bad
    host["Ts"][1] = float("nan")
    assert vjp("host").startswith("ir_spectra_batch_vjp: temperatures must be finite and positive (T_surface(2) = nan")
    host["Ts"][:] = Ts
    assert all(np.all(host[k] == 7.0) for k in ("gTs", "gT")) and bool((dev["gT"] == 7.0).all()) and bool((dev["gTs"] == 7.0).all())

    def fwd(ncol=n, dim1=nz, dim2=n, nsel=nsel, level=lv, skip=(), swap=None, given=0, handle=None):
        def p(k):
            if k in skip:
                return None
            return host[k].ctypes.data if k == swap else dev[k].data_ptr()
        L.radtran_ir_spectra_batch_device(handle or r._ptr, i(ncol), p("Ts"), i(dim1), i(dim2), p("T"), i(nsel),
                                          level.ctypes.data_as(IP) if level is not None else None, p("fup"), p("fdn"), p("fup_n"), p("fdn_n"),
                                          p("w_up"), p("w_dn"), i(given), None, err)
        return err.value.decode()

    who = "ir_spectra_batch_device: "
    for name, arg in (("T", "T"), ("T_surface", "Ts"), ("ir_fup", "fup"), ("fdn_n", "fdn_n"), ("w_up", "w_up")):
        assert fwd(swap=arg) == who + '"%s" is not device memory of this handle\'s device' % name
    assert fwd(dim1=nz - 1) == '"T" has the wrong input dimension.'
    assert fwd(dim2=n + 1) == '"T" has the wrong input dimension.'
    assert fwd(nsel=0) == who + "nsel must be at least 1 (nsel = 0)"
    assert fwd(ncol=-1, dim2=-1) == who + "ncol must not be negative (ncol = -1)"
    assert fwd(level=None) == who + '"spec_level" is a required argument'
    assert fwd(level=np.array([1, nl + 1], dtype=np.int32)) == who + "spec_level(2) = %d is outside 1..%d" % (nl + 1, nl)
    assert fwd(skip=("fup", "fdn", "fup_n", "fdn_n", "w_up", "w_dn")) == who + "none of ir_fup, ir_fdn, fup_n, fdn_n, w_up, w_dn was given"
    assert fwd(skip=("w_dn",), given=1) == who + '"w_dn" is a required argument (weights_given = 1 and its direction is asked for)'
    assert fwd(skip=("fup", "fdn", "fup_n", "fdn_n"), given=1) == who + "none of ir_fup, ir_fdn, fup_n, fdn_n was given (weights_given = 1)"
    assert fwd(skip=("T",)) == who + '"T" is a required argument (ncol = 3)'
    assert all(bool((dev[k] == 7.0).all()) for k in ("fup", "fdn", "fup_n", "fdn_n", "w_up", "w_dn"))      # nothing was written
    after = left_state(r)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    # a bin shard; a handle without opacities takes given weights and the gradient, not weights_given = 0
    sh = Radtran(small_tables, nz, 2, 0.3)
    sh.radiate(*col.args())
    sh.set_bin_shard(0, 2)
    assert fwd(handle=sh._ptr) == who + "needs the whole spectrum (a bin shard of 2)"
    assert vjp("host", handle=sh._ptr) == "ir_spectra_batch_vjp: needs the whole spectrum (a bin shard of 2)"
    assert vjp("device", handle=sh._ptr) == "ir_spectra_batch_vjp_device: needs the whole spectrum (a bin shard of 2)"
    fresh = Radtran(small_tables, nz, 2, 0.3)
    assert fwd(handle=fresh._ptr) == "ir_spectra_batch_device needs opacities: call radiate with compute_opacity first"
    assert fwd(handle=fresh._ptr, given=1) == "" and vjp("device", handle=fresh._ptr) == "" and vjp("host", handle=fresh._ptr) == ""
    fresh.synchronize()
    assert fwd() == "" and vjp("device") == "" and vjp("host") == ""      # the handle is usable afterwards
    r.synchronize()
    assert not bool((dev["fup"] == 7.0).any()) and not bool((dev["gT"] == 7.0).any()) and not np.any(host["gT"] == 7.0)
    # Python: a tensor that is not contiguous, or float32
    with pytest.raises(ClimaException, match='ir_spectra_batch_device: "T" is not C-contiguous'):
        r.ir_spectra_batch_tensors(dev["Ts"], _dev(T.T.copy()).t())
    with pytest.raises(ClimaException, match='ir_spectra_batch_device: "T" is not a float64 torch tensor'):
        r.ir_spectra_batch_tensors(dev["Ts"], dev["T"].float())
    with pytest.raises(ClimaException, match='ir_spectra_batch_device: "T" is not device memory of this handle\'s device'):
        r.ir_spectra_batch_tensors(dev["Ts"], dev["T"].cpu())
    with pytest.raises(ClimaException, match='ir_spectra_batch_vjp_device: "fup" is not C-contiguous'):
        r.ir_spectra_vjp_tensors(dev["Ts"], dev["T"], {"w_up": dev["w_up"]}, {"fup": new(nw_ir, nsel, n).permute(2, 1, 0)})


# ------------------------------------------------------------------ 8
FORTRAN_CALLS = """  allocate(Tc(nz,3), Tsc(3), su(n_ir-1,2,3), nd(2,3), wu(n_ir-1,2,nz+1), wd(n_ir-1,2,nz+1), grT(nz,3), grTs(3))
  do i = 1, 3
    Tc(:,i) = T + 2.0_dp*(i-1); Tsc(i) = T_surface - 1.5_dp*(i-1)
  enddo
  call rad%ir_spectra_batch(Tsc, Tc, [nz+1, 1], err, ir_fup_a=su, fdn_n=nd, w_up=wu, w_dn=wd); call check()
  call rad%ir_spectra_batch_vjp(Tsc, Tc, grTs, grT, err, w_up=wu, w_dn=wd, g_ir_fup_a=su, g_fdn_n=nd); call check()
  print '(a,2es24.16)', 'checksum ', sum(grTs), sum(grT)
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) grTs; write(u) grT
  close(u)
  call rad%ir_spectra_batch_vjp(Tsc, Tc, grTs, grT, err, w_up=wu, g_fdn_n=nd)
  print '(a)', 'expected error: '//err
  call rad%ir_spectra_batch_vjp(Tsc, Tc, grTs, grT(:nz-1,:), err, w_up=wu, g_ir_fup_a=su)
  print '(a)', 'expected error: '//err
"""


def test_08_fortran_binding_matches_python(tmp_path):
    from clima_amd import build, synthetic as S
    from clima_amd.fortran_case import write_case
    from clima_amd.radtran import Radtran
    from test_gpu_ir_jacobian import FORTRAN_PROGRAM
    if not os.path.exists(build.FLANG):
        pytest.skip("amdflang is not available on this box")
    build.build()
    head, rest = FORTRAN_PROGRAM.split("  allocate(ju(nz+1,nz+1)")
    tail = rest[rest.index("  call rad%destroy()"):]
    decl = "Tc(:,:), Tsc(:), su(:,:,:), nd(:,:), wu(:,:,:), wd(:,:,:), grT(:,:), grTs(:)"
    program = head.replace("ju(:,:), jd(:,:), jt(:,:)", decl) + FORTRAN_CALLS + tail
    tb = S.modern_earth_tables(nw=30)
    nz, nzen, albedo = 40, 4, 0.15
    col = S.modern_earth_column(nz)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "grad.bin")
    write_case(case, tb, col, nzen, albedo)
    src, exe = tmp_path / "grad.f90", str(tmp_path / "grad")
    src.write_text(program)
    subprocess.check_call([build.FLANG, "-O2", "-J", str(tmp_path), os.path.join(build.FORTRAN_DIR, "clima_radtran_hip.f90"),
                           str(src), "-o", exe, "-L" + build.CSRC, "-lclima_radtran_hip", "-Wl,-rpath," + build.CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"], cwd=str(tmp_path))
    out = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'expected error: ir_spectra_batch_vjp: "g_fdn_n" was given without "w_dn"' in out.stdout
    assert 'expected error: ir_spectra_batch_vjp: "grad_T" has the wrong dimension' in out.stdout
    r = Radtran(tb, nz, nzen, albedo)
    r.radiate(*col.args())
    T = np.asfortranarray(np.stack([np.asarray(col["T"], dtype=float) + 2.0 * i for i in range(3)], axis=1))
    Ts = np.array([float(col["T_surface"]) - 1.5 * i for i in range(3)])
    f = r.ir_spectra_batch(Ts, T, levels=[-1, 0], parts=("up", "dn"), fluxes=True, weights=True)
    gTs, gT = r.ir_spectra_vjp(Ts, T, dict(w_up=f["w_up"], w_dn=f["w_dn"]), dict(fup=f["fup"], fdn_n=f["fdn_n"]))
    m = np.fromfile(res, dtype=np.float64)
    assert m.size == 3 + nz * 3
    assert m[:3].tobytes() == gTs.tobytes() and m[3:].tobytes() == gT.tobytes(order="F")
    sums = [float(v) for v in out.stdout.split("checksum")[1].split()[:2]]
    assert np.allclose(sums, [gTs.sum(), gT.sum()], rtol=1e-12)
