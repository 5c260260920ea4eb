"""Python mirror of Clima's `Radtran` (clima/cython/Radtran.pyx, ClimaRadtranWrk.pyx,
RTChannel.pyx) over the HIP C ABI.  Same attribute names, argument meaning and error
behaviour (`ClimaException` carrying the reference's message text).

The reference's Python layer reaches `Radtran%radiate` only through `AdiabatClimate`
(`c.rad`); here the `Radtran` object itself is constructible from a table set because the
HDF5/YAML loaders are outside the hot path (SURVEY.md 8(f) "next #1").
"""
import ctypes as C
import os

import numpy as np

from . import lib as _lib

_dp = C.POINTER(C.c_double)


class ClimaException(Exception):
    """clima/cython/_clima.pyx: raised with the Fortran `err` text."""


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(v):
    return C.byref(C.c_int(int(v)))


def _f(v):
    return C.byref(C.c_double(float(v)))


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _fo(a):
    return np.asfortranarray(a, dtype=np.float64)


# What the IR derivative family's requests check alike.  `who` is the message's whole prefix ("name: ").
def _level_rows(who, nz, levels):
    """numpy-style `levels` into the ground-first level axis -> 1..nz+1 as the ABI takes them"""
    nl = nz + 1
    idx = np.atleast_1d(np.asarray(levels))
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
        raise ClimaException(who + '"levels" is not a non-empty list of integer level indices')
    for a, v in enumerate(idx.tolist()):
        if v < -nl or v >= nl:
            raise ClimaException(who + "levels[%d] = %d is outside %d..%d" % (a, v, -nl, nl - 1))
    return np.ascontiguousarray(np.where(idx < 0, idx + nl, idx) + 1, dtype=np.int32)


def _names_among(who, arg, given, allowed):
    """the names `given` for the argument `arg` (one or several), in the order of `allowed` (the ABI's)"""
    given = (given,) if isinstance(given, str) else tuple(given)
    for name in given:
        if name not in allowed:
            raise ClimaException(who + '"%s" is not one of %s' % (name, ", ".join(allowed)))
    if not given:
        raise ClimaException(who + '"%s" names none of %s' % (arg, ", ".join(allowed)))
    return tuple(name for name in allowed if name in given)


def _keys_among(who, arg, d, allowed):
    if not isinstance(d, dict):
        raise ClimaException(who + '"%s" is not a dict with keys among %s' % (arg, ", ".join(allowed)))
    for name in d:
        if name not in allowed:
            raise ClimaException(who + '"%s" is not one of %s' % (name, ", ".join(allowed)))


def _one_column(who, nz, T_surface, T):
    """(T_surface (1,), T (nz,)) of one column"""
    T, Ts = _c(np.atleast_1d(T)), _c(np.atleast_1d(T_surface))
    if Ts.shape != (1,):
        raise ClimaException(who + '"T_surface" has the shape %s, not a scalar' % (tuple(np.shape(T_surface)),))
    if T.shape != (nz,):
        raise ClimaException(who + '"T" has the shape %s, not %s' % (T.shape, (nz,)))
    return Ts, T


def _column_batch(who, nz, T_surface, T, least):
    """(T_surface (ncol,), T (nz, ncol) Fortran-ordered) of at least `least` columns; a 1-D T is one column"""
    T, Ts = np.asfortranarray(T, dtype=np.float64), _c(np.atleast_1d(T_surface))
    if Ts.ndim != 1:
        raise ClimaException(who + '"T_surface" has the shape %s, not (ncol,)' % (Ts.shape,))
    if T.ndim == 1 and len(Ts) == 1:
        T = np.asfortranarray(T[:, None])
    n = len(Ts)
    if n < least or T.shape != (nz, n):
        raise ClimaException(who + '"T" has the shape %s, not %s' % (T.shape, (nz, max(n, least))))
    return Ts, T


def grey_sensitivity(opr, grads, ir_tau_min, max_w0):
    """From `Radtran.ir_spectra_opr_vjp`'s gradients to the response to an added GREY optical depth, per (layer, bin):
    what a continuum, CIA, a cloud or the custom optical properties add to every g-point alike
    (src/radtran/clima_radtran_types.f90:869-876: tau = sum of the parts, w0 = min(max_w0, scattering / tau), w0 = 0 where
    tau <= tau_min).  `opr` is `Radtran.opr()`'s tuple (tau, w0 (nz, ngauss, nw), ...), `grads` the dict with "tau" and
    "w0" of those shapes.  `ir_tau_min` and `max_w0` are the OPACITY STEP's two constants -- clima_radtran_types.f90:9-11:
    tau_min = 1e-20 and max_w0 = 0.99999 -- below and at which that step pins w0; `ir_tau_min` here is NOT the two-stream
    solver's thin-layer switch `Radtran.ir_tau_min` (1e-6 by default): with that value the w0 term of every layer with
    1e-20 < tau <= 1e-6 would be dropped.  Returns (absorption, scattering),
    each (nz, nw): the derivative of the loss with respect to an added absorption optical depth of layer n in bin l,
        sum_i [grad_tau - grad_w0 w0 / tau],
    and to an added scattering optical depth,
        sum_i [grad_tau + grad_w0 (1 - w0) / tau],
    the g-points in g order.  Where the opacity step pins w0 (tau <= ir_tau_min, or w0 at max_w0) the w0 term is dropped.
    Pure numpy; no handle."""
    tau, w0 = np.asarray(opr[0], dtype=np.float64), np.asarray(opr[1], dtype=np.float64)
    for name in ("tau", "w0"):
        if name not in grads:
            raise ClimaException('grey_sensitivity: "grads" lacks "%s"' % name)
        if tau.ndim != 3 or np.shape(grads[name]) != tau.shape or w0.shape != tau.shape:
            raise ClimaException('grey_sensitivity: "%s" has the shape %s, not that of opr\'s tau %s' % (name, np.shape(grads[name]), tau.shape))
    g_tau, g_w0 = np.asarray(grads["tau"], dtype=np.float64), np.asarray(grads["w0"], dtype=np.float64)
    free = (tau > ir_tau_min) & (w0 < max_w0)
    rtau = 1.0 / np.where(free, tau, 1.0)
    dab = np.where(free, -(w0 * rtau), 0.0)
    dsc = np.where(free, (1.0 - w0) * rtau, 0.0)
    ab, sc = np.zeros((tau.shape[0], tau.shape[2])), np.zeros((tau.shape[0], tau.shape[2]))
    for i in range(tau.shape[1]):
        ab = ab + (g_tau[:, i, :] + g_w0[:, i, :] * dab[:, i, :])
        sc = sc + (g_tau[:, i, :] + g_w0[:, i, :] * dsc[:, i, :])
    return ab, sc


class RTChannel:
    """clima/cython/RTChannel.pyx"""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr

    def _vec(self, name):
        n = C.c_int()
        getattr(self._L, "rtchannel_%s_get_size" % name)(self._ptr, C.byref(n))
        arr = np.empty(n.value, np.double)
        getattr(self._L, "rtchannel_%s_get" % name)(self._ptr, C.byref(n), _d(arr))
        return arr

    @property
    def wavl(self):
        "ndarray[double,ndim=1]. Edges of the wavelength bins (nm)."
        return self._vec("wavl")

    @property
    def freq(self):
        "ndarray[double,ndim=1]. Edges of the bins in frequency (1/s)."
        return self._vec("freq")


class ClimaRadtranWrk:
    """clima/cython/ClimaRadtranWrk.pyx: arrays are copied out, Fortran order, index 0 =
    ground level, index nz = top of the atmosphere."""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr

    def _mat(self, name):
        d1, d2 = C.c_int(), C.c_int()
        getattr(self._L, "climaradtranwrk_%s_get_size" % name)(self._ptr, C.byref(d1), C.byref(d2))
        arr = np.empty((d1.value, d2.value), np.double, order="F")
        getattr(self._L, "climaradtranwrk_%s_get" % name)(self._ptr, C.byref(d1), C.byref(d2), _d(arr))
        return arr

    def _vec(self, name):
        d1 = C.c_int()
        getattr(self._L, "climaradtranwrk_%s_get_size" % name)(self._ptr, C.byref(d1))
        arr = np.empty(d1.value, np.double)
        getattr(self._L, "climaradtranwrk_%s_get" % name)(self._ptr, C.byref(d1), _d(arr))
        return arr

    fup_a = property(lambda self: self._mat("fup_a"), doc="(nz+1,nw) mW/m^2/Hz upward flux per bin")
    fdn_a = property(lambda self: self._mat("fdn_a"), doc="(nz+1,nw) mW/m^2/Hz downward flux per bin")
    amean = property(lambda self: self._mat("amean"), doc="(nz+1,nw) mean intensity, photons/cm^2/s (solar)")
    tau_band = property(lambda self: self._mat("tau_band"), doc="(nz,nw) band optical thickness")
    fup_n = property(lambda self: self._vec("fup_n"), doc="(nz+1) mW/m^2 upward flux")
    fdn_n = property(lambda self: self._vec("fdn_n"), doc="(nz+1) mW/m^2 downward flux")


class Radtran:
    """`type Radtran` (src/radtran/clima_radtran.f90:31-85) on the MI355X."""

    def __init__(self, tables, nz, num_zenith_angles, surface_albedo):
        """Equivalent of `Radtran(species, particles, settings, star, num_zenith_angles,
        surface_albedo, nz, datadir)` (clima_radtran.f90:128-219) with the loaded tables
        handed over as a `clima_amd.synthetic.TableSet`-shaped object."""
        L = _lib.load()
        self._L = L
        self._ptr = C.c_void_p()
        L.allocate_radtran(C.byref(self._ptr))
        self._err = C.create_string_buffer(_lib.ERR_LEN + 1)
        t = tables
        self.nz = int(nz)
        self.ng = t.nsp  # number of gases, as Radtran%ng
        self.np = t.np_
        self.species_names = list(t.species_names)
        self.particle_names = list(t.particle_names)
        wavl = _c(t.wavl)
        L.radtran_create_begin(self._ptr, _i(nz), _i(t.nsp), _i(t.np_), _i(t.nw), _d(wavl), self._err)
        self._check()
        for k in t.ktables:
            w, lp, tt, kk = _c(k["weights"]), _c(k["log10P"]), _c(k["temp"]), _c(k["log10k"])
            L.radtran_add_ktable(self._ptr, _i(k["sp_ind"] + 1), _i(len(w)), _d(w), _i(len(lp)), _d(lp),
                                 _i(len(tt)), _d(tt), _d(kk), self._err)
            self._check()
        for x in t.xsections:
            temp = x.get("temp")
            tt = _c(temp if temp is not None else np.zeros(1))
            da = _c(x["data"])
            L.radtran_add_xsection(self._ptr, _i(x["xs_type"]), _i(x["dim"]), _i(x["sp1"] + 1),
                                   _i(x.get("sp2", -1) + 1), _i(0 if temp is None else len(temp)), _d(tt), _d(da),
                                   self._err)
            self._check()
        if t.continuum is not None:
            c = t.continuum
            tt, a, b = _c(c["temp"]), _c(c["log10_H2O"]), _c(c["log10_foreign"])
            L.radtran_set_water_continuum(self._ptr, _i(c["LH2O"] + 1), _i(len(tt)), _d(tt), _d(a), _d(b), self._err)
            self._check()
        for p in t.particles:
            r, a, b, g = _c(p["radii"]), _c(p["w0"]), _c(p["qext"]), _c(p["gt"])
            L.radtran_add_particle(self._ptr, _i(p["p_ind"] + 1), _i(len(r)), _d(r), _d(a), _d(b), _d(g), self._err)
            self._check()
        iw, sw = _c(t.ir_wavl), _c(t.sol_wavl)
        L.radtran_set_channels(self._ptr, _i(len(iw)), _d(iw), _i(len(sw)), _d(sw), self._err)
        self._check()
        ps = _c(t.photons_sol)
        L.radtran_set_photons_sol(self._ptr, _i(len(ps)), _d(ps), self._err)
        self._check()
        L.radtran_create_end(self._ptr, _i(num_zenith_angles), _f(surface_albedo), self._err)
        self._check()
        self.nw = t.nw
        self.ngauss = t.ng
        # names for opacities2yaml (clima_radtran_types.f90:328-430)
        L.radtran_set_names(self._ptr, "\n".join(self.species_names).encode(), "\n".join(self.particle_names).encode(),
                            self._err)
        self._check()
        cont = t.continuum.get("model", "MT_CKD") if t.continuum is not None else ""
        L.radtran_set_opacity_labels(self._ptr, str(getattr(t, "k_method_name", "RandomOverlapResortRebin")).encode(),
                                     str(cont).encode(),
                                     "\n".join(str(p.get("dat_name", "unknown")) for p in t.particles).encode(), self._err)
        self._check()

    @classmethod
    def from_files(cls, settings_f, star_f, num_zenith_angles, surface_albedo, nz, datadir):
        """`Radtran(settings_f, star_f, num_zenith_angles, surface_albedo, nz, datadir, err)`
        (src/radtran/clima_radtran.f90:98-126): species and opacities from the settings YAML, tables
        from a `photochem_clima_data`-style directory (clima_amd/data_loader.py)."""
        from . import data_loader
        return cls(data_loader.load_tables(settings_f, star_f, datadir), nz, num_zenith_angles, surface_albedo)

    @classmethod
    def from_files_c(cls, settings_f, star_f, num_zenith_angles, surface_albedo, nz, datadir):
        """The same constructor with the files read BEHIND the C ABI (radtran_create_from_files,
        clima_amd/csrc/radtran_loader.hip): what a Fortran / C host without the reference's loaders calls."""
        self = cls.__new__(cls)
        L = _lib.load()
        self._L = L
        self._ptr = C.c_void_p()
        L.allocate_radtran(C.byref(self._ptr))
        self._err = C.create_string_buffer(_lib.ERR_LEN + 1)
        L.radtran_create_from_files(self._ptr, str(settings_f).encode(), str(star_f).encode(), _i(num_zenith_angles),
                                    _f(surface_albedo), _i(nz), str(datadir).encode(), self._err)
        self._check()
        d = [C.c_int() for _ in range(5)]
        L.radtran_dims_get(self._ptr, *[C.byref(x) for x in d])
        self.nz, self.ng, self.np, self.nw, self.ngauss = (x.value for x in d)
        a, b = C.create_string_buffer(4096), C.create_string_buffer(4096)
        L.radtran_names_get(self._ptr, _i(4096), a, b)
        self.species_names = [x for x in a.value.decode().split("\n") if x]
        self.particle_names = [x for x in b.value.decode().split("\n") if x]
        return self

    def __del__(self):
        if getattr(self, "_ptr", None) is not None and self._ptr.value:
            if getattr(self, "_locked", None):
                self._L.radtran_spectra_release(self._ptr)
            self._L.deallocate_radtran(self._ptr)
            self._ptr = C.c_void_p()

    def _check(self):
        msg = self._err.value
        if len(msg.strip()) > 0:
            raise ClimaException(msg.decode("utf-8").strip())

    # ------------------------------------------------------------------ the path
    def _column_args(self, T, P, densities, dz, pdensities, radii):
        T, P, dz = _c(T), _c(P), _c(dz)
        densities = _fo(densities)
        if densities.ndim != 2:
            raise ClimaException('"densities" has the wrong input dimension.')
        has_p = pdensities is not None or radii is not None
        if has_p and (pdensities is None or radii is None):
            raise ClimaException("Both pdensities and radii must be arguments.")
        if has_p:
            pdensities, radii = _fo(pdensities), _fo(radii)
            p1, p2 = pdensities.shape if pdensities.ndim == 2 else (pdensities.shape[0], 1)
            r1, r2 = radii.shape if radii.ndim == 2 else (radii.shape[0], 1)
            pd, ra = _d(pdensities), _d(radii)
        else:
            p1 = p2 = r1 = r2 = 0
            pd = ra = None
        keep = (T, P, dz, densities, pdensities, radii)
        args = (_i(len(T)), _d(T), _i(len(P)), _d(P), _i(densities.shape[0]), _i(densities.shape[1]), _d(densities),
                _i(len(dz)), _d(dz), _i(1 if has_p else 0), _i(p1), _i(p2), pd, _i(r1), _i(r2), ra)
        return keep, args

    def radiate(self, T_surface, T, P, densities, dz, pdensities=None, radii=None, compute_solar=True,
                compute_opacity=True):
        """Radtran%radiate (clima_radtran.f90:221-318).  T (K), P (bar), densities (nz,ng)
        molecules/cm^3, dz (cm); fills wrk_ir, wrk_sol and f_total."""
        keep, a = self._column_args(T, P, densities, dz, pdensities, radii)
        self._L.radtran_radiate_wrapper(self._ptr, _f(T_surface), *a, _i(compute_solar), _i(compute_opacity),
                                        self._err)
        del keep
        self._check()

    def TOA_fluxes(self, T_surface, T, P, densities, dz, pdensities=None, radii=None, compute_solar=True,
                   compute_opacity=True):
        """Radtran%TOA_fluxes (clima_radtran.f90:320-342) -> (ISR, OLR) in mW/m^2."""
        keep, a = self._column_args(T, P, densities, dz, pdensities, radii)
        isr, olr = C.c_double(), C.c_double()
        self._L.radtran_toa_fluxes_wrapper(self._ptr, _f(T_surface), *a, _i(compute_solar), _i(compute_opacity),
                                           C.byref(isr), C.byref(olr), self._err)
        del keep
        self._check()
        return isr.value, olr.value

    def bench_toa_fluxes(self, n, T_surface, T, P, densities, dz, pdensities=None, radii=None):
        """`n` synchronous TOA_fluxes calls timed one by one INSIDE the library (us per call, numpy array):
        the drop-in call as a Fortran / C host sees it, without the ctypes layer's own cost."""
        keep, a = self._column_args(T, P, densities, dz, pdensities, radii)
        us = np.zeros(int(n))
        isr, olr = C.c_double(), C.c_double()
        self._L.clima_bench_toa_fluxes(self._ptr, _i(n), _f(T_surface), *a, _d(us), C.byref(isr), C.byref(olr), self._err)
        del keep
        self._check()
        return us

    def bench_resident_sync(self, n):
        """`n` times radiate_resident + synchronize, timed one by one inside the library (us per call)."""
        us = np.zeros(int(n))
        self._L.clima_bench_resident_sync(self._ptr, _i(n), _d(us), self._err)
        self._check()
        return us

    def bench_resident_graph(self, n, k=1):
        """Timing only: one resident call's launches as a hipGraph, `n` passes of `k` graph launches + synchronize (us
        per pass); the replayed results are not valid."""
        us = np.zeros(int(n))
        self._L.clima_bench_resident_graph(self._ptr, _i(n), _i(k), _d(us), self._err)
        self._check()
        return us

    def apply_radiation_enhancement(self, rad_enhancement):
        self._L.radtran_apply_radiation_enhancement(self._ptr, _f(rad_enhancement))

    def opacities2yaml(self):
        """Radtran%opacities2yaml (clima/cython/Radtran.pyx:68-81): YAML text naming every opacity."""
        n, cp = C.c_int(), C.c_void_p()
        self._L.radtran_opacities2yaml_wrapper_1(self._ptr, C.byref(n), C.byref(cp))
        buf = C.create_string_buffer(n.value + 1)
        self._L.radtran_opacities2yaml_wrapper_2(self._ptr, C.byref(cp), C.byref(n), buf)
        return buf.value.decode()

    def set_custom_optical_properties(self, wv, P, dtau_dz, w0, g0):
        """Radtran%set_custom_optical_properties (src/radtran/clima_radtran.f90:494-506): `wv` nm,
        `P` dynes/cm^2 (decreasing), `dtau_dz` 1/cm, `w0`, `g0` of shape (size(P), size(wv))."""
        wv, P = _c(wv), _c(P)
        arrs = [np.asfortranarray(x, dtype=np.float64) for x in (dtau_dz, w0, g0)]
        for a in arrs:
            if a.ndim != 2:
                raise ClimaException("`dtau_dz`, `w0` and `g0` must be 2-D arrays")
        args = []
        for a in arrs:
            args += [_i(a.shape[0]), _i(a.shape[1]), _d(a)]
        self._L.radtran_set_custom_optical_properties(self._ptr, _i(len(wv)), _d(wv), _i(len(P)), _d(P), *args, self._err)
        self._check()

    def unset_custom_optical_properties(self):
        """src/radtran/clima_radtran.f90:508-512"""
        self._L.radtran_unset_custom_optical_properties(self._ptr)

    SPECTRA = ("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a")
    SPECTRA_ALL = ("ir_fup_a", "ir_fdn_a", "ir_tau_band", "sol_fup_a", "sol_fdn_a", "sol_amean", "sol_tau_band")   # spectra_all's

    def _spectra_request(self, spectra_levels, spectra):
        """(levels 1..nz+1 as the ABI takes them, the names asked for in the ABI's order) of a batch's `spectra_levels`
        (numpy-style indices into the ground-first level axis) and `spectra`"""
        nl = self.nz + 1
        idx = np.atleast_1d(np.asarray(spectra_levels))
        if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
            raise ClimaException('toa_fluxes_batch_spectra: "spectra_levels" is not a list of integer level indices')
        for a, v in enumerate(idx.tolist()):
            if v < -nl or v >= nl:
                raise ClimaException("toa_fluxes_batch_spectra: spectra_levels[%d] = %d is outside %d..%d" % (a, v, -nl, nl - 1))
        spectra = (spectra,) if isinstance(spectra, str) else tuple(spectra)
        for name in spectra:
            if name not in self.SPECTRA:
                raise ClimaException('toa_fluxes_batch_spectra: "%s" is not one of %s' % (name, ", ".join(self.SPECTRA)))
        levels = np.ascontiguousarray(np.where(idx < 0, idx + nl, idx) + 1, dtype=np.int32)
        return levels, tuple(name for name in self.SPECTRA if name in spectra)

    BOUNDS = ("surface_albedo", "surface_emissivity", "zenith_u", "zenith_weights", "photon_scale_factor")   # the ABI's order

    def _bounds_request(self, bounds, n, dims, tensors=False):
        """The five per-column arrays of a bounds batch in the ABI's order (None: not given) out of the dict `bounds`:
        float64, C-contiguous, (n, nw_sol), (n, nw_ir), (n, nzen), (n, nzen), (n,) for dims = (nw_sol, nw_ir, nzen) --
        numpy arrays, or with `tensors` torch tensors, which are taken as they are or refused.  Unknown keys and wrong
        shapes are refused by name before anything is called."""
        who = "toa_fluxes_batch_bounds_device" if tensors else "toa_fluxes_batch_bounds"
        if not isinstance(bounds, dict):
            raise ClimaException('%s: "bounds" is not a dict of %s' % (who, ", ".join(self.BOUNDS)))
        for name in bounds:
            if name not in self.BOUNDS:
                raise ClimaException('%s: "%s" is not one of %s' % (who, name, ", ".join(self.BOUNDS)))
        nw_sol, nw_ir, nzen = dims
        shapes = dict(zip(self.BOUNDS, ((n, nw_sol), (n, nw_ir), (n, nzen), (n, nzen), (n,))))
        out = []
        for name in self.BOUNDS:
            a = bounds.get(name)
            if a is not None and tensors:
                import torch
                if not isinstance(a, torch.Tensor) or a.dtype != torch.float64:
                    raise ClimaException('%s: "%s" is not a float64 torch tensor' % (who, name))
                if not a.is_contiguous():
                    raise ClimaException('%s: "%s" is not C-contiguous' % (who, name))
            elif a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
            if a is not None and tuple(a.shape) != shapes[name]:
                raise ClimaException('%s: "%s" has the shape %s, not %s' % (who, name, tuple(a.shape), shapes[name]))
            out.append(a)
        return out

    def _bounds_dims(self):
        return len(self.sol.freq) - 1, len(self.ir.freq) - 1, len(self.zenith_u)

    def TOA_fluxes_batch(self, columns, return_fluxes=False, spectra_levels=None,
                         spectra=("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a"), bounds=None):
        """Many independent columns (BASELINE config 4): `columns` is a sequence of column dicts /
        `synthetic.Column`s (T_surface, T, P, densities, dz[, pdensities, radii]).  Returns
        (ISR, OLR) arrays, plus the level fluxes (nz+1, 5, ncol) = ir up, ir down, solar up,
        solar down, f_total when `return_fluxes`.

        `spectra_levels` (radtran_toa_fluxes_batch_spectra): numpy-style indices into the ground-first level axis
        (0 the ground, -1 or nz the top of the atmosphere; any order, repeats allowed) whose per-bin rows are wanted
        of EVERY column.  The return value then gains a last element, a dict name -> array (nsel, nw_channel, ncol)
        for the names in `spectra`: `d["ir_fup_a"][:, :, c]` is `wrk_ir.fup_a[spectra_levels, :]` as the handle would
        hold it after column c's own TOA_fluxes call, bit for bit.

        `bounds` (radtran_toa_fluxes_batch_bounds): a dict with any of `surface_albedo` (ncol, nw_sol),
        `surface_emissivity` (ncol, nw_ir), `zenith_u`, `zenith_weights` (ncol, nzen) and `photon_scale_factor` (ncol,):
        column c is computed as if these had been set on the handle before its own TOA_fluxes call, bit for bit; a
        field not given is the handle's for every column.  The handle's own fields are not changed."""
        n = len(columns)
        nz = self.nz
        Ts = np.array([float(c["T_surface"]) for c in columns])
        T = np.stack([np.asarray(c["T"], dtype=np.float64) for c in columns])           # (ncol, nz)
        P = np.stack([np.asarray(c["P"], dtype=np.float64) for c in columns])
        dz = np.stack([np.asarray(c["dz"], dtype=np.float64) for c in columns])
        dens = np.stack([np.asarray(c["densities"], dtype=np.float64).T for c in columns])  # (ncol, nsp, nz)
        if T.shape != (n, nz) or dens.shape != (n, self.ng, nz):
            raise ClimaException('"densities" has the wrong input dimension.')
        hp = self.np > 0
        if hp:
            if any(c.get("radii") is None for c in columns):
                raise ClimaException('"pdensities" and "radii" are required arguments.')
            pd = np.stack([np.asarray(c["pdensities"], dtype=np.float64).T for c in columns])
            ra = np.stack([np.asarray(c["radii"], dtype=np.float64).T for c in columns])
        else:
            pd = ra = np.zeros(1)
        isr, olr = np.empty(n), np.empty(n)
        fl = np.empty((n, 5, nz + 1)) if return_fluxes else None
        args = (self._ptr, _i(n), _d(Ts), _d(np.ascontiguousarray(T)), _d(np.ascontiguousarray(P)),
                _d(np.ascontiguousarray(dens)), _d(np.ascontiguousarray(dz)), _i(1 if hp else 0),
                _d(np.ascontiguousarray(pd)), _d(np.ascontiguousarray(ra)), _d(isr), _d(olr),
                _d(fl) if return_fluxes else None)
        out = (isr, olr, np.transpose(fl, (2, 1, 0))) if return_fluxes else (isr, olr)
        bnd = None if bounds is None else self._bounds_request(bounds, n, self._bounds_dims())
        if spectra_levels is None:
            if bnd is None:
                self._L.radtran_toa_fluxes_batch(*args, self._err)
            else:
                self._L.radtran_toa_fluxes_batch_bounds(*args, *[_d(a) if a is not None else None for a in bnd], _i(0), None,
                                                        None, None, None, None, self._err)
            self._check()
            return out
        levels, names = self._spectra_request(spectra_levels, spectra)
        nw = {"ir": len(self.ir.freq) - 1, "sol": len(self.sol.freq) - 1}
        spec = {name: np.empty((n, len(levels), nw[name.split("_")[0]])) for name in names}
        ask = (_i(len(levels)), levels.ctypes.data_as(C.POINTER(C.c_int)), *[_d(spec[name]) if name in spec else None for name in self.SPECTRA])
        if bnd is None:
            self._L.radtran_toa_fluxes_batch_spectra(*args, *ask, self._err)
        else:
            self._L.radtran_toa_fluxes_batch_bounds(*args, *[_d(a) if a is not None else None for a in bnd], *ask, self._err)
        self._check()
        return out + ({name: np.transpose(a, (1, 2, 0)) for name, a in spec.items()},)

    def TOA_fluxes_batch_tensors(self, T_surface, T, P, densities, dz, pdensities=None, radii=None, return_fluxes=False,
                                 sync=True, spectra_levels=None, spectra=("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a"),
                                 bounds=None):
        """`TOA_fluxes_batch` for columns that live in device memory (radtran_toa_fluxes_batch_device): torch CUDA
        float64 tensors, C-contiguous, T_surface (ncol,); T, P, dz (ncol, nz); densities (ncol, nsp, nz);
        pdensities / radii (ncol, np, nz).  Nothing passes through the host.  Returns fresh tensors on the same
        device: ISR, OLR (ncol,), plus the level fluxes (ncol, 5, nz+1) = ir up, ir down, solar up, solar down,
        f_total when `return_fluxes` -- bit for bit what `TOA_fluxes_batch` gives for the same columns.

        The library's work is ordered behind what torch's current stream has enqueued.  With `sync=True` the call
        ends with `synchronize()`.  With `sync=False` it returns at once, torch's current stream ordered behind the
        handle's: the tensors are FINAL ONLY AFTER `synchronize()` -- that is where a fused hand-off wait that
        expired in the batch is found, and the batch is then computed again, unfused, into the same tensors
        (`fused_fallbacks` + 1), and where an opacity failure is raised.  Keep inputs and outputs alive until then.

        `spectra_levels`, `spectra`: as in `TOA_fluxes_batch` (radtran_toa_fluxes_batch_spectra_device); the return
        value gains a last element, a dict name -> fresh tensor (ncol, nsel, nw_channel) on the same device, equal
        to the host form's arrays and final under the same rule: after `synchronize()`, which refills them too when
        it repeats the batch.

        `bounds`: as in `TOA_fluxes_batch`, the arrays torch CUDA float64 tensors of the same shapes
        (radtran_toa_fluxes_batch_bounds_device); a repeat of the batch runs under the same bounds, so keep them alive
        until `synchronize()` as well."""
        import torch
        nz, hp = self.nz, self.np > 0
        if hp and (pdensities is None or radii is None):
            raise ClimaException('"pdensities" and "radii" are required arguments.')
        n = int(T_surface.shape[0]) if isinstance(T_surface, torch.Tensor) and T_surface.dim() == 1 else -1
        want = [("T_surface", T_surface, (n,)), ("T", T, (n, nz)), ("P", P, (n, nz)), ("densities", densities, (n, self.ng, nz)),
                ("dz", dz, (n, nz))]
        if hp:
            want += [("pdensities", pdensities, (n, self.np, nz)), ("radii", radii, (n, self.np, nz))]
        for name, t, shape in want:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise ClimaException('toa_fluxes_batch_device: "%s" is not a float64 torch tensor' % name)
            if tuple(t.shape) != shape:
                raise ClimaException('"%s" has the wrong input dimension.' % name)
            if not t.is_contiguous():   # (no silent copy: the caller decides where a transposed view is materialised)
                raise ClimaException('toa_fluxes_batch_device: "%s" is not C-contiguous' % name)
        bnd = None if bounds is None else self._bounds_request(bounds, n, self._bounds_dims(), tensors=True)
        # (a tensor that is not on the handle's device is refused by the library, which names it)
        dev = next((t.device for _, t, _ in want if t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
        isr, olr = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        fl = torch.empty((n, 5, nz + 1), dtype=torch.float64, device=dev) if return_fluxes else None

        def addr(t):
            return t.data_ptr() if t is not None else None

        spec = None
        if spectra_levels is not None:
            levels, names = self._spectra_request(spectra_levels, spectra)
            nw = {"ir": len(self.ir.freq) - 1, "sol": len(self.sol.freq) - 1}
            spec = {name: torch.empty((n, len(levels), nw[name.split("_")[0]]), dtype=torch.float64, device=dev) for name in names}
        cur = torch.cuda.current_stream(dev)
        mine = torch.cuda.ExternalStream(self.stream(), device=dev)
        producer = cur.cuda_stream
        if not producer:
            # the legacy default stream: NULL tells the library that the inputs are complete, so the order is made here
            mine.wait_stream(cur)
        args = (self._ptr, _i(n), addr(T_surface), addr(T), addr(P), addr(densities), addr(dz), _i(1 if hp else 0),
                addr(pdensities) if hp else None, addr(radii) if hp else None, addr(isr), addr(olr), addr(fl))
        if spec is None:
            ask = (_i(0), None, None, None, None, None)
        else:
            ask = (_i(len(levels)), levels.ctypes.data_as(C.POINTER(C.c_int)), *[addr(spec.get(name)) for name in self.SPECTRA])
        if bnd is not None:
            self._L.radtran_toa_fluxes_batch_bounds_device(*args, *[addr(a) for a in bnd], *ask, producer or None, self._err)
        elif spec is None:
            self._L.radtran_toa_fluxes_batch_device(*args, producer or None, self._err)
        else:
            self._L.radtran_toa_fluxes_batch_spectra_device(*args, *ask, producer or None, self._err)
        self._check()
        if sync:
            self.synchronize()
        else:
            ev = torch.cuda.Event()
            ev.record(mine)
            cur.wait_event(ev)
        out = (isr, olr, fl) if return_fluxes else (isr, olr)
        return out if spec is None else out + (spec,)

    def radiate_ir_batch(self, T_surface, T, out=None, pin=False):
        """ncol IR-only calls with the resident opacities in one go: column c is
        `radiate(T_surface[c], T[:, c], ..., compute_solar=False, compute_opacity=False)`
        (the RCE Jacobian's loop, src/adiabat/clima_adiabat_solve.f90:798-812).
        Returns (fup_n, fdn_n, f_total), each (nz+1, ncol).  `out` + `pin`: the caller's three arrays are page-locked from
        the second call with the same ones on and filled by the device directly (radtran_batch_pin_results_set); this
        object keeps them alive until spectra_release()."""
        T = np.asfortranarray(T, dtype=np.float64)
        Ts = _c(np.atleast_1d(T_surface))
        if T.ndim != 2 or T.shape[0] != self.nz or T.shape[1] != len(Ts):
            raise ClimaException('"T" has the wrong input dimension.')
        n = T.shape[1]
        pin = bool(pin) and out is not None
        if out is None:     # (out: three (nz+1, ncol) Fortran-ordered arrays to fill, as a caller that keeps its buffers would)
            out = [np.empty((self.nz + 1, n), order="F") for _ in range(3)]
        self._L.radtran_batch_pin_results_set(self._ptr, _i(1 if pin else 0))
        self._locked = getattr(self, "_locked", [])
        if pin and not any(out is o for o in self._locked):
            self._locked.append(out)
        self._L.radtran_radiate_ir_batch(self._ptr, _i(n), _d(Ts), _i(T.shape[0]), _i(n), _d(T),
                                         _d(out[0]), _d(out[1]), _d(out[2]), self._err)
        self._check()
        return tuple(out)

    SOLAR_BATCH_SPECTRA = ("fup", "fdn", "amean")

    def _solar_batch_request(self, dims, zenith_u, zenith_weights, surface_albedo, photon_scale_factor, spectra_levels, spectra):
        """The arrays of `radiate_solar_batch` as the ABI takes them -- (ncol, nzen, zenith_u, zenith_weights, surface_albedo
        or None, photon_scale_factor or None, levels 1..nz+1 or None, names in the ABI's order) -- for dims = (nz, nw_sol);
        wrong shapes and unknown spectrum names are refused by name (reads SOLAR_BATCH_SPECTRA alone: no handle needed)"""
        who = "radiate_solar_batch: "
        nz, nw_sol = dims
        u = _c(zenith_u)
        if u.ndim == 1:
            u = u.reshape(-1, 1)
            if zenith_weights is None:
                zenith_weights = np.ones_like(u)
            elif np.ndim(zenith_weights) == 1:
                zenith_weights = np.reshape(zenith_weights, (-1, 1))
        if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] < 1:
            raise ClimaException(who + '"zenith_u" has the shape %s, not (ncol,) or (ncol, nzen)' % (tuple(np.shape(zenith_u)),))
        n, nzen = u.shape
        if zenith_weights is None:
            raise ClimaException(who + '"zenith_weights" is required with a two-dimensional "zenith_u"')
        want = {"zenith_weights": (n, nzen), "surface_albedo": (n, nw_sol), "photon_scale_factor": (n,)}
        got = {"zenith_weights": zenith_weights, "surface_albedo": surface_albedo, "photon_scale_factor": photon_scale_factor}
        for name, a in got.items():
            if a is None:
                continue
            a = _c(a)
            if a.shape != want[name]:
                raise ClimaException(who + '"%s" has the shape %s, not %s' % (name, a.shape, want[name]))
            got[name] = a
        levels, names = None, ()
        if spectra_levels is not None:
            nl = nz + 1
            idx = np.atleast_1d(np.asarray(spectra_levels))
            if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
                raise ClimaException(who + '"spectra_levels" is not a list of integer level indices')
            for a, v in enumerate(idx.tolist()):
                if v < -nl or v >= nl:
                    raise ClimaException(who + "spectra_levels[%d] = %d is outside %d..%d" % (a, v, -nl, nl - 1))
            spectra = (spectra,) if isinstance(spectra, str) else tuple(spectra)
            for name in spectra:
                if name not in self.SOLAR_BATCH_SPECTRA:
                    raise ClimaException(who + '"%s" is not one of %s' % (name, ", ".join(self.SOLAR_BATCH_SPECTRA)))
            levels = np.ascontiguousarray(np.where(idx < 0, idx + nl, idx) + 1, dtype=np.int32)
            names = tuple(name for name in self.SOLAR_BATCH_SPECTRA if name in spectra)
        return n, nzen, u, got["zenith_weights"], got["surface_albedo"], got["photon_scale_factor"], levels, names

    def radiate_solar_batch(self, zenith_u, zenith_weights=None, surface_albedo=None, photon_scale_factor=None,
                            spectra_levels=None, spectra=("fup", "fdn", "amean")):
        """ncol solar calls on the resident opacities in one go (radtran_radiate_solar_batch): case c is
        `radiate(..., compute_solar=True, compute_opacity=False)` after `zenith_u`, `zenith_weights`, `surface_albedo` and
        `photon_scale_factor` had been set to the case's.  Arrays carry the case first: `zenith_u`, `zenith_weights` (ncol,
        nzen) -- nzen is the batch's own, 1..16; a 1-D `zenith_u` means one angle of weight 1 per case --, `surface_albedo`
        (ncol, nw_sol), `photon_scale_factor` (ncol,); None: the handle's current value.  Returns (fup_n, fdn_n, f_total),
        each (nz+1, ncol), f_total = (fdn_n - fup_n) plus the IR rows of the handle's last IR call; with `spectra_levels`
        (numpy-style indices into the ground-first level axis) also a dict name -> (nsel, nw_sol, ncol) for the names in
        `spectra` ("fup", "fdn", "amean": wrk_sol.fup_a / fdn_a / amean at those levels).  The handle's state is left
        untouched."""
        nz, nw_sol = self.nz, len(self.sol.freq) - 1
        n, nzen, u, w, alb, scale, levels, names = self._solar_batch_request(
            (nz, nw_sol), zenith_u, zenith_weights, surface_albedo, photon_scale_factor, spectra_levels, spectra)
        out = [np.empty((nz + 1, n), order="F") for _ in range(3)]
        spec = {name: np.empty((len(levels), nw_sol, n)) for name in names}
        opt = lambda a: _d(a) if a is not None else None   # noqa: E731
        self._L.radtran_radiate_solar_batch(
            self._ptr, _i(n), _i(nzen), _d(u), _d(w), opt(alb), opt(scale), _d(out[0]), _d(out[1]), _d(out[2]),
            _i(0 if levels is None else len(levels)), None if levels is None else levels.ctypes.data_as(C.POINTER(C.c_int)),
            *[opt(spec.get(name)) for name in self.SOLAR_BATCH_SPECTRA], self._err)
        self._check()
        # (the ABI's (nw_sol, nsel, ncol) column-major is (ncol, nsel, nw_sol) in C order)
        spec = {k: np.ascontiguousarray(v.reshape(n, len(levels), nw_sol).transpose(1, 2, 0)) for k, v in spec.items()}
        return tuple(out) if levels is None else tuple(out) + (spec,)

    def solar_batch_shared(self, on=None):
        """(on, batches): whether `radiate_solar_batch` may take the shared kernel, and the batches that took it so far;
        `on` 0 / 1 sets it first (radtran_solar_batch_shared_set / _get: for tests and measurements)"""
        if on is not None:
            self._L.radtran_solar_batch_shared_set(self._ptr, _i(1 if on else 0))
        a, b = C.c_int(), C.c_int()
        self._L.radtran_solar_batch_shared_get(self._ptr, C.byref(a), C.byref(b))
        return a.value, b.value

    def ir_jacobian(self, T_surface, T):
        """The exact IR temperature Jacobian of the level fluxes at the resident opacities (radtran_ir_jacobian):
        (jac_up, jac_dn, jac_total), each (nz+1, nz+1) Fortran-ordered, [i, j] = d flux(level i, ground-first) / d x(j)
        with x(0) = T_surface, x(1 + m) = T[m]; mW m^-2 K^-1.  The limit of the RCE Jacobian's one-sided differences
        (src/adiabat/clima_adiabat_solve.f90:768-822) as the step goes to 0."""
        T, Ts = _c(np.atleast_1d(T)), _c(np.atleast_1d(T_surface))
        if T.ndim != 1 or Ts.shape != (1,):
            raise ClimaException('"T" has the wrong input dimension.')
        nl = self.nz + 1
        out = [np.empty((nl, nl), order="F") for _ in range(3)]
        self._L.radtran_ir_jacobian(self._ptr, _d(Ts), _i(len(T)), _d(T), _i(nl), _i(nl),
                                    _d(out[0]), _d(out[1]), _d(out[2]), self._err)
        self._check()
        return tuple(out)

    def ir_jacobian_reduced(self, T_surface, T, group_of_x, rows=None, parts=False):
        """`ir_jacobian` in the caller's unknowns (radtran_ir_jacobian_reduced): `group_of_x[j]` (nz+1 entries, one per
        x of `ir_jacobian`) is 0 for an x held fixed or the unknown 1..ngroup it moves with (ngroup = the largest
        entry); `rows` are the levels wanted, 1..nz+1 ground-first (None: every level).  Returns jac_total
        (nrow, ngroup), Fortran-ordered: [a, g-1] = sum over the members j of group g, ascending, of
        jac_total[rows[a]-1, j]; with `parts` (jac_up, jac_dn, jac_total).  `atmosphere.rce_jacobian_map` builds the map
        of AdiabatClimate's solver (doubled radiative grid, ghost layers, convective zones)."""
        T, Ts = _c(np.atleast_1d(T)), _c(np.atleast_1d(T_surface))
        if T.ndim != 1 or Ts.shape != (1,):
            raise ClimaException('"T" has the wrong input dimension.')
        grp = np.ascontiguousarray(np.atleast_1d(group_of_x), dtype=np.int32)
        rows = np.arange(1, self.nz + 2) if rows is None else rows
        rows = np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
        if grp.ndim != 1:
            raise ClimaException('ir_jacobian_reduced: "group_of_x" has the wrong dimension (%d axes, one expected)' % grp.ndim)
        if rows.ndim != 1:
            raise ClimaException('ir_jacobian_reduced: "rows" has the wrong dimension (%d axes, one expected)' % rows.ndim)
        ngroup, nrow = int(grp.max()) if grp.size else 0, len(rows)
        out = [np.empty((nrow, max(ngroup, 0)), order="F") if (parts or i == 2) else None for i in range(3)]
        ip = C.POINTER(C.c_int)
        self._L.radtran_ir_jacobian_reduced(self._ptr, _d(Ts), _i(len(T)), _d(T), _i(len(grp)), grp.ctypes.data_as(ip),
                                            _i(ngroup), _i(nrow), rows.ctypes.data_as(ip), _i(nrow), _i(ngroup),
                                            _d(out[0]) if parts else None, _d(out[1]) if parts else None, _d(out[2]),
                                            self._err)
        self._check()
        return tuple(out) if parts else out[2]

    IR_JACOBIAN_SPECTRAL_PARTS = ("up", "dn")

    def _ir_jacobian_spectral_request(self, nz, T_surface, T, levels, parts):
        """The arrays of `ir_jacobian_spectral` as the ABI takes them -- (T_surface, T, levels 1..nz+1, names in the
        ABI's order) -- for a handle of nz layers; wrong shapes, unknown parts and levels outside -(nz+1)..nz are refused
        by name (reads IR_JACOBIAN_SPECTRAL_PARTS alone: no handle needed)"""
        who = "ir_jacobian_spectral: "
        Ts, T = _one_column(who, nz, T_surface, T)
        names = _names_among(who, "parts", parts, self.IR_JACOBIAN_SPECTRAL_PARTS)
        return Ts, T, _level_rows(who, nz, levels), names

    def ir_jacobian_spectral(self, T_surface, T, levels=(-1,), parts=("up",)):
        """Rows of `ir_jacobian` before the sum over the bins (radtran_ir_jacobian_spectral_rows): a dict name ->
        (nw_ir, nrow, nz+1) Fortran-ordered array for the names in `parts` ("up", "dn"), [l, a, j] = d wrk_ir.fup_a (fdn_a)
        [levels[a], l] / d x(j) with x(0) = T_surface, x(1 + m) = T[m]; mW m^-2 Hz^-1 K^-1.  `levels` are numpy-style indices
        into the ground-first level axis (-1: the top of the atmosphere, 0: the surface), repeats allowed.  Times the bins'
        widths and summed over l it is `ir_jacobian`'s row.  One adjoint two-stream solve per (bin, g-point, row,
        direction); the handle's state is left untouched."""
        Ts, T, rows, names = self._ir_jacobian_spectral_request(self.nz, T_surface, T, levels, parts)
        nw_ir, nrow, nl = len(self.ir.freq) - 1, len(rows), self.nz + 1
        out = {name: np.empty((nw_ir, nrow, nl), order="F") for name in names}
        self._L.radtran_ir_jacobian_spectral_rows(
            self._ptr, _d(Ts), _i(len(T)), _d(T), _i(nrow), rows.ctypes.data_as(C.POINTER(C.c_int)), _i(nw_ir), _i(nrow), _i(nl),
            *[_d(out[name]) if name in out else None for name in self.IR_JACOBIAN_SPECTRAL_PARTS], self._err)
        self._check()
        return out

    IR_SPECTRA_BATCH_PARTS = ("up", "dn")

    def _ir_spectra_batch_request(self, nz, T_surface, T, levels, parts, weights):
        """The arrays of `ir_spectra_batch` as the ABI takes them -- (T_surface (ncol), T (nz, ncol) Fortran-ordered, levels
        1..nz+1, names in the ABI's order) -- for a handle of nz layers; wrong shapes, unknown parts, levels outside
        -(nz+1)..nz and a request that names no output are refused by name (reads IR_SPECTRA_BATCH_PARTS alone: no handle
        needed).  T_surface None with T None: no columns, the weights alone."""
        who = "ir_spectra_batch: "
        if T is None and T_surface is None:
            T, T_surface = np.empty((nz, 0), order="F"), np.empty(0)
        Ts, T = _column_batch(who, nz, T_surface, T, 0)
        names = _names_among(who, "parts", parts, self.IR_SPECTRA_BATCH_PARTS)
        if len(Ts) == 0 and not weights:
            raise ClimaException(who + "no columns and weights=False: nothing is asked for")
        return Ts, T, _level_rows(who, nz, levels), names

    def ir_spectra_batch(self, T_surface, T, levels=(-1,), parts=("up",), fluxes=False, weights=False):
        """Per-bin IR spectra of many temperature profiles on the stored opacities (radtran_ir_spectra_batch): column c is
        `radiate(T_surface[c], T[:, c], ..., compute_solar=False, compute_opacity=False)` read at `wrk_ir.fup_a / fdn_a
        [levels[a], l]`, without a solve per column.  Returns a dict of Fortran-ordered arrays for the directions in `parts`
        ("up", "dn"): "fup" / "fdn" (nw_ir, nsel, ncol); with `fluxes` also "fup_n" / "fdn_n" (nsel, ncol), the spectra
        summed over the bins times their widths (`wrk_ir.fup_n[levels[a]]`); with `weights` also "w_up" / "w_dn"
        (nw_ir, nsel, nz+1), the temperature-independent weights with fup[l, a, c] = sum_j w_up[l, a, j] B(avg_freq[l], x_c[j]),
        x_c[0] = T_surface[c], x_c[1 + m] = T[m, c].  `levels` are numpy-style indices into the ground-first level axis
        (-1: the top of the atmosphere, 0: the surface), repeats allowed.  T_surface = T = None with `weights`: the weights
        alone.  One adjoint pass per call, then Planck values and FMAs per column; the handle's state is left untouched."""
        Ts, T, rows, names = self._ir_spectra_batch_request(self.nz, T_surface, T, levels, parts, weights)
        nw_ir, nsel, nl, n = len(self.ir.freq) - 1, len(rows), self.nz + 1, len(Ts)
        out = {}
        for name in names:
            if n > 0:
                out["f" + name] = np.empty((nw_ir, nsel, n), order="F")
                if fluxes:
                    out["f%s_n" % name] = np.empty((nsel, n), order="F")
            if weights:
                out["w_" + name] = np.empty((nw_ir, nsel, nl), order="F")
        ptr = lambda key: _d(out[key]) if key in out else None   # noqa: E731
        self._L.radtran_ir_spectra_batch(
            self._ptr, _i(n), _d(Ts), _i(T.shape[0]), _i(n), _d(T), _i(nsel), rows.ctypes.data_as(C.POINTER(C.c_int)),
            ptr("fup"), ptr("fdn"), ptr("fup_n"), ptr("fdn_n"), ptr("w_up"), ptr("w_dn"), self._err)
        self._check()
        return out

    IR_SPECTRA_VJP_WEIGHTS = ("w_up", "w_dn")
    IR_SPECTRA_VJP_GRADS = ("fup", "fdn", "fup_n", "fdn_n")

    def _ir_spectra_vjp_request(self, nz, nw_ir, T_surface, T, weights, grads):
        """The arrays of `ir_spectra_vjp` as the ABI takes them -- (T_surface (ncol), T (nz, ncol), nsel, the two weights and
        the four cotangents in the ABI's order, None where absent), all Fortran-ordered float64 -- for a handle of nz
        layers and nw_ir IR bins; unknown keys, wrong shapes, a cotangent without its weights and a request without any
        cotangent are refused by name (reads the two name lists alone: no handle needed)."""
        who = "ir_spectra_vjp: "
        Ts, T = _column_batch(who, nz, T_surface, T, 1)
        n = len(Ts)
        _keys_among(who, "weights", weights, self.IR_SPECTRA_VJP_WEIGHTS)
        _keys_among(who, "grads", grads, self.IR_SPECTRA_VJP_GRADS)
        w = [np.asfortranarray(weights[k], dtype=np.float64) if weights.get(k) is not None else None for k in self.IR_SPECTRA_VJP_WEIGHTS]
        g = [np.asfortranarray(grads[k], dtype=np.float64) if grads.get(k) is not None else None for k in self.IR_SPECTRA_VJP_GRADS]
        if w[0] is None and w[1] is None:
            raise ClimaException(who + '"weights" holds none of %s' % ", ".join(self.IR_SPECTRA_VJP_WEIGHTS))
        if all(a is None for a in g):
            raise ClimaException(who + '"grads" holds none of %s' % ", ".join(self.IR_SPECTRA_VJP_GRADS))
        first = w[0] if w[0] is not None else w[1]
        nsel = first.shape[1] if first.ndim == 3 else -1
        for k, a in zip(self.IR_SPECTRA_VJP_WEIGHTS, w):
            if a is not None and (nsel < 1 or a.shape != (nw_ir, nsel, nz + 1)):
                raise ClimaException(who + '"%s" has the shape %s, not (%d, nsel, %d)' % (k, a.shape, nw_ir, nz + 1))
        for k, a in zip(self.IR_SPECTRA_VJP_GRADS, g):
            want = (nsel, n) if k.endswith("_n") else (nw_ir, nsel, n)
            if a is not None and a.shape != want:
                raise ClimaException(who + '"%s" has the shape %s, not %s' % (k, a.shape, want))
            if a is not None and w[0 if "up" in k else 1] is None:
                raise ClimaException(who + '"%s" was given without "%s"' % (k, "w_up" if "up" in k else "w_dn"))
        return Ts, T, nsel, w, g

    def ir_spectra_vjp(self, T_surface, T, weights, grads):
        """The temperature gradient of `ir_spectra_batch` (radtran_ir_spectra_batch_vjp): `weights` is the dict of
        "w_up" / "w_dn" (nw_ir, nsel, nz+1) a call with `weights=True` returned, `grads` a dict of cotangents with
        `ir_spectra_batch`'s keys and shapes -- "fup" / "fdn" (nw_ir, nsel, ncol), "fup_n" / "fdn_n" (nsel, ncol), an
        absent one counting as 0.  Returns (grad_T_surface (ncol,), grad_T (nz, ncol)): the derivatives of the loss whose
        derivatives with respect to the outputs `grads` are, with respect to T_surface[c] and T[m, c].  No solve and no
        opacities: one dB/dT per (bin, level, column); bitwise repeatable; the handle's state is left untouched."""
        nz, nw_ir = self.nz, len(self.ir.freq) - 1
        Ts, T, nsel, w, g = self._ir_spectra_vjp_request(nz, nw_ir, T_surface, T, weights, grads)
        n = len(Ts)
        gTs, gT = np.empty(n), np.empty((nz, n), order="F")
        ptr = lambda a: _d(a) if a is not None else None   # noqa: E731
        self._L.radtran_ir_spectra_batch_vjp(self._ptr, _i(n), _d(Ts), _i(nz), _i(n), _d(T), _i(nsel), ptr(w[0]), ptr(w[1]),
                                             ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), _d(gTs), _d(gT), self._err)
        self._check()
        return gTs, gT

    def _ir_tensor_check(self, who, name, t, shape):
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ClimaException('%s: "%s" is not a float64 torch tensor' % (who, name))
        if tuple(t.shape) != tuple(shape):
            raise ClimaException('%s: "%s" has the shape %s, not %s' % (who, name, tuple(t.shape), tuple(shape)))
        if not t.is_contiguous():   # (no silent copy: the caller decides where a transposed view is materialised)
            raise ClimaException('%s: "%s" is not C-contiguous' % (who, name))

    def _on_handle_stream(self, dev, call, sync):
        """`call(producer)` enqueues on the handle's stream; ordered as `TOA_fluxes_batch_tensors` orders its call: behind
        torch's current stream on `dev`, and that stream behind the handle's afterwards (sync: `synchronize()` instead)"""
        import torch
        cur = torch.cuda.current_stream(dev)
        mine = torch.cuda.ExternalStream(self.stream(), device=dev)
        producer = cur.cuda_stream
        if not producer:
            # the legacy default stream: NULL tells the library that the inputs are complete, so the order is made here
            mine.wait_stream(cur)
        call(producer or None)
        self._check()
        if sync:
            self.synchronize()
        else:
            ev = torch.cuda.Event()
            ev.record(mine)
            cur.wait_event(ev)

    def ir_spectra_batch_tensors(self, T_surface, T, levels=(-1,), parts=("up",), fluxes=False, weights=None,
                                 return_weights=False, sync=False):
        """`ir_spectra_batch` for profiles that live in device memory (radtran_ir_spectra_batch_device): torch CUDA float64
        tensors, C-contiguous with the column first -- T_surface (ncol,), T (ncol, nz) -- the `TOA_fluxes_batch_tensors`
        convention; nothing passes through the host, nothing is copied, a tensor that is not contiguous is refused.
        Returns a dict of fresh tensors on the same device: "fup" / "fdn" (ncol, nsel, nw_ir); with `fluxes` "fup_n" /
        "fdn_n" (ncol, nsel); with `return_weights` "w_up" / "w_dn" (nz+1, nsel, nw_ir) -- bit for bit `ir_spectra_batch`'s
        arrays, transposed.

        `weights`: None computes the weights from the stored opacities (one adjoint pass).  The dict of "w_up" / "w_dn" an
        earlier call with the same `levels` returned under `return_weights` is used as it is: no adjoint pass runs, the
        handle needs no opacities, and the results are bit for bit those of the call that computed them.  Their validity is
        the caller's: they describe the atmosphere, the emissivity, has_hard_surface and ir_tau_min of that call.

        The library's work is ordered behind what torch's current stream has enqueued.  With `sync=False` the call returns
        at once, torch's current stream ordered behind the handle's: work enqueued on it afterwards sees the results; the
        host may read them after `synchronize()`.  The temperatures are not checked (that would need a host read): a T
        that is not positive gives whatever the Planck function gives for it."""
        import torch
        who = "ir_spectra_batch_device"
        nz, nl, nw_ir = self.nz, self.nz + 1, len(self.ir.freq) - 1
        names = _names_among(who + ": ", "parts", parts, self.IR_SPECTRA_BATCH_PARTS)
        rows = _level_rows(who + ": ", nz, levels)
        nsel = len(rows)
        n = int(T_surface.shape[0]) if isinstance(T_surface, torch.Tensor) and T_surface.dim() == 1 else -1
        self._ir_tensor_check(who, "T_surface", T_surface, (max(n, 1),))
        self._ir_tensor_check(who, "T", T, (n, nz))
        if weights is not None:
            if not isinstance(weights, dict):
                raise ClimaException('%s: "weights" is not a dict with keys among w_up, w_dn' % who)
            for name in names:
                if weights.get("w_" + name) is None:
                    raise ClimaException('%s: "weights" lacks "w_%s"' % (who, name))
                self._ir_tensor_check(who, "w_" + name, weights["w_" + name], (nl, nsel, nw_ir))
        dev = T.device if T.is_cuda else torch.device("cuda", torch.cuda.current_device())
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
        out, w = {}, {}
        for name in names:
            out["f" + name] = new(n, nsel, nw_ir)
            if fluxes:
                out["f%s_n" % name] = new(n, nsel)
            if weights is not None:
                w["w_" + name] = weights["w_" + name]
            elif return_weights:
                w["w_" + name] = new(nl, nsel, nw_ir)
        addr = lambda d, key: d[key].data_ptr() if key in d else None   # noqa: E731
        self._on_handle_stream(dev, lambda producer: self._L.radtran_ir_spectra_batch_device(
            self._ptr, _i(n), T_surface.data_ptr(), _i(nz), _i(n), T.data_ptr(), _i(nsel), rows.ctypes.data_as(C.POINTER(C.c_int)),
            addr(out, "fup"), addr(out, "fdn"), addr(out, "fup_n"), addr(out, "fdn_n"), addr(w, "w_up"), addr(w, "w_dn"),
            _i(0 if weights is None else 1), producer, self._err), sync)
        if return_weights:
            out.update(w)
        return out

    def ir_spectra_vjp_tensors(self, T_surface, T, weights, grads, sync=False):
        """`ir_spectra_vjp` on torch CUDA float64 tensors in `ir_spectra_batch_tensors`' layout
        (radtran_ir_spectra_batch_vjp_device): `weights` "w_up" / "w_dn" (nz+1, nsel, nw_ir), `grads` "fup" / "fdn"
        (ncol, nsel, nw_ir), "fup_n" / "fdn_n" (ncol, nsel).  Returns fresh tensors (grad_T_surface (ncol,), grad_T
        (ncol, nz)), bit for bit the host form's; stream ordering and `sync` as in `ir_spectra_batch_tensors`."""
        import torch
        who = "ir_spectra_batch_vjp_device"
        nz, nl, nw_ir = self.nz, self.nz + 1, len(self.ir.freq) - 1
        _keys_among(who + ": ", "weights", weights, self.IR_SPECTRA_VJP_WEIGHTS)
        _keys_among(who + ": ", "grads", grads, self.IR_SPECTRA_VJP_GRADS)
        w = {k: v for k, v in weights.items() if v is not None}
        g = {k: v for k, v in grads.items() if v is not None}
        if not w:
            raise ClimaException('%s: "weights" holds none of %s' % (who, ", ".join(self.IR_SPECTRA_VJP_WEIGHTS)))
        if not g:
            raise ClimaException('%s: "grads" holds none of %s' % (who, ", ".join(self.IR_SPECTRA_VJP_GRADS)))
        n = int(T_surface.shape[0]) if isinstance(T_surface, torch.Tensor) and T_surface.dim() == 1 else -1
        self._ir_tensor_check(who, "T_surface", T_surface, (max(n, 1),))
        self._ir_tensor_check(who, "T", T, (n, nz))
        first = next(iter(w.values()))
        nsel = int(first.shape[1]) if isinstance(first, torch.Tensor) and first.dim() == 3 else 1
        for k, t in w.items():
            self._ir_tensor_check(who, k, t, (nl, nsel, nw_ir))
        for k, t in g.items():
            self._ir_tensor_check(who, k, t, (n, nsel) if k.endswith("_n") else (n, nsel, nw_ir))
            if ("w_up" if "up" in k else "w_dn") not in w:
                raise ClimaException('%s: "%s" was given without "%s"' % (who, k, "w_up" if "up" in k else "w_dn"))
        dev = T.device if T.is_cuda else torch.device("cuda", torch.cuda.current_device())
        gTs, gT = torch.empty(n, dtype=torch.float64, device=dev), torch.empty((n, nz), dtype=torch.float64, device=dev)
        addr = lambda d, key: d[key].data_ptr() if key in d else None   # noqa: E731
        self._on_handle_stream(dev, lambda producer: self._L.radtran_ir_spectra_batch_vjp_device(
            self._ptr, _i(n), T_surface.data_ptr(), _i(nz), _i(n), T.data_ptr(), _i(nsel), addr(w, "w_up"), addr(w, "w_dn"),
            addr(g, "fup"), addr(g, "fdn"), addr(g, "fup_n"), addr(g, "fdn_n"), gTs.data_ptr(), gT.data_ptr(), producer, self._err), sync)
        return gTs, gT

    IR_SPECTRA_OPR_WRT = ("tau", "w0", "g")

    def _ir_spectra_opr_names(self, who, nz, grads, levels, wrt):
        """What both forms of `ir_spectra_opr_vjp` check alike, with the prefix `who`: the names in `wrt` (-> in the ABI's
        order), `levels` (-> 1..nz+1 as the ABI takes them) and the keys of `grads` (-> the dict without its None entries);
        reads IR_SPECTRA_VJP_GRADS and IR_SPECTRA_OPR_WRT alone"""
        names = _names_among(who, "wrt", wrt, self.IR_SPECTRA_OPR_WRT)
        rows = _level_rows(who, nz, levels)
        _keys_among(who, "grads", grads, self.IR_SPECTRA_VJP_GRADS)
        given = {k: v for k, v in grads.items() if v is not None}
        if not given:
            raise ClimaException(who + '"grads" holds none of %s' % ", ".join(self.IR_SPECTRA_VJP_GRADS))
        return names, rows, given

    def _ir_spectra_opr_request(self, nz, nw_ir, T_surface, T, grads, levels, wrt):
        """The arrays of `ir_spectra_opr_vjp` as the ABI takes them -- (T_surface (1,), T (nz,), levels 1..nz+1, the four
        cotangents in the ABI's order (Fortran-ordered float64, None where absent), the names of `wrt` in the ABI's
        order) -- for a handle of nz layers and nw_ir IR bins; wrong shapes, unknown keys and names, levels outside
        -(nz+1)..nz and a request without any cotangent are refused by name (reads IR_SPECTRA_VJP_GRADS and
        IR_SPECTRA_OPR_WRT alone: no handle needed)."""
        who = "ir_spectra_opr_vjp: "
        Ts, T = _one_column(who, nz, T_surface, T)
        names, rows, given = Radtran._ir_spectra_opr_names(self, who, nz, grads, levels, wrt)
        nsel = len(rows)
        g = [np.asfortranarray(given[k], dtype=np.float64) if k in given else None for k in self.IR_SPECTRA_VJP_GRADS]
        for k, a in zip(self.IR_SPECTRA_VJP_GRADS, g):
            want = (nsel,) if k.endswith("_n") else (nw_ir, nsel)
            if a is not None and a.shape != want:
                raise ClimaException(who + '"%s" has the shape %s, not %s' % (k, a.shape, want))
        return Ts, T, rows, g, names

    def ir_spectra_opr_vjp(self, T_surface, T, grads, levels=(-1,), wrt=("tau", "w0", "g")):
        """The gradient of a loss on one column's IR spectra with respect to the stored optical properties
        (radtran_ir_spectra_opr_vjp): the column is `radiate(T_surface, T, ..., compute_solar=False, compute_opacity=False)`
        read at `wrk_ir.fup_a / fdn_a [levels[a], l]` and `fup_n / fdn_n [levels[a]]`; `grads` is a dict of cotangents keyed
        as `ir_spectra_vjp`'s -- "fup" / "fdn" (nw_ir, nsel), "fup_n" / "fdn_n" (nsel,), an absent one counting as 0.
        Returns a dict with the names in `wrt`: "tau" and "w0" (nz, ngauss, nw), "g" (nz, nw), Fortran-ordered, in `opr()`'s
        layout element by element (TOA-first, opacity-bin index, 0 outside the IR channel), the g-point's weight included;
        tau, w0 and g count as independent inputs.  One adjoint and one forward two-stream solve per (bin, g-point)
        however many levels; bitwise repeatable; the handle's state is left untouched.  `grey_sensitivity` turns the result
        into the response to an added grey absorber or scatterer."""
        nz, nw_ir = self.nz, len(self.ir.freq) - 1
        Ts, T, rows, g, names = self._ir_spectra_opr_request(nz, nw_ir, T_surface, T, grads, levels, wrt)
        shapes = dict(tau=(nz, self.ngauss, self.nw), w0=(nz, self.ngauss, self.nw), g=(nz, self.nw))
        out = {name: np.empty(shapes[name], order="F") for name in names}
        ptr = lambda a: _d(a) if a is not None else None   # noqa: E731
        self._L.radtran_ir_spectra_opr_vjp(self._ptr, _d(Ts), _i(nz), _d(T), _i(len(rows)), rows.ctypes.data_as(C.POINTER(C.c_int)),
                                           ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(out.get("tau")), ptr(out.get("w0")),
                                           ptr(out.get("g")), self._err)
        self._check()
        return out

    def ir_spectra_opr_vjp_tensors(self, T_surface, T, grads, levels=(-1,), wrt=("tau", "w0", "g"), sync=False):
        """`ir_spectra_opr_vjp` on torch CUDA float64 tensors (radtran_ir_spectra_opr_vjp_device): T_surface (1,), T (nz,),
        `grads` "fup" / "fdn" (nsel, nw_ir), "fup_n" / "fdn_n" (nsel,), C-contiguous -- the host form's arrays, transposed.
        Returns a dict of fresh tensors "tau" / "w0" (nw, ngauss, nz), "g" (nw, nz), bit for bit the host form's, transposed;
        stream ordering and `sync` as in `ir_spectra_batch_tensors`."""
        import torch
        who = "ir_spectra_opr_vjp_device"
        nz, nw_ir = self.nz, len(self.ir.freq) - 1
        names, rows, g = Radtran._ir_spectra_opr_names(self, who + ": ", nz, grads, levels, wrt)
        nsel = len(rows)
        self._ir_tensor_check(who, "T_surface", T_surface, (1,))
        self._ir_tensor_check(who, "T", T, (nz,))
        for k, t in g.items():
            self._ir_tensor_check(who, k, t, (nsel,) if k.endswith("_n") else (nsel, nw_ir))
        dev = T.device if T.is_cuda else torch.device("cuda", torch.cuda.current_device())
        shapes = dict(tau=(self.nw, self.ngauss, nz), w0=(self.nw, self.ngauss, nz), g=(self.nw, nz))
        out = {name: torch.empty(shapes[name], dtype=torch.float64, device=dev) for name in names}
        addr = lambda d, key: d[key].data_ptr() if key in d else None   # noqa: E731
        self._on_handle_stream(dev, lambda producer: self._L.radtran_ir_spectra_opr_vjp_device(
            self._ptr, T_surface.data_ptr(), _i(nz), T.data_ptr(), _i(nsel), rows.ctypes.data_as(C.POINTER(C.c_int)),
            addr(g, "fup"), addr(g, "fdn"), addr(g, "fup_n"), addr(g, "fdn_n"), addr(out, "tau"), addr(out, "w0"), addr(out, "g"),
            producer, self._err), sync)
        return out

    SOL_SPECTRA_OPR_GRADS = ("fup", "fdn", "amean", "fup_n", "fdn_n")
    SOL_SPECTRA_OPR_WRT = ("tau", "w0", "g", "albedo")

    def _sol_spectra_opr_names(self, who, nz, grads, levels, wrt):
        """What both forms of `sol_spectra_opr_vjp` check alike, with the prefix `who`: the names in `wrt` (-> in the ABI's
        order), `levels` (-> 1..nz+1 as the ABI takes them) and the keys of `grads` (-> the dict without its None entries);
        reads SOL_SPECTRA_OPR_GRADS and SOL_SPECTRA_OPR_WRT alone"""
        names = _names_among(who, "wrt", wrt, self.SOL_SPECTRA_OPR_WRT)
        rows = _level_rows(who, nz, levels)
        _keys_among(who, "grads", grads, self.SOL_SPECTRA_OPR_GRADS)
        given = {k: v for k, v in grads.items() if v is not None}
        if not given:
            raise ClimaException(who + '"grads" holds none of %s' % ", ".join(self.SOL_SPECTRA_OPR_GRADS))
        return names, rows, given

    def _sol_spectra_opr_request(self, nz, nw_sol, grads, levels, wrt):
        """The arrays of `sol_spectra_opr_vjp` as the ABI takes them -- (levels 1..nz+1, the five cotangents in the ABI's
        order (Fortran-ordered float64, None where absent), the names of `wrt` in the ABI's order) -- for a handle of nz
        layers and nw_sol solar bins; wrong shapes, unknown keys and names, levels outside -(nz+1)..nz and a request
        without any cotangent are refused by name (reads SOL_SPECTRA_OPR_GRADS and SOL_SPECTRA_OPR_WRT alone: no handle
        needed)."""
        who = "sol_spectra_opr_vjp: "
        names, rows, given = Radtran._sol_spectra_opr_names(self, who, nz, grads, levels, wrt)
        nsel = len(rows)
        g = [np.asfortranarray(given[k], dtype=np.float64) if k in given else None for k in self.SOL_SPECTRA_OPR_GRADS]
        for k, a in zip(self.SOL_SPECTRA_OPR_GRADS, g):
            want = (nsel,) if k.endswith("_n") else (nw_sol, nsel)
            if a is not None and a.shape != want:
                raise ClimaException(who + '"%s" has the shape %s, not %s' % (k, a.shape, want))
        return rows, g, names

    def sol_spectra_opr_vjp(self, grads, levels=(-1,), wrt=("tau", "w0", "g", "albedo")):
        """The gradient of a loss on the solar spectra with respect to the stored optical properties and the surface albedo
        (radtran_sol_spectra_opr_vjp): what is differentiated is `radiate(..., compute_solar=True, compute_opacity=False)`
        under the handle's zenith angles and weights, albedo, photon scale factor and diurnal factor, read at
        `wrk_sol.fup_a / fdn_a / amean [levels[a], l]` and `wrk_sol.fup_n / fdn_n [levels[a]]`, in the call's own units;
        `grads` is a dict of cotangents -- "fup" / "fdn" / "amean" (nw_sol, nsel), "fup_n" / "fdn_n" (nsel,), an absent one
        counting as 0.  Returns a dict with the names in `wrt`: "tau" and "w0" (nz, ngauss, nw), "g" (nz, nw),
        Fortran-ordered, in `opr()`'s layout element by element (TOA-first, opacity-bin index, 0 outside the solar
        channel), the g-point's weight included, and "albedo" (nw_sol,); tau, w0 and g count as independent inputs, the
        delta-Eddington scaling is differentiated.  One adjoint and one forward two-stream solve per (bin, g-point)
        however many levels and zenith angles; bitwise repeatable; the handle's state is left untouched.
        `grey_sensitivity` works on the result as on `ir_spectra_opr_vjp`'s."""
        nz, nw_sol = self.nz, len(self.sol.freq) - 1
        rows, g, names = self._sol_spectra_opr_request(nz, nw_sol, grads, levels, wrt)
        shapes = dict(tau=(nz, self.ngauss, self.nw), w0=(nz, self.ngauss, self.nw), g=(nz, self.nw), albedo=(nw_sol,))
        out = {name: np.empty(shapes[name], order="F") for name in names}
        ptr = lambda a: _d(a) if a is not None else None   # noqa: E731
        self._L.radtran_sol_spectra_opr_vjp(self._ptr, _i(len(rows)), rows.ctypes.data_as(C.POINTER(C.c_int)),
                                            ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]), ptr(out.get("tau")),
                                            ptr(out.get("w0")), ptr(out.get("g")), ptr(out.get("albedo")), self._err)
        self._check()
        return out

    def sol_spectra_opr_vjp_tensors(self, grads, levels=(-1,), wrt=("tau", "w0", "g", "albedo"), sync=False):
        """`sol_spectra_opr_vjp` on torch CUDA float64 tensors (radtran_sol_spectra_opr_vjp_device): `grads` "fup" / "fdn" /
        "amean" (nsel, nw_sol), "fup_n" / "fdn_n" (nsel,), C-contiguous -- the host form's arrays, transposed.  Returns a
        dict of fresh tensors "tau" / "w0" (nw, ngauss, nz), "g" (nw, nz), "albedo" (nw_sol,), bit for bit the host form's,
        transposed; stream ordering and `sync` as in `ir_spectra_batch_tensors`."""
        import torch
        who = "sol_spectra_opr_vjp_device"
        nz, nw_sol = self.nz, len(self.sol.freq) - 1
        names, rows, g = Radtran._sol_spectra_opr_names(self, who + ": ", nz, grads, levels, wrt)
        nsel = len(rows)
        for k, t in g.items():
            self._ir_tensor_check(who, k, t, (nsel,) if k.endswith("_n") else (nsel, nw_sol))
        first = next(iter(g.values()))
        dev = first.device if first.is_cuda else torch.device("cuda", torch.cuda.current_device())
        shapes = dict(tau=(self.nw, self.ngauss, nz), w0=(self.nw, self.ngauss, nz), g=(self.nw, nz), albedo=(nw_sol,))
        out = {name: torch.empty(shapes[name], dtype=torch.float64, device=dev) for name in names}
        addr = lambda d, key: d[key].data_ptr() if key in d else None   # noqa: E731
        self._on_handle_stream(dev, lambda producer: self._L.radtran_sol_spectra_opr_vjp_device(
            self._ptr, _i(nsel), rows.ctypes.data_as(C.POINTER(C.c_int)),
            addr(g, "fup"), addr(g, "fdn"), addr(g, "amean"), addr(g, "fup_n"), addr(g, "fdn_n"),
            addr(out, "tau"), addr(out, "w0"), addr(out, "g"), addr(out, "albedo"), producer, self._err), sync)
        return out

    def ir_spectra_torch(self, T_surface, T, levels=(-1,), parts=("up",), fluxes=False, weights=None):
        """`ir_spectra_batch_tensors` as a differentiable torch op: the same dict of tensors (without the weights), with
        gradients flowing to `T_surface` (ncol,) and `T` (ncol, nz) through `ir_spectra_vjp_tensors` -- the exact gradient
        of this library's forward model at fixed opacities, one kernel per backward pass, nothing on the host.
        `weights=None` computes the weights once per call (forward and backward share them); the dict an
        `ir_spectra_batch_tensors(..., return_weights=True)` call with the same `levels` returned is reused as it is,
        which leaves a Planck pass per forward and a dB/dT pass per backward.  No gradient flows to the weights."""
        import torch
        rad = self
        keys = []

        class _IrSpectra(torch.autograd.Function):
            @staticmethod
            def forward(ctx, Ts, Tc):
                out = rad.ir_spectra_batch_tensors(Ts, Tc, levels, parts, fluxes, weights=weights, return_weights=weights is None)
                ctx.weights = weights if weights is not None else {k: out.pop(k) for k in list(out) if k.startswith("w_")}
                keys[:] = [k for k in out if not k.startswith("w_")]
                ctx.save_for_backward(Ts, Tc)
                return tuple(out[k] for k in keys)

            @staticmethod
            def backward(ctx, *gout):
                Ts, Tc = ctx.saved_tensors
                g = {k: t.contiguous() for k, t in zip(keys, gout) if t is not None}
                if not g:
                    return None, None
                w = {k: ctx.weights[k] for k in ctx.weights if any(("up" in k) == ("up" in q) for q in g)}
                return rad.ir_spectra_vjp_tensors(Ts, Tc, w, g)

        res = _IrSpectra.apply(T_surface, T)
        return dict(zip(keys, res))

    # ---- HBM-resident form (bench / batched callers)
    def upload_column(self, T_surface, T, P, densities, dz, pdensities=None, radii=None):
        T, P, dz, densities = _c(T), _c(P), _c(dz), _fo(densities)
        if len(T) != self.nz or len(P) != self.nz or len(dz) != self.nz or densities.shape != (self.nz, self.ng):
            raise ClimaException('"densities" has the wrong input dimension.')
        pd = ra = None
        if pdensities is not None:
            pdensities, radii = _fo(pdensities), _fo(radii)
            pd, ra = _d(pdensities), _d(radii)
        self._L.radtran_upload_column(self._ptr, _f(T_surface), _d(T), _d(P), _d(densities), _d(dz), pd, ra, self._err)
        self._check()

    def radiate_resident(self, compute_solar=True, compute_opacity=True):
        self._L.radtran_radiate_resident(self._ptr, _i(compute_solar), _i(compute_opacity), self._err)
        self._check()

    def synchronize(self):
        self._L.radtran_synchronize(self._ptr, self._err)
        self._check()

    def set_bin_shard(self, rank, world):
        self._L.radtran_set_bin_shard(self._ptr, _i(rank), _i(world), self._err)
        self._check()

    # ---- the library's own multi-GPU step (include/clima_radtran_hip.h, radtran_comm_*): one process per GPU;
    # after comm_init_* every radiate / TOA_fluxes / radiate_resident of this handle works on the rank's bins and
    # ends with one RCCL all-reduce of the level fluxes on the handle's stream
    COMM_ID_BYTES = 128

    @staticmethod
    def set_device(device):
        L = _lib.load()
        err = C.create_string_buffer(_lib.ERR_LEN + 1)
        L.radtran_set_device(_i(device), err)
        if err.value:
            raise ClimaException(err.value.decode())

    @staticmethod
    def comm_unique_id():
        """rank 0: a fresh communicator id (bytes) to hand to every rank."""
        L = _lib.load()
        err = C.create_string_buffer(_lib.ERR_LEN + 1)
        buf = C.create_string_buffer(Radtran.COMM_ID_BYTES)
        L.radtran_comm_unique_id(buf, err)
        if err.value:
            raise ClimaException(err.value.decode())
        return buf.raw

    def comm_init_rank(self, nranks, rank, comm_id):
        assert len(comm_id) == self.COMM_ID_BYTES
        self._L.radtran_comm_init_rank(self._ptr, _i(nranks), _i(rank), C.create_string_buffer(bytes(comm_id), self.COMM_ID_BYTES), self._err)
        self._check()

    def comm_init_file(self, nranks, rank, path):
        self._L.radtran_comm_init_file(self._ptr, _i(nranks), _i(rank), os.fsencode(path), self._err)
        self._check()

    def comm(self):
        """(nranks, rank, all-reduces enqueued so far); nranks 0 without a communicator"""
        n, r, k = C.c_int(0), C.c_int(0), C.c_int(0)
        self._L.radtran_comm_get(self._ptr, C.byref(n), C.byref(r), C.byref(k))
        return n.value, r.value, k.value

    def comm_destroy(self):
        self._L.radtran_comm_destroy(self._ptr)

    def bin_shard(self):
        v = [C.c_int() for _ in range(6)]
        self._L.radtran_bin_shard_get(self._ptr, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def spectra_all(self, do_solar=True, out=None):
        """The seven per-bin arrays of the last call through radtran_spectra_get_all (one synchronise; the arrays of
        `out` -- a dict from an earlier call -- are page-locked by the library on first use).  Column-major like the
        reference's holders: fup_a, fdn_a (nz+1, nw), tau_band (nz, nw) per channel, amean for the solar one."""
        nl, ni, ns = self.nz + 1, len(self.ir.freq) - 1, len(self.sol.freq) - 1
        if out is None:
            out = {name: np.zeros((nl - name.endswith("tau_band"), ni if name.startswith("ir_") else ns), order="F")
                   for name in self.SPECTRA_ALL}
        self._L.radtran_spectra_get_all(self._ptr, C.byref(C.c_bool(bool(do_solar))), _i(nl), _i(ni), _i(ns),
                                        *[_d(out[name]) for name in self.SPECTRA_ALL], self._err)
        self._check()
        self._locked = getattr(self, "_locked", [])
        if not any(o is out for o in self._locked):
            self._locked.append(out)          # page-locked by the library: kept alive until spectra_release / the handle goes
        return out

    def spectra_release(self):
        """Un-page-lock what spectra_all locked (before those arrays are freed)."""
        self._L.radtran_spectra_release(self._ptr)
        self._locked = []

    @property
    def merged_integrations(self):
        """(merged, standalone): integrations kept back that went out in the next call's prep launch / on their own."""
        m, s = C.c_int(), C.c_int()
        self._L.radtran_merged_integrations_get(self._ptr, C.byref(m), C.byref(s))
        return m.value, s.value

    def flux_tensor(self):
        """The packed level fluxes [ir_up, ir_dn, sol_up, sol_dn][nz+1] as a torch CUDA tensor
        aliasing the library's buffer (the RCCL all-reduce payload of a bin-sharded run)."""
        import torch
        ptr, n = self.flux_device_ptr()

        class _Alias:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        return torch.as_tensor(_Alias(), device="cuda")

    def finish_reduced(self):
        self._L.radtran_finish_reduced(self._ptr, self._err)
        self._check()

    def flux_device_ptr(self):
        p, n = C.c_void_p(), C.c_int()
        self._L.radtran_flux_device_ptr(self._ptr, C.byref(p), C.byref(n))
        return p.value, n.value

    def stream(self):
        p = C.c_void_p()
        self._L.radtran_stream_get(self._ptr, C.byref(p))
        return p.value

    def profile(self, enable=True):
        """HIP events on the library stream: True/1 around every kernel, 2 around the dominant
        kernel (k_opacity) only (two event records per call instead of eight), False/0 off."""
        self._L.radtran_profile_set(self._ptr, _i(2 if enable == 2 and enable is not True else (1 if enable else 0)))

    def profile_stride(self, stride):
        """Events on every `stride`-th call only."""
        self._L.radtran_profile_stride_set(self._ptr, _i(int(stride)))

    def profile_reset(self):
        self._L.radtran_profile_reset(self._ptr)

    def kernel_time(self, kernel_id):
        ms, n = C.c_double(), C.c_int()
        self._L.radtran_kernel_time_get(self._ptr, _i(kernel_id), C.byref(ms), C.byref(n), self._err)
        self._check()
        return ms.value, n.value

    def algorithmic_bytes(self):
        a, b, c, d = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._L.radtran_algorithmic_bytes(self._ptr, C.byref(a), C.byref(b), C.byref(c), C.byref(d), self._err)
        self._check()
        return dict(tables_distinct=a.value, input=b.value, output=c.value, tables_full=d.value)

    def algorithmic_nodes(self):
        """distinct interpolation nodes the uploaded column touches (N_PT, N_T) and the table sizes."""
        v = [C.c_double() for _ in range(4)]
        self._L.radtran_algorithmic_nodes(self._ptr, *[C.byref(x) for x in v], self._err)
        self._check()
        return dict(N_PT=v[0].value, N_PT_full=v[1].value, N_T=v[2].value, N_T_full=v[3].value)

    def opr(self):
        """OpticalPropertiesResult: tau,w0 (nz,ngauss,nw), g,tau_band (nz,nw); TOA-first."""
        nz, ng, nw = self.nz, self.ngauss, self.nw
        tau = np.empty((nz, ng, nw), order="F")
        w0 = np.empty((nz, ng, nw), order="F")
        g = np.empty((nz, nw), order="F")
        tb = np.empty((nz, nw), order="F")
        self._L.radtran_opr_get(self._ptr, _d(tau), _d(w0), _d(g), _d(tb), self._err)
        self._check()
        return tau, w0, g, tb

    # ------------------------------------------------------------------ Radtran.pyx surface
    def set_bolometric_flux(self, flux):
        self._L.radtran_set_bolometric_flux_wrapper(self._ptr, _f(flux))

    def bolometric_flux(self):
        v = C.c_double()
        self._L.radtran_bolometric_flux_wrapper(self._ptr, C.byref(v))
        return v.value

    def skin_temperature(self, bond_albedo):
        v = C.c_double()
        self._L.radtran_skin_temperature_wrapper(self._ptr, _f(bond_albedo), C.byref(v))
        return v.value

    def equilibrium_temperature(self, bond_albedo):
        v = C.c_double()
        self._L.radtran_equilibrium_temperature_wrapper(self._ptr, _f(bond_albedo), C.byref(v))
        return v.value

    def _vec_get(self, name, size_name=None):
        n = C.c_int()
        getattr(self._L, "radtran_%s_get_size" % (size_name or name))(self._ptr, C.byref(n))
        arr = np.empty(n.value, np.double)
        getattr(self._L, "radtran_%s_get" % name)(self._ptr, C.byref(n), _d(arr))
        return arr

    def _vec_set(self, name, arr, size_name=None):
        arr = _c(arr)
        n = C.c_int()
        getattr(self._L, "radtran_%s_get_size" % (size_name or name))(self._ptr, C.byref(n))
        if arr.ndim != 1 or arr.shape[0] != n.value:
            raise ClimaException('"%s" is the wrong size' % name)
        getattr(self._L, "radtran_%s_set" % name)(self._ptr, C.byref(n), _d(arr))

    zenith_u = property(lambda s: s._vec_get("zenith_u"), lambda s, a: s._vec_set("zenith_u", a),
                        doc="cosine of the zenith angles")
    zenith_weights = property(lambda s: s._vec_get("zenith_weights", "zenith_u"),
                              lambda s, a: s._vec_set("zenith_weights", a, "zenith_u"))
    surface_albedo = property(lambda s: s._vec_get("surface_albedo"), lambda s, a: s._vec_set("surface_albedo", a),
                              doc="surface albedo in each solar bin")
    surface_emissivity = property(lambda s: s._vec_get("surface_emissivity"),
                                  lambda s, a: s._vec_set("surface_emissivity", a),
                                  doc="surface emissivity in each IR bin")
    photons_sol = property(lambda s: s._vec_get("photons_sol"))
    f_total = property(lambda s: s._vec_get("f_total"))

    def _scalar(name, ctype, to, doc=None, settable=True, getter=None, outs=1, pick=0):
        """radtran_<name>_get / _set as a property of Python type `to`; getter: another _get, with `outs` outputs of which
        this is number `pick`"""
        def get(self):
            v = [ctype() for _ in range(outs)]
            getattr(self._L, "radtran_%s_get" % (getter or name))(self._ptr, *[C.byref(x) for x in v])
            return to(v[pick].value)

        def set_(self, val):
            getattr(self._L, "radtran_%s_set" % name)(self._ptr, C.byref(ctype(to(val))))

        return property(get, set_ if settable else None, doc=doc)

    has_hard_surface = _scalar("has_hard_surface", C.c_bool, bool)  # logical(c_bool), clima/cython/Radtran_pxd.pxd:45-46
    photon_scale_factor = _scalar("photon_scale_factor", C.c_double, float)
    ir_tau_min = _scalar("ir_tau_min", C.c_double, float)
    diurnal_fac = _scalar("diurnal_fac", C.c_double, float)
    fused = _scalar("fused", C.c_int, bool,
                    "True: opacity + two-stream of a compute_opacity call run as one grid (k_fused).")
    coop_items = _scalar("coop_items", C.c_int, int, "ng = 8: calls with at most this many (bin, source layer) items use "
                         "the group-of-lanes opacity kernel.")
    fused_spins = _scalar("fused_spins", C.c_int, int, "Polls a two-stream block of the fused grid spends waiting for its "
                          "opacity tiles (0: every wait expires and the call is repeated through separate launches).")
    fused_fallbacks = _scalar("fused_fallbacks", C.c_int, int, "Calls re-issued through the separate launches after a fused "
                              "hand-off wait expired.", settable=False)
    ir_green = _scalar("ir_green", C.c_int, int, "radiate_ir_batch's response form: 0 never, 1 (default) when enough columns "
                       "are sparse deviations of one profile, 2 whenever any is.", outs=2)
    ir_green_batches = _scalar("ir_green_batches", C.c_int, int, "Batches that took the response form.", settable=False,
                               getter="ir_green", outs=2, pick=1)
    defer_integration = _scalar("defer_integration", C.c_int, bool, "True (default): a `radiate_resident` call keeps its "
                                "frequency integration back for the next call's prep launch (one grid for both); anything "
                                "that reads results launches it first.  Same results bit for bit.")
    calls_in_flight = _scalar("calls_in_flight", C.c_int, int, "Pipelined `radiate_resident` calls in flight: 0 (default) two "
                              "where a call's grid does not fit the device in one residency round, 1 one at a time, 2 two "
                              "whenever eligible.  Consecutive calls alternate between two sets of work buffers and two "
                              "streams; everything else joins first.  Same results bit for bit.")
    overlapped_calls = _scalar("overlapped_calls", C.c_int, int, "Calls enqueued on one call slot while the other slot's "
                               "call had not been joined.", settable=False)
    del _scalar

    def _sub(self, name, cls):
        p = C.c_void_p()
        getattr(self._L, "radtran_%s_get" % name)(self._ptr, C.byref(p))
        obj = cls(self._L, p)
        obj._parent = self  # keep the handle alive while the borrowed pointer is in use
        return obj

    ir = property(lambda s: s._sub("ir", RTChannel), doc="RTChannel of the IR bins")
    sol = property(lambda s: s._sub("sol", RTChannel), doc="RTChannel of the solar bins")
    wrk_ir = property(lambda s: s._sub("wrk_ir", ClimaRadtranWrk), doc="IR results")
    wrk_sol = property(lambda s: s._sub("wrk_sol", ClimaRadtranWrk), doc="solar results")
