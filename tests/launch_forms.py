"""The launch-form table: one row per configuration of a handle, with the plan plan_radiate (clima_amd/csrc/kernels.hip)
is expected to make for each kind of call on it.  A helper, not a test: tests/test_launch_form_table.py holds the rows to
the library's own planner (clima_test_plan_radiate) and shows that together they name every kernel instance the planner
can choose; tests/test_gpu_entry_points.py runs every entry point on every row.

A row's plans are the hook's outputs for four kinds of call:
  single0   a radiate / TOA_fluxes call with coop_items = 0
  single    the same call at the handle's default coop_items
  batch     a chunk of a column batch (its fused form, where the integration fits one launch, is what makes the batch
            take one launch per chunk; otherwise the columns' calls run back to back, each a `single` call whose column
            is not known to be all pairs)
  ir_only   radiate(compute_solar=False, compute_opacity=False) on the stored opacities
Where the hook disagrees with a row the hook is right: the row is corrected, and a row is added or moved so that the form
it was written for stays covered."""
import collections
import ctypes as C
import os

import numpy as np

# ---- the hook's vocabulary (include/clima_radtran_hip.h, clima_test_plan_radiate)
IN_FIELDS = ("nz", "ng", "nzen", "n_ir", "n_sol", "op_n", "nsrc", "ncol", "batch", "ir_batch", "rebin_mode", "cust_on",
             "compute_opacity", "all_pairs", "fused", "allow_fused", "ts_block_mode", "no_half", "coop_items", "force_slots",
             "nbins")
TS_FIELDS = ("form", "slots", "groups", "per_launch", "zero_launch")
OUT_FIELDS = (("opacity", "coop_ng") + tuple("%s_%s" % (p, f) for p in ("fused", "ts", "block") for f in TS_FIELDS) +
              ("prep_clears", "caller_clears", "write_w0", "integrate_one_launch"))
NONE, WAVE, HALF, PAIRED, BLOCK = range(5)      # TS_*: forms of the two-stream kernels
STORED, TILE, COOP, UNSUPPORTED = range(4)      # OP_*: stored opacities | lane per item | group of lanes
FORM_NAMES = ("none", "wave", "half", "paired", "block")
OPACITY_NAMES = ("stored", "tile", "coop", "unsupported")

DEFAULT_COOP_ITEMS = 34816     # a handle's coop_items as made
BATCH_COLS = 2                 # CLIMA_HIP_BATCH_COLS of every row: 5 columns run as chunks of 2, 2 and 1
MAX_ZEN = 16
KINDS = ("single0", "single", "batch", "ir_only")
UNEVEN_WEIGHTS = np.array([0.30, 0.28, 0.20, 0.12, 0.06, 0.025, 0.011, 0.004])   # test_uneven_g_weights_multi_edge_rebin's

# (form, slots, groups, per_launch, zero_launch) of the fused grid, the stand-alone wave forms, the workgroup-per-bin form
Plan = collections.namedtuple("Plan", "opacity coop_ng fused ts block prep_clears caller_clears write_w0")
NO = (NONE, 0, 0, 0, 0)


def plan_of(out):
    """the hook's outputs (dict) as a Plan"""
    return Plan(out["opacity"], out["coop_ng"], *[tuple(out["%s_%s" % (p, f)] for f in TS_FIELDS) for p in ("fused", "ts", "block")],
                out["prep_clears"], out["caller_clears"], out["write_w0"])


def hook_plan(L, **fields):
    """clima_test_plan_radiate: every input by name -> dict of every output by name"""
    assert sorted(fields) == sorted(IN_FIELDS), sorted(set(fields) ^ set(IN_FIELDS))
    a = (C.c_int * len(IN_FIELDS))(*[int(fields[k]) for k in IN_FIELDS])
    out = (C.c_int * len(OUT_FIELDS))(*([-1] * len(OUT_FIELDS)))
    L.clima_test_plan_radiate(a, out)
    return dict(zip(OUT_FIELDS, out))


def hook_rebin_mode(L, weights, stream):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    mode = C.c_int(-1)
    L.clima_test_rebin_mode_for(C.byref(C.c_int(len(w))), w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(C.c_int(int(stream))),
                                C.byref(mode))
    return mode.value


def instance(out, rebin_mode, cust_on):
    """The kernel instances a plan names, each launch on its own (the opacity launch and a stand-alone two-stream launch are
    two kernels: their combinations are not a third).  A fused plan: the grid's form and slots, with its rebin mode and
    CUSTOM where slots <= 4 (the 5-8 slot, half-wave and paired kernels exist for the default form only).  Otherwise
    the opacity kernel, its width and whether it stores w0, and the stand-alone form that runs with its slots (the
    workgroup-per-bin form where no wave form applies).  Either way, who clears for the form that runs: the prep
    launch, the caller, a launch of its own.  `out`: the hook's outputs, in order or by name."""
    o = dict(zip(OUT_FIELDS, out)) if not isinstance(out, dict) else out
    clears = "prep%d caller%d" % (o["prep_clears"], o["caller_clears"])
    if o["fused_form"] != NONE:
        # one kernel: the opacity tiles (always lane per item, w0 left to the two-stream part) and the two-stream blocks
        assert o["opacity"] == TILE and not o["write_w0"] and not o["fused_zero_launch"]
        form = FORM_NAMES[o["fused_form"]]
        rm = ("RM%d" % rebin_mode, "CUSTOM%d" % int(cust_on)) if o["fused_slots"] <= 4 else ()
        return (("fused", form, o["fused_slots"]) + rm, ("clears", "fused " + form, clears, "zero0"))
    op = ("opacity", OPACITY_NAMES[o["opacity"]], o["coop_ng"] if o["opacity"] == COOP else 0, "w0=%d" % o["write_w0"])
    if o["ts_form"] != NONE:
        form, slots, zero = FORM_NAMES[o["ts_form"]], o["ts_slots"], o["ts_zero_launch"]
    elif o["block_form"] != NONE:
        form, slots, zero = "block", 0, o["block_zero_launch"]
    else:
        form, slots, zero = "none", 0, 0
    return (op, ("two-stream", form, slots), ("clears", form, clears, "zero%d" % zero))


class Row:
    """One configuration.  tables: keywords of synthetic.make_tables; nz: layers (of the doubled grid where `doubled`);
    env: the environment around the handle's construction; the rest are the handle's and the column's settings."""

    def __init__(self, name, nz, plans, tables=None, doubled=False, nzen=2, custom=False, env=None, rebin_mode=0,
                 hard=True, per_bin_surface=False, diurnal_fac=None, photon_scale_factor=None, zero_species=None,
                 radii_scale=None):
        self.name, self.nz, self.doubled, self.nzen, self.custom = name, nz, doubled, nzen, custom
        self.tables_kw = dict(nw=8, seed=900 + nz)
        self.tables_kw.update(tables or {})
        self.env = dict(CLIMA_HIP_BATCH_COLS=str(BATCH_COLS))
        self.env.update(env or {})
        self.rebin_mode, self.hard, self.per_bin_surface = rebin_mode, hard, per_bin_surface
        self.diurnal_fac, self.photon_scale_factor = diurnal_fac, photon_scale_factor
        self.zero_species, self.radii_scale = zero_species, radii_scale
        self.plans = dict(zip(KINDS, plans))
        assert not doubled or nz % 2 == 0

    def __repr__(self):
        return self.name

    # ---- what the planner is told of a call on this row's handle (plan_input, clima_amd/csrc/radtran_api.hip)
    @property
    def ng(self):
        w = self.tables_kw.get("weights")
        return len(w) if w is not None else self.tables_kw.get("ng", 8)

    @property
    def weights(self):
        from clima_amd import synthetic as S
        w = self.tables_kw.get("weights")
        return np.asarray(w, dtype=float) if w is not None else S.gauss_weights01(self.ng)

    def bins(self):
        """(n_ir, n_sol, nw) as synthetic.make_tables cuts the channels"""
        nw = self.tables_kw["nw"]
        return nw - int(round(0.4 * nw)), int(round(0.6 * nw)), nw

    def plan_in(self, kind):
        n_ir, n_sol, nw = self.bins()
        stored = kind == "ir_only"
        batch = kind == "batch"
        return dict(nz=self.nz, ng=self.ng, nzen=self.nzen, n_ir=n_ir, n_sol=0 if stored else n_sol, op_n=nw,
                    nsrc=self.nz // 2 if self.doubled and not batch else self.nz, ncol=BATCH_COLS if batch else 1, batch=batch,
                    ir_batch=0, rebin_mode=self.rebin_mode, cust_on=self.custom, compute_opacity=not stored,
                    all_pairs=self.doubled and not batch and not stored, fused=1, allow_fused=1, ts_block_mode=0,
                    no_half=0, coop_items=DEFAULT_COOP_ITEMS if kind == "single" else 0, force_slots=0, nbins=max(n_ir, n_sol))

    @property
    def one_launch(self):
        """the batch takes one launch per chunk (batch_form: the chunk's plan is fused; the integration fits one launch
        at every row's bin count)"""
        return self.plans["batch"].fused[0] != NONE

    # ---- the handle and the columns
    def tables(self):
        from clima_amd import synthetic as S
        return S.make_tables(**self.tables_kw)

    def scalars(self):
        s = {}
        if not self.hard:
            s["has_hard_surface"] = False
        if self.diurnal_fac is not None:
            s["diurnal_fac"] = self.diurnal_fac
        if self.photon_scale_factor is not None:
            s["photon_scale_factor"] = self.photon_scale_factor
        return s

    def surface(self):
        """(albedo per solar bin, emissivity per IR bin) or None"""
        if not self.per_bin_surface:
            return None
        n_ir, n_sol, _ = self.bins()
        return np.linspace(0.05, 0.85, n_sol), np.linspace(0.6, 1.0, n_ir)

    def _finish(self, col):
        from clima_amd import synthetic as S
        col = S.Column({k: (np.array(v, copy=True, order="K") if isinstance(v, np.ndarray) else v) for k, v in col.items()})
        if self.zero_species is not None:
            col["densities"][:, self.zero_species] = 0.0
        if self.radii_scale is not None:
            col["radii"] = np.asfortranarray(col["radii"] * self.radii_scale)
            col["pdensities"] = np.asfortranarray(col["pdensities"] * 50.0)
        return col

    def column(self):
        """the column of the single calls"""
        from clima_amd import synthetic as S
        if self.doubled:
            from test_gpu_batch_device import doubled
            return self._finish(doubled(self.nz // 2 - 1)[0])
        return self._finish(S.modern_earth_column(self.nz))

    def columns(self, n, seed=23):
        """n different columns (the pipeline's A and B, a batch's columns)"""
        from clima_amd import synthetic as S
        if self.doubled:
            from test_gpu_batch_device import doubled
            return [self._finish(c) for c in doubled(self.nz // 2 - 1, max(n, 2), seed=seed)[:n]]
        return [self._finish(c) for c in S.perturbed_columns(n, self.nz, seed=seed)]

    def environment(self):
        """context manager: the row's switches in os.environ (they are read when a handle is made)"""
        return _Environment(self.env)

    def make(self, cls, *more, **kw):
        """cls(tables, nz, nzen, albedo) under the row's environment; the caller sets scalars, surface and custom properties"""
        with self.environment():
            return cls(self.tables_cached(), self.nz, self.nzen, 0.25, *more, **kw)

    def tables_cached(self):
        if getattr(self, "_tables", None) is None:
            self._tables = self.tables()
        return self._tables


class _Environment:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the rows.  Abbreviations of the (form, slots, groups, per_launch, zero_launch) blocks the plans below are made of:
def W(slots, zero=0):     # whole wave, 8 g-points: two groups of 4 columns in one launch, ADDED into cleared outputs
    return (WAVE, slots, 2, 2, zero)


def H(slots):             # half wave, 8 g-points: one group, whole values stored
    return (HALF, slots, 1, 1, 0)


B1, B2, B4, B8 = ((BLOCK, s, 1, 1, 0) for s in (1, 2, 4, 8))     # workgroup per bin, all 8 g-points in one block
B16 = (BLOCK, 16, 2, 2, 1)                                       # ... two groups of 4, a clearing launch of its own
STREAM = {"CLIMA_HIP_REBIN": "stream"}
UNEVEN = UNEVEN_WEIGHTS / UNEVEN_WEIGHTS.sum()


def _separate(slots, block):
    """8 g-points, not fused: the prep launch clears for the whole-wave kernel's two groups; on stored opacities nobody
    has cleared, so the kernel's own clearing launch does"""
    return [Plan(TILE, 8, NO, W(slots), block, 1, 0, 1), Plan(COOP, 8, NO, W(slots), block, 1, 0, 1),
            Plan(TILE, 8, NO, W(slots), block, 1, 0, 1), Plan(STORED, 0, NO, W(slots, 1), block, 0, 0, 1)]


def _fused_half(hs, slots, block):
    """the fused half-wave grid stores whole values: nothing is cleared, w0 is left to the grid; a call small enough for
    the group-of-lanes kernel is not fused; the IR-only call takes the stand-alone half-wave kernel"""
    fused = Plan(TILE, 8, H(hs), W(slots, 1), block, 0, 0, 0)
    return [fused, Plan(COOP, 8, NO, W(slots), block, 1, 0, 1), fused, Plan(STORED, 0, NO, H(hs), block, 0, 0, 1)]


def _fused_wave(slots, stored_ts, block, single0=None):
    """the fused whole-wave grid adds two groups: the prep launch clears.  single0: the fused form of the single call
    where it is not the chunk's (exact pairs); stored_ts: the stand-alone form of the IR-only call"""
    return [Plan(TILE, 8, single0 or W(slots), W(slots), block, 1, 0, 0), Plan(COOP, 8, NO, W(slots), block, 1, 0, 1),
            Plan(TILE, 8, W(slots), W(slots), block, 1, 0, 0), Plan(STORED, 0, NO, stored_ts, block, 0, 0, 1)]


def _block_only(block, prep):
    """no wave form applies (more than 512 layers: nothing to clear in the prep launch; more than MAX_ZEN zenith angles)"""
    return [Plan(TILE, 8, NO, NO, block, prep, 0, 1), Plan(COOP, 8, NO, NO, block, prep, 0, 1),
            Plan(TILE, 8, NO, NO, block, prep, 0, 1), Plan(STORED, 0, NO, NO, block, 0, 0, 1)]


def _other_ng(lanes, ts, block):
    """ng != 8: the group-of-lanes kernel whatever coop_items says, never fused; more than one group: cleared by the prep
    launch, or by the kernel's own clearing launch on stored opacities"""
    many = int(ts[2] > 1)
    first = Plan(COOP, lanes, NO, ts, block, many, 0, 1)
    return [first, first, first, Plan(STORED, 0, NO, ts[:4] + (many,), block, 0, 0, 1)]


SCALED = dict(diurnal_fac=0.37, photon_scale_factor=0.4286)
ROWS = [
    # -- not fused: at most 64 layers
    Row("nz1", 1, _separate(1, B1), nzen=1),
    Row("nz2", 2, _separate(1, B2), nzen=1, hard=False),
    Row("s64", 64, _separate(1, B8), per_bin_surface=True),
    # -- the fused half-wave grid, 3 to 7 slots
    Row("h65", 65, _fused_half(3, 2, B8), nzen=3, per_bin_surface=True),
    Row("h100", 100, _fused_half(4, 2, B8)),
    Row("h130", 130, _fused_half(5, 3, B16)),
    Row("h170", 170, _fused_half(6, 3, B16)),
    Row("h224", 224, _fused_half(7, 4, B16), **SCALED),
    # -- the fused whole-wave grid, 4 to 8 slots
    Row("w225", 225, _fused_wave(4, W(4, 1), B16), zero_species=1),
    Row("w257", 257, _fused_wave(5, W(5, 1), B16), hard=False),
    Row("w350", 350, _fused_wave(6, W(6, 1), B16)),
    Row("w512", 512, _fused_wave(8, W(8, 1), B16), radii_scale=2.5),
    Row("b513", 513, _block_only(B16, 0), **SCALED),
    # -- all layers in exact pairs: the paired form for the single call, the whole-wave form for a chunk
    Row("p230", 230, _fused_wave(4, W(4, 1), B16, single0=(PAIRED, 4, 2, 2, 0)), doubled=True),
    Row("p258", 258, _fused_wave(5, W(5, 1), B16, single0=(PAIRED, 6, 2, 2, 0)), doubled=True),
    Row("p402", 402, _fused_wave(7, W(7, 1), B16, single0=(PAIRED, 8, 2, 2, 0)), doubled=True),
    # -- custom optical properties (k_fused<0, true, 0> at 2, 3, 4 slots; none beyond)
    Row("c65", 65, _fused_wave(2, H(3), B8), custom=True),
    Row("c130", 130, _fused_wave(3, H(5), B16), custom=True),
    Row("c256", 256, _fused_wave(4, W(4, 1), B16), custom=True),
    Row("c257", 257, _separate(5, B16), custom=True),
    # -- rebin modes 1 (streaming) and 2 (multi-edge), without and with custom properties, at 2, 3, 4 slots
    Row("r1-70", 70, _fused_wave(2, H(3), B8), env=STREAM, rebin_mode=1),
    Row("r1-130", 130, _fused_wave(3, H(5), B16), env=STREAM, rebin_mode=1),
    Row("r1-200", 200, _fused_wave(4, H(7), B16), env=STREAM, rebin_mode=1),
    Row("r1c-70", 70, _fused_wave(2, H(3), B8), env=STREAM, rebin_mode=1, custom=True),
    Row("r1c-150", 150, _fused_wave(3, H(5), B16), env=STREAM, rebin_mode=1, custom=True),
    Row("r1c-200", 200, _fused_wave(4, H(7), B16), env=STREAM, rebin_mode=1, custom=True),
    Row("r2-100", 100, _fused_wave(2, H(4), B8), tables=dict(weights=UNEVEN), rebin_mode=2),
    Row("r2-150", 150, _fused_wave(3, H(5), B16), tables=dict(weights=UNEVEN), rebin_mode=2),
    Row("r2-200", 200, _fused_wave(4, H(7), B16), tables=dict(weights=UNEVEN), rebin_mode=2),
    Row("r2c-70", 70, _fused_wave(2, H(3), B8), tables=dict(weights=UNEVEN), rebin_mode=2, custom=True),
    Row("r2c-130", 130, _fused_wave(3, H(5), B16), tables=dict(weights=UNEVEN), rebin_mode=2, custom=True),
    Row("r2c-200", 200, _fused_wave(4, H(7), B16), tables=dict(weights=UNEVEN), rebin_mode=2, custom=True),
    Row("r2-300", 300, _separate(5, B16), tables=dict(weights=UNEVEN), rebin_mode=2, radii_scale=2.5),
    # -- other g-point counts: the group-of-lanes kernel at 8, 16, 32 lanes
    Row("g4-70", 70, _other_ng(8, (WAVE, 2, 1, 1, 0), (BLOCK, 16, 1, 1, 0)), tables=dict(ng=4), rebin_mode=1, zero_species=1),
    Row("g16-100", 100, _other_ng(16, (HALF, 4, 2, 2, 0), (BLOCK, 8, 2, 2, 1)), tables=dict(ng=16), rebin_mode=1),
    Row("g16-300", 300, _other_ng(16, (WAVE, 5, 4, 1, 0), (BLOCK, 8, 2, 2, 1)), tables=dict(ng=16), rebin_mode=1),
    Row("g32-40", 40, _other_ng(32, (WAVE, 1, 8, 1, 0), (BLOCK, 4, 2, 2, 1)), tables=dict(ng=32, sorted_k=False), rebin_mode=1),
    # -- more than MAX_ZEN zenith angles: the workgroup-per-bin form, one group and two
    Row("z17-100", 100, _block_only(B8, 1), nzen=17),
    Row("z17-130", 130, _block_only(B16, 1), nzen=17),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
