"""The launch-form table (tests/launch_forms.py) against the library's own planner, without a device.

1. Every row states the plan plan_radiate makes for its four kinds of call, and the rebin mode its weights get.
2. Together the rows name every kernel instance the planner can choose over
       nz 1..600, ng in {1, 4, 8, 16, 32}, nzen in {1, 16, 17}, rebin_mode in {0, 1, 2},
       cust_on, all_pairs, batch, compute_opacity, fused, no_half in {0, 1}, coop_items in {0, default},
       and, on stored opacities, with and without the solar channel,
   the other inputs as a handle of the rows' size has them.  What an instance is: launch_forms.instance.  The opacity
   launch and a stand-alone two-stream launch are counted each on its own: they are separate kernels, and the product of
   the group-of-lanes widths with the eight slot counts is not a set of kernels anybody compiled.  The fused grid IS one
   kernel, so there form, slots, rebin mode and CUSTOM are counted together.
3. The only instances no row names are the ones in EXCEPTIONS: those no handle reaches without a process-wide switch.
   The test fails when that list holds something the enumeration does not produce, and when anything outside it is
   uncovered; the list is a condition, not something to grow.

A planner change that moves a row out of the form it was written for fails 1; one that opens a form no row reaches
fails 2."""
import ctypes as C
import itertools

import pytest

import launch_forms as LF

# CLIMA_HIP_NO_HALF=1 is read once per process: with the half-wave kernels ruled out, the layer counts they take (65-224)
# go to the whole-wave fused grid at 2 to 4 slots in the default form (4 slots is reached without the switch, at 225-256
# layers), and all-pairs columns of at most 128 layers to the paired form at 2 slots.
EXCEPTIONS = {
    ("fused", "paired", 2, "RM0", "CUSTOM0"): "all pairs, at most 128 layers: the half-wave grid takes them unless CLIMA_HIP_NO_HALF=1",
    ("fused", "wave", 2, "RM0", "CUSTOM0"): "65-128 layers, default form: the half-wave grid takes them unless CLIMA_HIP_NO_HALF=1",
    ("fused", "wave", 3, "RM0", "CUSTOM0"): "129-192 layers, default form: the half-wave grid takes them unless CLIMA_HIP_NO_HALF=1",
}


@pytest.mark.parametrize("row", LF.ROWS, ids=repr)
def test_row_states_the_planners_plan(hip_lib, row):
    assert 6 <= row.tables_kw["nw"] <= 10
    stream = row.env.get("CLIMA_HIP_REBIN") == "stream"
    assert LF.hook_rebin_mode(hip_lib, row.weights, stream) == row.rebin_mode
    for kind in LF.KINDS:
        out = LF.hook_plan(hip_lib, **row.plan_in(kind))
        assert LF.plan_of(out) == row.plans[kind], (row.name, kind)
        assert out["integrate_one_launch"] == 1          # (so a fused chunk plan is all batch_form asks for)


def test_rebin_mode_hook(hip_lib):
    from clima_amd import synthetic as S
    assert LF.hook_rebin_mode(hip_lib, S.gauss_weights01(8), False) == 0     # the window form: 8 Gauss weights only
    assert LF.hook_rebin_mode(hip_lib, S.gauss_weights01(8), True) == 1
    assert LF.hook_rebin_mode(hip_lib, LF.UNEVEN, False) == 2
    assert LF.hook_rebin_mode(hip_lib, LF.UNEVEN, True) == 2
    for ng in (1, 4, 16, 32):
        assert LF.hook_rebin_mode(hip_lib, S.gauss_weights01(ng), False) == 1


def named_instances(L, rows):
    named = {}
    for row in rows:
        for kind in LF.KINDS:
            for inst in LF.instance(LF.hook_plan(L, **row.plan_in(kind)), row.rebin_mode, row.custom):
                named.setdefault(inst, []).append((row.name, kind))
    return named


@pytest.fixture(scope="module")
def enumerated(hip_lib):
    """instance -> the first inputs that produced it"""
    n_in, n_out = len(LF.IN_FIELDS), len(LF.OUT_FIELDS)
    a, out = (C.c_int * n_in)(), (C.c_int * n_out)()
    at = {k: i for i, k in enumerate(LF.IN_FIELDS)}
    n_ir, n_sol, nw = LF.ROWS[0].bins()
    for k, v in dict(n_ir=n_ir, op_n=nw, ir_batch=0, allow_fused=1, ts_block_mode=0, force_slots=0, nbins=max(n_ir, n_sol)).items():
        a[at[k]] = v
    plan, seen, done = hip_lib.clima_test_plan_radiate, {}, set()
    # call: 1 computes the opacities, 0 runs on the stored ones, 2 the same without the solar channel
    for no_half, ng, nzen, rm, cust, pairs, batch, call, fused, coop in itertools.product(
            (0, 1), (1, 4, 8, 16, 32), (1, LF.MAX_ZEN, LF.MAX_ZEN + 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (1, 0, 2), (0, 1),
            (0, LF.DEFAULT_COOP_ITEMS)):
        fixed = dict(no_half=no_half, ng=ng, nzen=nzen, rebin_mode=rm, cust_on=cust, all_pairs=pairs, batch=batch,
                     ncol=LF.BATCH_COLS if batch else 1, compute_opacity=int(call == 1), n_sol=0 if call == 2 else n_sol,
                     fused=fused, coop_items=coop)
        for k, v in fixed.items():
            a[at[k]] = v
        for nz in range(1, 601):
            a[at["nz"]] = a[at["nsrc"]] = nz
            plan(a, out)
            key = (bytes(out), rm, cust)
            if key in done:
                continue
            done.add(key)
            for inst in LF.instance(tuple(out), rm, cust):
                seen.setdefault(inst, dict(fixed, nz=nz))
    return seen


def test_rows_name_every_instance_the_planner_can_choose(hip_lib, enumerated):
    named = named_instances(hip_lib, LF.ROWS)
    assert len(enumerated) > 50
    stale = [e for e in EXCEPTIONS if e not in enumerated]
    assert not stale, "EXCEPTIONS lists instances the planner never produces: %s" % stale
    listed_but_named = [e for e in EXCEPTIONS if e in named]
    assert not listed_but_named, "EXCEPTIONS lists instances a row reaches: %s" % listed_but_named
    uncovered = {i: how for i, how in enumerated.items() if i not in named and i not in EXCEPTIONS}
    assert not uncovered, "no row names:\n" + "\n".join("  %s  first at %s" % kv for kv in sorted(uncovered.items(), key=str))


def test_exceptions_need_the_process_wide_switch(enumerated):
    """every exception is produced with no_half = 1 only (the enumeration runs no_half = 0 first and keeps the first inputs)"""
    for e, why in EXCEPTIONS.items():
        assert enumerated[e]["no_half"] == 1 and "CLIMA_HIP_NO_HALF" in why, e


def test_the_table_has_its_rows():
    """a row that is deleted or renamed is missed here, whether or not another row names its instances too"""
    assert [r.name for r in LF.ROWS] == (
        "nz1 nz2 s64 h65 h100 h130 h170 h224 w225 w257 w350 w512 b513 p230 p258 p402 c65 c130 c256 c257 r1-70 r1-130 r1-200 "
        "r1c-70 r1c-150 r1c-200 r2-100 r2-150 r2-200 r2c-70 r2c-130 r2c-200 r2-300 g4-70 g16-100 g16-300 g32-40 z17-100 "
        "z17-130").split()


def test_settings_are_spread_over_both_batch_forms():
    """each setting sits in a one-launch row and in a per-column row, and no row carries two"""
    settings = {"no hard surface": lambda r: not r.hard, "per-bin surface": lambda r: r.per_bin_surface,
                "scalars": lambda r: r.diurnal_fac is not None and r.photon_scale_factor is not None,
                "zero species": lambda r: r.zero_species is not None, "scaled radii": lambda r: r.radii_scale is not None}
    for name, has in settings.items():
        forms = {r.one_launch for r in LF.ROWS if has(r)}
        assert forms == {True, False}, name
    for r in LF.ROWS:
        assert sum(bool(has(r)) for has in settings.values()) <= 1, r.name
