#!/usr/bin/env python3
"""What radtran_radiate_solar_batch costs against what it replaces, on the GPU.

For 64 and 1024 illumination cases, at config 2's column (200 layers, 600 solar bins) and at the 102-layer x 400-bin shape
(the doubled radiative grid), with one angle per case and with the handle's 4 angles, in ONE process, alternating the
variants, `--repeats` timed repeats each after one warm-up of every variant:
  (a) radiate_solar_batch, the shared kernel (k_twostream_sol_batch)
  (b) radiate_solar_batch, one full solve per case (radtran_solar_batch_shared_set(0))
  (c) what both replace: the setters, then radiate(compute_solar=True, compute_opacity=False), per case
  (d) TOA_fluxes_batch(bounds=...) on ncol copies of the column (every copy computes the opacities again)
Times are host clocks around synchronous calls.

  python tools/gpu_solar_batch.py [--out FILE] [--repeats 5] [--small] [--few]

--small: tiny shapes, to rehearse the script.
--few: 1 to 16 cases at 402, 300 and 102 layers x 400 bins instead: where the default form of a small batch is decided."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--small", action="store_true")
ap.add_argument("--few", action="store_true")
args = ap.parse_args()

from clima_amd import lib  # noqa: E402
from clima_amd import synthetic as S  # noqa: E402
from clima_amd.atmosphere import copy_atm_to_radiative_grid  # noqa: E402
from clima_amd.radtran import Radtran  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(title, tables, col, handle_nzen, albedo, ncase, nzen):
    nz = len(col["T"])
    r = Radtran(tables, nz, handle_nzen, albedo)
    r.radiate(*col.args())
    n_sol = len(r.sol.freq) - 1
    rng = np.random.default_rng(11)
    f = rng.uniform(0.3, 1.0, size=(4, ncase))
    if nzen == 1:
        zu, zw = f[0][:, None].copy(), np.ones((ncase, 1))
    else:
        u, w = np.asarray(r.zenith_u, dtype=float), np.asarray(r.zenith_weights, dtype=float)
        zu, zw = np.ascontiguousarray(f[0][:, None] * u[None, :]), np.ascontiguousarray(f[1][:, None] * w[None, :])
    alb = np.ascontiguousarray(f[2][:, None] * np.linspace(0.05, 0.85, n_sol)[None, :])
    scale = 2.0 * f[3]
    args_col = col.args()
    rc = r      # the handle of (c): one made with the batch's number of angles where that is not the handle's
    if nzen != handle_nzen:
        rc = Radtran(tables, nz, nzen, albedo)
        rc.radiate(*args_col)
    own = {k: np.array(getattr(rc, k), dtype=float, copy=True) for k in ("zenith_u", "zenith_weights", "surface_albedo", "photon_scale_factor")}

    def batch(shared):
        r.solar_batch_shared(shared)
        return r.radiate_solar_batch(zu, zw, alb, scale)

    def singles():
        for c in range(ncase):
            rc.zenith_u, rc.zenith_weights = zu[c], zw[c]
            rc.surface_albedo, rc.photon_scale_factor = alb[c], float(scale[c])
            rc.radiate(*args_col, compute_solar=True, compute_opacity=False)
        rc.zenith_u, rc.zenith_weights = own["zenith_u"], own["zenith_weights"]
        rc.surface_albedo, rc.photon_scale_factor = own["surface_albedo"], float(own["photon_scale_factor"])

    variants = [("(a) solar batch, shared kernel", lambda: batch(1)), ("(b) solar batch, one solve per case", lambda: batch(0)),
                ("(c) setters + radiate per case", singles)]
    if nzen == handle_nzen:      # (the bounds batch takes the handle's number of angles)
        cols = [col] * ncase
        bounds = dict(zenith_u=zu, zenith_weights=zw, surface_albedo=alb, photon_scale_factor=scale)
        variants.append(("(d) TOA_fluxes_batch(bounds) on copies", lambda: r.TOA_fluxes_batch(cols, bounds=bounds)))
    times = {name: [] for name, _ in variants}
    a, b = batch(1), batch(0)
    worst = max(float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in zip(a[:2], b[:2]))
    for name, fn in variants[2:]:
        fn()
    for _ in range(args.repeats):
        r.radiate(*args_col)      # (a column batch leaves its optical properties in its own memory: the handle's own again)
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    say("%s: %d cases x %d angle(s), %d layers, %d solar bins; (a) against (b): %.1e of the largest flux; library %s"
        % (title, ncase, nzen, nz, n_sol, worst, os.path.basename(lib.LIB_PATH)))
    med = {}
    for name, _ in variants:
        ms = [1e3 * x for x in times[name]]
        med[name] = statistics.median(ms)
        say("  %-40s median %9.3f ms  (min %9.3f  max %9.3f)  %7.2f us/case   repeats: %s"
            % (name, med[name], min(ms), max(ms), 1e3 * med[name] / ncase, " ".join("%.3f" % x for x in ms)))
    names = [n for n, _ in variants]
    say("  (b) / (a) = %.2f; (c) / (a) = %.1f%s" % (med[names[1]] / med[names[0]], med[names[2]] / med[names[0]],
                                                     "; (d) / (a) = %.1f" % (med[names[3]] / med[names[0]]) if len(names) > 3 else ""))
    assert r.fused_fallbacks == 0


if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=60), S.modern_earth_column(100), 2, 0.2, (9, 40)),
              ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), 2, 0.3, (9, 40))]
elif args.few:
    # few cases on tall grids: where the IR batch prefers the single call's kernel (5-8 slots: one wave per SIMD)
    t400 = S.modern_earth_tables(nw=400)
    shapes = [("402 layers x 400 bins", t400, S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(200))), 4, 0.15, (1, 2, 4, 8, 16)),
              ("300 layers x 400 bins", t400, S.modern_earth_column(300), 4, 0.15, (1, 2, 4, 8)),
              ("102 layers x 400 bins", t400, S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), 4, 0.15, (1, 2, 4, 8))]
else:
    shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200), 4, 0.15, (64, 1024)),
              ("102 layers x 400 bins", S.modern_earth_tables(nw=400), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), 4, 0.15, (64, 1024))]
for title, tables, col, hz, albedo, counts in shapes:
    for ncase in counts:
        for nzen in (1, hz):
            measure(title, tables, col, hz, albedo, ncase, nzen)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
