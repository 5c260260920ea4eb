#!/usr/bin/env python3
"""Cost of per-column surface, zenith and stellar scaling in the column batches (radtran_toa_fluxes_batch_bounds, host
and device form), on the GPU.

For each shape, in ONE process, alternating the variants, five timed repeats each after one warm-up of every variant:
  (a) the plain batches:                TOA_fluxes_batch / TOA_fluxes_batch_tensors (+ synchronize)
  (b) the bounds batches with all five arrays (surface_albedo, surface_emissivity, zenith_u, zenith_weights,
      photon_scale_factor), every column its own
  (c) what (b) replaces: the five setters, then one TOA_fluxes, per column
Times are host clocks around calls that end in a device synchronise; the device form's input tensors (the bounds
among them) are made once, outside the timed window; its results stay on the device.

  python tools/gpu_batch_bounds.py [--out FILE] [--plain-only] [--repeats 5] [--small]

--plain-only: variant (a) alone, declaring only the symbols a library without the bounds entry points exports, so that
CLIMA_HIP_LIB can name a build of the parent commit: run it alternately with this build's for the A/B of the unchanged
path (the plain batch must lie within the parent's own spread).
--small: tiny shapes, to rehearse the script."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--small", action="store_true")
args = ap.parse_args()

from clima_amd import lib  # noqa: E402
if args.plain_only:
    for name in ("radtran_toa_fluxes_batch_bounds", "radtran_toa_fluxes_batch_bounds_device", "clima_test_pack_bounds",
                 "clima_test_pack_bounds_host"):
        lib.SIGNATURES.pop(name, None)
import torch  # noqa: E402
from clima_amd import synthetic as S  # noqa: E402
from clima_amd.atmosphere import copy_atm_to_radiative_grid  # noqa: E402
from clima_amd.radtran import Radtran  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stacked_tensors(cols, np_):
    a = dict(T_surface=np.array([float(c["T_surface"]) for c in cols]),
             T=np.stack([np.asarray(c["T"], dtype=np.float64) for c in cols]),
             P=np.stack([np.asarray(c["P"], dtype=np.float64) for c in cols]),
             densities=np.ascontiguousarray(np.stack([np.asarray(c["densities"], dtype=np.float64).T for c in cols])),
             dz=np.stack([np.asarray(c["dz"], dtype=np.float64) for c in cols]))
    if np_ > 0:
        a["pdensities"] = np.ascontiguousarray(np.stack([np.asarray(c["pdensities"], dtype=np.float64).T for c in cols]))
        a["radii"] = np.ascontiguousarray(np.stack([np.asarray(c["radii"], dtype=np.float64).T for c in cols]))
    return {k: torch.from_numpy(v).cuda() for k, v in a.items()}


def make_bounds(r, n, seed=11):
    """every column its own: albedo and emissivity ramps, zenith angles and scale, each scaled by a column's factor"""
    rng = np.random.default_rng(seed)
    n_sol, n_ir = len(r.sol.freq) - 1, len(r.ir.freq) - 1
    u, w = np.asarray(r.zenith_u, dtype=float), np.asarray(r.zenith_weights, dtype=float)
    f = rng.uniform(0.3, 1.0, size=(5, n))
    b = dict(surface_albedo=f[0][:, None] * np.linspace(0.05, 0.85, n_sol)[None, :],
             surface_emissivity=f[1][:, None] * np.linspace(0.6, 1.0, n_ir)[None, :],
             zenith_u=f[2][:, None] * u[None, :], zenith_weights=f[3][:, None] * w[None, :], photon_scale_factor=2.0 * f[4])
    return {k: np.ascontiguousarray(v) for k, v in b.items()}


def measure(title, tables, cols, nzen, albedo):
    nz, n = len(cols[0]["T"]), len(cols)
    r = Radtran(tables, nz, nzen, albedo)
    t = stacked_tensors(cols, r.np)
    variants = [("(a) host batch, plain", lambda: r.TOA_fluxes_batch(cols)),
                ("(a) device batch, plain", lambda: r.TOA_fluxes_batch_tensors(**t))]
    if not args.plain_only:
        b = make_bounds(r, n)
        bt = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
        own = {k: np.array(getattr(r, k), dtype=float, copy=True) for k in b}

        def singles():
            for c, col in enumerate(cols):
                r.surface_albedo, r.surface_emissivity = b["surface_albedo"][c], b["surface_emissivity"][c]
                r.zenith_u, r.zenith_weights = b["zenith_u"][c], b["zenith_weights"][c]
                r.photon_scale_factor = float(b["photon_scale_factor"][c])
                r.TOA_fluxes(*col.args())
            r.surface_albedo, r.surface_emissivity = own["surface_albedo"], own["surface_emissivity"]
            r.zenith_u, r.zenith_weights = own["zenith_u"], own["zenith_weights"]
            r.photon_scale_factor = float(own["photon_scale_factor"])

        variants += [("(b) host bounds batch, five arrays", lambda: r.TOA_fluxes_batch(cols, bounds=b)),
                     ("(b) device bounds batch, five arrays", lambda: r.TOA_fluxes_batch_tensors(**t, bounds=bt)),
                     ("(c) five setters + TOA_fluxes per column", singles)]
    times = {name: [] for name, _ in variants}
    for name, f in variants:      # warm-up: code objects, arenas, staging buffers
        f()
    for _ in range(args.repeats):
        for name, f in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    say("%s: %d columns x %d layers, %d + %d bins, %d zenith angles; library %s"
        % (title, n, nz, len(r.ir.freq) - 1, len(r.sol.freq) - 1, nzen, os.path.basename(lib.LIB_PATH)))
    for name, _ in variants:
        ms = [1e3 * x for x in times[name]]
        med = statistics.median(ms)
        say("  %-44s median %9.3f ms  (min %9.3f  max %9.3f)  %9.0f columns/s   repeats: %s"
            % (name, med, min(ms), max(ms), n / (med * 1e-3), " ".join("%.3f" % x for x in ms)))
    assert r.fused_fallbacks == 0, "a batch was repeated: the times above are not the fused form's"
    return {name: statistics.median(v) for name, v in times.items()}


if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=60), S.perturbed_columns(9, nz=100, seed=3), 2, 0.2),
              ("small B", S.modern_earth_tables(nw=40), [S.Column(copy_atm_to_radiative_grid(c)) for c in S.perturbed_columns(5, 50, seed=5)], 2, 0.3)]
else:
    shapes = [("config 4", S.modern_earth_tables(), S.perturbed_columns(1024, nz=200, seed=7), 8, 0.15),
              ("doubled grid", S.modern_earth_tables(nw=400),
               [S.Column(copy_atm_to_radiative_grid(c)) for c in S.perturbed_columns(64, 50, seed=5)], 8, 0.15)]
for shape in shapes:
    m = measure(*shape)
    if not args.plain_only:
        for form in ("host", "device"):
            a, b = m["(a) %s batch, plain" % form], m["(b) %s bounds batch, five arrays" % form]
            say("  %s form: (b) / (a) = %.3f; (c) / (b) = %.1f" % (form, b / a, m["(c) five setters + TOA_fluxes per column"] / b))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
