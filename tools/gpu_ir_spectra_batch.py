#!/usr/bin/env python3
"""What radtran_ir_spectra_batch costs against the calls it replaces, on the GPU.

At config 2's shape (200 layers, 600 IR bins) and at the 102-layer doubled grid (400 bins), for 1, 64 and 1024 columns, in
ONE process, alternating the variants, `--repeats` timed repeats each after one warm-up of every variant:
  (s1) ir_spectra_batch, TOA up alone
  (s2) ir_spectra_batch, TOA up and ground down, fluxes=True
       with the device time of the adjoint pass (the weights) and of the apply + integrate kernels of the same calls,
       from HIP events on the handle's stream (profile ids 4 and 5), in a run of their own
  (a)  what the call replaces: a loop of IR-only calls, each followed by the two spectra getters
  (b)  radiate_ir_batch with ir_green = 0 on the same columns, for context: all levels, no spectra
Times are host clocks around synchronous calls; the medians are reported.

  python tools/gpu_ir_spectra_batch.py [--out FILE] [--repeats 9] [--small]

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
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--small", action="store_true")
args = ap.parse_args()

from clima_amd import lib  # noqa: E402
from clima_amd import synthetic as S  # noqa: E402
from clima_amd.atmosphere import copy_atm_to_radiative_grid  # noqa: E402
from clima_amd.radtran import Radtran  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return t


def row(name, ms, extra=""):
    med = statistics.median(ms)
    say("    %-44s median %9.3f ms  (min %9.3f  max %9.3f)%s" % (name, med, min(ms), max(ms), extra))
    return med


def measure(title, tables, col, ncols, repeats):
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    nw_ir = len(r.ir.freq) - 1
    say("%s: %d layers, %d IR bins x %d g-points; library %s"
        % (title, nz, nw_ir, len(tables.ktables[0]["weights"]), os.path.relpath(lib.LIB_PATH)))
    rng = np.random.default_rng(nz)
    rest = col.args()[2:]
    for n in ncols:
        T = np.asfortranarray(np.asarray(col["T"], dtype=float)[:, None] + rng.uniform(-15.0, 15.0, (nz, n)))
        Ts = float(col["T_surface"]) + rng.uniform(-15.0, 15.0, n)

        def loop():
            up, dn = np.empty((nw_ir, n)), np.empty((nw_ir, n))
            for c in range(n):
                r.radiate(Ts[c], T[:, c], *rest, compute_solar=False, compute_opacity=False)
                up[:, c] = np.array(r.wrk_ir.fup_a)[nz, :]
                dn[:, c] = np.array(r.wrk_ir.fdn_a)[0, :]
            return up, dn

        def ir_batch():
            r.ir_green = 0
            return r.radiate_ir_batch(Ts, T)

        s1 = lambda: r.ir_spectra_batch(Ts, T)                                                              # noqa: E731
        s2 = lambda: r.ir_spectra_batch(Ts, T, levels=(-1, 0), parts=("up", "dn"), fluxes=True)             # noqa: E731
        variants = [("(s1) ir_spectra_batch, TOA up", s1), ("(s2) ir_spectra_batch, TOA up + ground dn, fluxes", s2),
                    ("(a) loop of IR-only calls + getters", loop), ("(b) radiate_ir_batch, ir_green = 0", ir_batch)]
        # the loop at 1024 columns takes tens of milliseconds per repeat: fewer repeats, the same median
        reps = {name: (max(3, repeats // 3) if name.startswith("(a)") and n > 64 else repeats) for name, _ in variants}
        got = {name: fn() for name, fn in variants}              # the warm-up, and a look at the values
        up, dn = got[variants[2][0]]
        g = got[variants[1][0]]
        e = max(np.max(np.abs(g["fup"][:, 0, :] - up)) / np.max(np.abs(up)), np.max(np.abs(g["fdn"][:, 1, :] - dn)) / np.max(np.abs(dn)))
        say("  %d column(s); (s2) against (a): %.1e of the spectra's maximum" % (n, e))
        times = {name: [] for name, _ in variants}
        for k in range(repeats):
            for name, fn in variants:
                if k < reps[name]:
                    times[name] += timed(fn, 1)
        med = {name: row(name, times[name]) for name, _ in variants}
        # device time of the two parts, events on the handle's stream, in calls of their own
        for name, fn in variants[:2]:
            r.profile(True)
            r.profile_reset()
            for _ in range(repeats):
                fn()
            (ms_w, n_w), (ms_a, n_a) = r.kernel_time(4), r.kernel_time(5)
            r.profile(False)
            say("    %-44s device: adjoint pass %.3f ms, apply + integrate %.3f ms per call (means of %d)"
                % (name[:4], ms_w / max(n_w, 1), ms_a / max(n_w, 1), n_w))
        say("    (a) / (s1) = %.1f; (a) / (s2) = %.1f; (b) / (s2) = %.2f"
            % (med[variants[2][0]] / med[variants[0][0]], med[variants[2][0]] / med[variants[1][0]], med[variants[3][0]] / med[variants[1][0]]))
    r.radiate(*col.args(), compute_solar=False, compute_opacity=False)


if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=110), S.modern_earth_column(40), (1, 20)),
              ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(15))), (3,))]
else:
    shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200), (1, 64, 1024)),
              ("102 layers x 400 bins", S.modern_earth_tables(nw=400), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), (1, 64, 1024))]
for title, tables, col, ncols in shapes:
    measure(title, tables, col, ncols, args.repeats)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
