#!/usr/bin/env python3
"""What the device-resident IR spectra batch and its temperature gradient cost, on the GPU.

At config 2's shape (200 layers, 600 IR bins) and at the 102-layer doubled grid (400 bins), for 64 and 1024 columns, the
top-of-atmosphere up row, in ONE process, alternating the variants, `--repeats` timed repeats each after one warm-up of
every variant:
  (a) ir_spectra_batch: host arrays, per call
  (b) ir_spectra_batch_tensors computing the weights (weights_given = 0)
  (c) ir_spectra_batch_tensors with the weights of an earlier call (weights_given = 1)
  (d) ir_spectra_vjp_tensors: the gradient, device arrays
  (e) what (d) replaces: ir_jacobian_spectral per column and the contraction with the cotangent on the host
Times are host clocks around the call and the `synchronize()` behind it; medians, with the repeats' spread.  The device
time of (b), (c), (d) from HIP events on the handle's stream (profile ids 4, 5, 6) comes from calls of their own.
  (f) the paths that existed before -- the host batch (64 columns, config 2's shape) and the single radiate call -- on this
      build and on `--parent-lib` (the parent commit's build of the library), in child processes that alternate, 3 rounds.

  python tools/gpu_ir_spectra_grad.py [--out FILE] [--repeats 9] [--small] [--parent-lib clima_amd/csrc/variants/lib_parent.so]

--small: tiny shapes, to rehearse the script."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--small", action="store_true")
ap.add_argument("--parent-lib")
ap.add_argument("--ab-child", action="store_true", help="(internal) time the existing paths on CLIMA_HIP_LIB, print one JSON line")
args = ap.parse_args()

from clima_amd import lib  # noqa: E402
if args.ab_child:
    # a build of the parent commit exports none of the new symbols: the table is cut down to what the library has
    import ctypes
    have = ctypes.CDLL(lib.LIB_PATH)
    lib.SIGNATURES = {k: v for k, v in lib.SIGNATURES.items() if hasattr(have, k)}
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
    say("    %-52s median %9.3f ms  (min %9.3f  max %9.3f)%s" % (name, med, min(ms), max(ms), extra))
    return med


def ab_child():
    tables, col = (S.modern_earth_tables(nw=110), S.modern_earth_column(40)) if args.small else (S.modern_earth_tables(), S.modern_earth_column(200))
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    rng = np.random.default_rng(nz)
    n = 64
    T = np.asfortranarray(np.asarray(col["T"], dtype=float)[:, None] + rng.uniform(-15.0, 15.0, (nz, n)))
    Ts = float(col["T_surface"]) + rng.uniform(-15.0, 15.0, n)
    batch = lambda: r.ir_spectra_batch(Ts, T)       # noqa: E731
    single = lambda: r.radiate(*col.args())         # noqa: E731
    batch(), single()
    tb, ts = [], []
    for _ in range(args.repeats):
        tb += timed(batch, 1)
        ts += timed(single, 3)
    print(json.dumps(dict(batch=[statistics.median(tb), min(tb), max(tb)], single=[statistics.median(ts), min(ts), max(ts)])))


def measure(title, tables, col, ncols, repeats):
    import torch
    nz = len(col["T"])
    r = Radtran(tables, nz, 4, 0.15)
    r.radiate(*col.args())
    nw_ir = len(r.ir.freq) - 1
    say("%s: %d layers, %d IR bins x %d g-points; library %s"
        % (title, nz, nw_ir, len(tables.ktables[0]["weights"]), os.path.relpath(lib.LIB_PATH)))
    rng = np.random.default_rng(nz)
    for n in ncols:
        T = np.asfortranarray(np.asarray(col["T"], dtype=float)[:, None] + rng.uniform(-15.0, 15.0, (nz, n)))
        Ts = float(col["T_surface"]) + rng.uniform(-15.0, 15.0, n)
        dT, dTs = torch.from_numpy(np.ascontiguousarray(T.T)).cuda(), torch.from_numpy(Ts).cuda()
        first = r.ir_spectra_batch_tensors(dTs, dT, return_weights=True, sync=True)
        w = {"w_up": first["w_up"]}
        g = {"fup": torch.from_numpy(rng.uniform(-1.0, 1.0, (n, 1, nw_ir))).cuda()}
        gh = g["fup"].cpu().numpy()[:, 0, :]

        def host():
            return r.ir_spectra_batch(Ts, T)

        def dev_weights():
            return r.ir_spectra_batch_tensors(dTs, dT, sync=True)

        def dev_given():
            return r.ir_spectra_batch_tensors(dTs, dT, weights=w, sync=True)

        def vjp():
            return r.ir_spectra_vjp_tensors(dTs, dT, w, g, sync=True)

        def rows_loop():
            out = np.empty((nz + 1, n))
            for c in range(n):
                jac = r.ir_jacobian_spectral(Ts[c], T[:, c])["up"]          # (nw_ir, 1, nz+1)
                out[:, c] = gh[c] @ jac[:, 0, :]
            return out

        variants = [("(a) ir_spectra_batch, host arrays", host), ("(b) device form, computing the weights", dev_weights),
                    ("(c) device form, weights_given = 1", dev_given), ("(d) gradient, device form", vjp),
                    ("(e) ir_jacobian_spectral per column + host contraction", rows_loop)]
        reps = {name: (max(3, repeats // 3) if name.startswith("(e)") and n > 64 else repeats) for name, _ in variants}
        got = {name: fn() for name, fn in variants}              # the warm-up, and a look at the values
        gTs, gT = got[variants[3][0]]
        mine = np.concatenate([gTs.cpu().numpy()[None, :], gT.cpu().numpy().T])
        loop = got[variants[4][0]]
        say("  %d columns; (d) against (e): %.1e of the gradient's maximum; (c) against (a): %s"
            % (n, np.max(np.abs(mine - loop)) / np.max(np.abs(loop)),
               "bit for bit" if got[variants[2][0]]["fup"].cpu().numpy().tobytes() == got[variants[0][0]]["fup"].tobytes(order="F") else "DIFFERENT"))
        times = {name: [] for name, _ in variants}
        for k in range(repeats):
            for name, fn in variants:
                if k < reps[name]:
                    times[name] += timed(fn, 1)
        med = {name[:3]: row(name, times[name]) for name, _ in variants}
        dev_ms = {}
        for name, fn in variants[1:4]:
            r.profile(True)
            r.profile_reset()
            for _ in range(repeats):
                fn()
            ms = [r.kernel_time(k) for k in (4, 5, 6)]
            r.profile(False)
            dev_ms[name[:3]] = [m / repeats for m, _ in ms]
            say("    %-4s device: adjoint pass %.3f ms, apply %.3f ms, gradient %.3f ms per call (means of %d)"
                % (name[:3], dev_ms[name[:3]][0], dev_ms[name[:3]][1], dev_ms[name[:3]][2], repeats))
        say("    (d) / (c) = %.2f by the host clock, %.2f by the device time of the kernels; (e) / (d) = %.0f; (a) / (c) = %.2f"
            % (med["(d)"] / med["(c)"], dev_ms["(d)"][2] / max(dev_ms["(c)"][1], 1e-9), med["(e)"] / med["(d)"], med["(a)"] / med["(c)"]))
    r.radiate(*col.args(), compute_solar=False, compute_opacity=False)


def ab(parent):
    say("(f) the existing paths, this build against the parent commit's (%s): child processes, alternating, 3 rounds" % os.path.relpath(parent))
    res = {"this build": [], "parent": []}
    for rnd in range(3):
        for name, path in (("this build", None), ("parent", os.path.abspath(parent))):
            env = dict(os.environ)
            if path:
                env["CLIMA_HIP_LIB"] = path
            else:
                env.pop("CLIMA_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", "--repeats", str(args.repeats)] + (["--small"] if args.small else [])
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                say("    %s round %d FAILED: %s" % (name, rnd + 1, out.stderr.strip().splitlines()[-1] if out.stderr.strip() else out.returncode))
                continue
            d = json.loads(out.stdout.strip().splitlines()[-1])
            res[name].append(d)
            say("    %-10s round %d: ir_spectra_batch, 64 columns: median %8.3f ms (min %8.3f max %8.3f); radiate: median %8.3f ms (min %8.3f max %8.3f)"
                % (name, rnd + 1, *d["batch"], *d["single"]))
    for key, what in (("batch", "ir_spectra_batch"), ("single", "radiate")):
        if res["this build"] and res["parent"]:
            a, b = [d[key][0] for d in res["this build"]], [d[key][0] for d in res["parent"]]
            inside = min(b) <= statistics.median(a) <= max(b) or min(a) <= statistics.median(b) <= max(a)
            say("    %s: medians of the rounds, this build %s, parent %s: %s the rounds' spread"
                % (what, " ".join("%.3f" % v for v in a), " ".join("%.3f" % v for v in b), "inside" if inside else "OUTSIDE"))


if args.ab_child:
    ab_child()
    sys.exit(0)
if args.small:
    shapes = [("small A", S.modern_earth_tables(nw=110), S.modern_earth_column(40), (4, 20)),
              ("small B", S.modern_earth_tables(nw=40), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(15))), (3,))]
else:
    shapes = [("config 2's column", S.modern_earth_tables(), S.modern_earth_column(200), (64, 1024)),
              ("102 layers x 400 bins", S.modern_earth_tables(nw=400), S.Column(copy_atm_to_radiative_grid(S.modern_earth_column(50))), (64, 1024))]
for title, tables, col, ncols in shapes:
    measure(title, tables, col, ncols, args.repeats)
say("(d) / (c), where the gradient's time goes: per (bin, level, column) the forward (k_rows_apply) evaluates planck_fcn -- one")
say("  table-driven fast_exp and two f64 divisions -- and the gradient (k_vjp_rows) adjoint_dbdt -- the library's exp and expm1 and")
say("  four f64 divisions (x = . / T, x / em, e / em, / T) --, beside one cotangent load and two FMAs: 310 vector instructions per")
say("  column in k_vjp_rows<4>'s assembly against 85 in k_rows_apply<1, 4>'s.  At 1 024 columns both kernels fill the device and the")
say("  device-time ratio above is that arithmetic's, more than the exponentials' count (2 : 1) alone; at 64 columns the gradient's")
say("  grid (a wave per level and column tile) fills the device where the forward's (a wave per 64 bins and column tile) does not.")
if args.parent_lib:
    ab(args.parent_lib)
else:
    say("(f) not measured: no --parent-lib given")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
