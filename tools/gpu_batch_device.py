#!/usr/bin/env python3
"""Developer diagnostic: a column batch whose inputs are resident as torch tensors, two ways on one handle --
  device: Radtran.TOA_fluxes_batch_tensors (radtran_toa_fluxes_batch_device) + synchronize: nothing leaves the device;
  host:   what the same caller had to do before: .cpu() of the tensors, TOA_fluxes_batch, the results back up.
The two alternate in one process, 2 warm-ups and 10 timed passes each: medians, minima and the spread (max - min).
Cases: config 4 of BASELINE.json (1 024 perturbed columns, 200 layers, 1 000 bins) and 64 columns of the
AdiabatClimate-like shape (102-layer doubled grid, 400 bins, 4 zenith angles).
Usage: gpu_batch_device.py [config4|adiabat ...] [ncol=N]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from clima_amd import synthetic as S
from clima_amd.atmosphere import copy_atm_to_radiative_grid
from clima_amd.radtran import Radtran

WARM, REPS = 2, 10


def stack(cols, np_):
    a = dict(T_surface=np.array([float(c["T_surface"]) for c in cols]), T=np.stack([c["T"] for c in cols]),
             P=np.stack([c["P"] for c in cols]), densities=np.ascontiguousarray(np.stack([np.asarray(c["densities"]).T for c in cols])),
             dz=np.stack([c["dz"] for c in cols]))
    if np_ > 0:
        a["pdensities"] = np.ascontiguousarray(np.stack([np.asarray(c["pdensities"]).T for c in cols]))
        a["radii"] = np.ascontiguousarray(np.stack([np.asarray(c["radii"]).T for c in cols]))
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda() for k, v in a.items()}


def host_route(r, t):
    """tensors -> host arrays -> radtran_toa_fluxes_batch -> tensors (the column dicts of TOA_fluxes_batch are views)"""
    h = {k: v.cpu().numpy() for k, v in t.items()}
    cols = []
    for c in range(h["T"].shape[0]):
        col = dict(T_surface=h["T_surface"][c], T=h["T"][c], P=h["P"][c], dz=h["dz"][c], densities=h["densities"][c].T)
        if "radii" in h:
            col.update(pdensities=h["pdensities"][c].T, radii=h["radii"][c].T)
        cols.append(col)
    isr, olr, fl = r.TOA_fluxes_batch(cols, return_fluxes=True)
    return torch.from_numpy(isr).cuda(), torch.from_numpy(olr).cuda(), torch.from_numpy(np.ascontiguousarray(np.transpose(fl, (2, 1, 0)))).cuda()


def device_route(r, t):
    return r.TOA_fluxes_batch_tensors(**t, return_fluxes=True)      # sync=True: ends with synchronize()


def stats(t):
    t = np.asarray(t) * 1e3
    return "median %.3f ms (min %.3f, spread %.3f)" % (np.median(t), t.min(), t.max() - t.min())


def run(label, r, cols):
    t = stack(cols, r.np)
    n = len(cols)
    td, th = [], []
    for rep in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = device_route(r, t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        h = host_route(r, t)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep >= WARM:
            td.append(t1 - t0); th.append(t2 - t1)
    same = all(bool(torch.equal(a, b)) for a, b in zip(d, h))
    md, mh = float(np.median(td)), float(np.median(th))
    print("%s, %d columns, %d alternating passes:\n  device arrays + synchronize   %s = %.1f us per column\n"
          "  .cpu(), host batch, .cuda()   %s = %.1f us per column\n  ratio host / device %.3f; results bitwise equal: %s; "
          "fused_fallbacks %d" % (label, n, REPS, stats(td), md * 1e6 / n, stats(th), mh * 1e6 / n, mh / md, same, r.fused_fallbacks),
          flush=True)


args = [a for a in sys.argv[1:] if "=" not in a] or ["config4", "adiabat"]
ncol = next((int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("ncol=")), None)
if "config4" in args:
    r = Radtran(S.modern_earth_tables(), 200, 4, 0.15)
    run("config 4 (200 layers, 1000 bins)", r, S.perturbed_columns(ncol or 1024, nz=200, seed=7))
    del r
if "adiabat" in args:
    cols = [S.Column(copy_atm_to_radiative_grid(c)) for c in S.perturbed_columns(ncol or 64, nz=50, seed=7)]
    r = Radtran(S.modern_earth_tables(nw=400), len(cols[0]["T"]), 4, 0.15)
    run("AdiabatClimate-like (102-layer doubled grid, 400 bins)", r, cols)
