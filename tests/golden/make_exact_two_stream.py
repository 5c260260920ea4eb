#!/usr/bin/env python3
"""Generate tests/golden/exact_two_stream_<i>.npz: what the two-stream SYSTEM gives, from tests/exact_two_stream.py
(mpmath, 50 digits, rounded once to float64).  Needs mpmath, the golden inputs (twostream_golden_*.npz) and the CPU
oracle (for the conditions below); neither the reference nor oracle/_ref.  Data only: inputs and exact outputs.

a. Golden cases.  c00...c89: ir_fup, ir_fdn, sol_fup, sol_fdn, sol_amean of the golden inputs; r00...: the fluxes of the
   changed Planck profiles (rMM_cJ_fup / _fdn).

b. New columns, inputs and exact outputs, smooth Planck profiles as golden cases 36... have them.
   e00...  edge columns, the fields of a golden case.  Heights 6, 65, 130 (one, two and three layer slots of the wave
           kernels, and an end in the middle of a slot); `edge_kind` names each, `edge_paired` marks the versions of
           pairwise identical layers (3, 33, 65 distinct layers doubled: nz 6, 66, 130).
           mixed-*: g in [-0.6, 0.9], one layer of tau = 0, one of tau = 3e4, one of w0 = 0, one at both caps
             (w0 = 0.99999, g = 0.999999); hard surface with emissivity 1, no hard surface, hard surface with
             emissivity 0.7.  The unpaired ones carry deviation lists for the response form (eNN_dev_k, _dev_db (2, 7):
             top level, surface, two neighbouring levels mid-column and three random levels, at 3 % and at 1e-4 of
             the level's Planck value; _dev_up, _dev_dn (2, 7, nz+1) the exact changes; _dev_umax the largest entry of
             the column's exact unit-response matrices, the scale a change is measured on after the factor dB).
           res-top-*, res-mid-*: one layer (the top one, the middle one) with its w0 tuned so that its lambda, formed in
             double from the delta-scaled w0' and g' as the solvers form it, is the double nearest (1 + off) / u0:
             the solar source terms divide by lambda^2 - 1/u0^2.  off = 1e-4, 1e-6 and 1e-8 at both placements; u0
             from 0.59 to 1 (U0S).
   m00...  multi-angle illumination sets for the solar batch: a res-mid column (off = 1e-6), 5 cases of nzen = 3 or 16
           angles (zen_u, zen_w (5, nzen), rsfc (5)) -> fup, fdn, amean (5, nz+1) = sum_z w_z solar(u_z).  The first
           angle of case 0 is the column's near-resonant u0; one weight of case 2 is exactly 0.
   u00...  unit-response matrices up, dn [level, k] at nz = 3, 33, 65, hard and no hard surface, emissivity 0.8: w0 up
           to the cap, layer 1 below ir_tau_min and layer 0 above it.

c. Conditions of the fixture (asserted by `check_conditions`, not measurements): on every new column the reference
   algorithm's true error -- the larger of the oracle's two compilations against exact -- is at most 1e-9 of the
   channel's largest flux (amean, and the unit matrices, on their own largest value), and both compilations are finite.
   A new case cannot hide behind a bound that its own reference error has loosened.
   Near resonance the source terms grow as 1 / off and cancel against the homogeneous solution, which costs the
   reference about 2^-53 w0' / off whatever the layer's thickness.  At off = 1e-8 the condition therefore needs a small
   w0': the tuned layer gets u0 = 0.59 (top) or 0.6 (mid-column), where lambda = 1/u0 is met at w0 of 0.05 to 0.09, and
   the reference stays within 9.2e-10 (with u0 of 0.75 and more, w0' of 0.3 to 0.7, it is 1e-8 off and over the limit).
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import exact_two_stream as X  # noqa: E402

PART_BYTES = 800_000
TAU_MIN = 1.0e-6
HEIGHTS = (6, 65, 130)
OFFS = (1e-4, 1e-6, 1e-8)
U0S = {1e-4: (0.62, 0.9), 1e-6: (0.7, 1.0), 1e-8: (0.59, 0.6)}      # (top, mid); at 1e-8 a small w0': see c.
MAX_W0, MAX_GT = 0.99999, 0.999999
REF_ERR_MAX = 1e-9


def load(pattern):
    d = {}
    for p in sorted(glob.glob(os.path.join(HERE, pattern))):
        with np.load(p) as z:
            d.update({k: z[k] for k in z.files})
    return d


def split_parts(out):
    """make_twostream_golden.split_parts: the arrays in key order, in parts of at most PART_BYTES uncompressed."""
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        v = np.asarray(v)
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    return parts


# ------------------------------------------------------------------------------------------------ inputs

def _planck(rng, nz, power, nu):
    h, kb, cl = 6.62607004e-34, 1.380649e-23, 299792458.0
    lev = np.linspace(0.0, 1.0, nz + 1)
    T = 180.0 + 110.0 * lev ** power + rng.uniform(-1.0, 1.0, nz + 1)
    return 1.0e3 * ((2.0 * h * nu ** 3) / cl ** 2) / (np.exp((h * nu) / (kb * T)) - 1.0)


def _smooth_tau(rng, n, lo=-3.0, hi=1.5):
    mid = (np.arange(n) + 0.5) / n
    return (10.0 ** rng.uniform(lo, hi)) * (mid ** 2 + 1e-4) / n * 40.0 * 10 ** rng.uniform(-0.3, 0.3, n)


def lambda_double(w0_in, gt_in):
    """the solar lambda of one layer as oracle/clima_oracle.c:305-312 forms it, in double"""
    w0 = w0_in * (1.0 - gt_in * gt_in) / (1.0 - w0_in * gt_in * gt_in)
    gt = gt_in / (1.0 + gt_in)
    s3 = np.sqrt(3.0)
    gam1 = s3 * (2.0 - w0 * (1 + gt)) / 2.0
    gam2 = s3 * w0 * (1.0 - gt) / 2.0
    return float(np.sqrt(gam1 * gam1 - gam2 * gam2))


def tune_w0(gt_in, u0, off):
    """w0 of a layer with asymmetry gt_in whose double lambda is nearest (1 + off) / u0: lambda falls with w0, bisect."""
    target = (1.0 + off) / u0
    lo, hi = 0.0, MAX_W0
    assert lambda_double(lo, gt_in) > target > lambda_double(hi, gt_in), (gt_in, u0)
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if lambda_double(mid, gt_in) > target:
            lo = mid
        else:
            hi = mid
    return min((lo, hi), key=lambda w: abs(lambda_double(w, gt_in) - target))


def _mixed_layers(rng, n):
    tau = _smooth_tau(rng, n)
    w0 = rng.uniform(0.0, MAX_W0, n)
    g = rng.uniform(-0.6, 0.9, n)
    g[0], g[n - 1] = -0.6, 0.9
    if n >= 6:
        zero, w0zero, caps, thick = n // 5, n // 3, n // 2, n - 2
    else:
        zero, w0zero, caps, thick = 0, 0, 1, 2
    tau[zero] = 0.0
    w0[w0zero] = 0.0
    w0[caps], g[caps] = MAX_W0, MAX_GT
    tau[caps] = 0.4         # (at the caps 1 / (gam1 + gam2) = 5e4: a thin layer there costs the reference 1e-8 on unit vectors)
    tau[thick] = 3.0e4
    return tau, w0, g


def _resonant_layers(rng, n, where, u0, off):
    tau = _smooth_tau(rng, n, -1.5, 0.5)
    w0 = rng.uniform(0.0, 0.9, n)
    g = rng.uniform(0.0, 0.85, n)
    r = 0 if where == "top" else n // 2
    tau[r] = 0.3 if where == "top" else 0.5
    g[r] = float(rng.uniform(0.1, 0.7))
    w0[r] = tune_w0(g[r], u0, off)
    return tau, w0, g


def new_inputs():
    """Every input of part b, deterministic."""
    out = {}
    kinds, paired_flags = [], []
    rng = np.random.default_rng(20261020)
    n = 0

    def add(kind, paired, layers, bp, ir_par, sol_par):
        nonlocal n
        tau, w0, g = layers
        if paired:
            tau, w0, g = np.repeat(tau, 2), np.repeat(w0, 2), np.repeat(g, 2)
        k = "e%02d_" % n
        out.update({k + "tau": tau, k + "w0": w0, k + "g": g, k + "bplanck": bp,
                    k + "ir_par": np.array(ir_par, dtype=float), k + "sol_par": np.array(sol_par, dtype=float)})
        kinds.append(kind)
        paired_flags.append(paired)
        n += 1
        return k

    surfaces = (("hard", 1.0, 1.0), ("nosfc", 1.0, 0.0), ("em07", 0.7, 1.0))
    for paired in (False, True):
        for nz in HEIGHTS:
            nd = nz if not paired else (nz + 1) // 2          # 6 / 65 / 130, or 3 / 33 / 65 doubled
            nzc = nd * (2 if paired else 1)
            for si, (name, em, hs) in enumerate(surfaces):
                bp = _planck(rng, nzc, (1.0, 2.5, 1.5)[si], (2.0e13, 6.0e13, 4.0e13)[si])
                k = add("mixed-" + name, paired, _mixed_layers(rng, nd), bp, (em, hs, TAU_MIN),
                        ((0.6, 0.2), (0.25, 0.6), (0.9, 1.0))[si])
                if not paired:
                    fixed = [0, nzc, nzc // 2, nzc // 2 + 1]
                    rest = [i for i in range(nzc + 1) if i not in fixed]
                    ks = fixed + sorted(int(x) for x in rng.choice(rest, 3, replace=False))
                    rel = np.array([0.03, 1e-4])[:, None] * (1.0 + rng.random((2, len(ks))))
                    out[k + "dev_k"] = np.array([ks, ks])
                    out[k + "dev_db"] = rel * bp[ks][None, :]
            j = 0
            for where in ("top", "mid"):
                for off in OFFS:
                    u0 = U0S[off][where == "mid"]
                    bp = _planck(rng, nzc, 1.0 + 0.3 * j, 3.0e13)
                    add("res-%s-%.0e" % (where, off), paired, _resonant_layers(rng, nd, where, u0, off), bp,
                        (0.9, float(j % 2), TAU_MIN), (u0, (0.3, 0.0, 0.8)[j % 3]))
                    j += 1
    out["edge_n"] = np.array([n])
    out["edge_kind"] = np.array(kinds)
    out["edge_paired"] = np.array(paired_flags)

    # ---- multi-angle illumination sets
    rng = np.random.default_rng(20261021)
    m = 0
    for nz in HEIGHTS:
        for nzen in (3, 16):
            u_res = (0.7, 0.85, 0.95)[HEIGHTS.index(nz)]
            tau, w0, g = _resonant_layers(rng, nz, "mid", u_res, 1e-6)
            x, w = np.polynomial.legendre.leggauss(nzen)
            zu, zw = np.empty((5, nzen)), np.empty((5, nzen))
            for c in range(5):
                zu[c] = np.sort(rng.uniform(0.05, 1.0, nzen))
                ww = rng.uniform(0.2, 1.0, nzen)
                zw[c] = ww / ww.sum()
            zu[0, 0] = u_res
            zw[2, 1] = 0.0
            zu[4], zw[4] = x / 2 + 0.5, w / 2                 # the library's own angles (clima_radtran.f90:164-165)
            k = "m%02d_" % m
            out.update({k + "tau": tau, k + "w0": w0, k + "g": g, k + "zen_u": zu, k + "zen_w": zw,
                        k + "rsfc": np.array([0.3, 0.0, 1.0, 0.15, 0.6])})
            m += 1
    out["multi_n"] = np.array([m])

    # ---- unit-response matrices
    rng = np.random.default_rng(20261022)
    u = 0
    for nz in (3, 33, 65):
        for hard in (True, False):
            tau = np.geomspace(3.0e-6, 2.5, nz) * rng.uniform(0.7, 1.3, nz)
            tau[0], tau[1] = 2.0 * TAU_MIN, 0.3 * TAU_MIN
            w0 = rng.uniform(0.0, MAX_W0, nz)
            w0[nz // 2] = MAX_W0
            g = rng.uniform(-0.3, 0.85, nz)
            k = "u%02d_" % u
            out.update({k + "tau": tau, k + "w0": w0, k + "g": g, k + "ir_par": np.array([0.8, float(hard), TAU_MIN])})
            u += 1
    out["unit_n"] = np.array([u])
    return out


# ------------------------------------------------------------------------------------------------ exact outputs

def column_exact(d, k, dps=X.DPS):
    """the five outputs of one column (a golden case cNN_ or an edge column eNN_)"""
    em, hs, tmin = (float(v) for v in d[k + "ir_par"])
    u0, rs = (float(v) for v in d[k + "sol_par"])
    fup, fdn = X.exact_ir(d[k + "tau"], d[k + "w0"], d[k + "g"], em, bool(hs), tmin, d[k + "bplanck"], dps=dps)
    am, sup, sdn = X.exact_solar(d[k + "tau"], d[k + "w0"], d[k + "g"], u0, rs, dps=dps)
    return {k + "ir_fup": fup, k + "ir_fdn": fdn, k + "sol_fup": sup, k + "sol_fdn": sdn, k + "sol_amean": am}


def changed_profile(gold, r, j):
    kb = "c%02d_" % int(gold[r + "base"][0])
    bp = np.array(gold[kb + "bplanck"], dtype=float)
    bp[gold[r + "c%d_k" % j]] = gold[r + "c%d_b" % j]
    return kb, bp


def response_exact(gold, r, dps=X.DPS):
    """the changed fluxes of one response case: one factorisation, one solve per changed profile"""
    import mpmath
    out = {}
    kb = "c%02d_" % int(gold[r + "base"][0])
    em, hs, tmin = (float(v) for v in gold[kb + "ir_par"])
    with mpmath.workdps(dps):
        col = X.IrColumn(gold[kb + "tau"], gold[kb + "w0"], gold[kb + "g"], em, bool(hs), tmin)
        for j in range(int(gold[r + "ncol"][0])):
            _, bp = changed_profile(gold, r, j)
            fu, fd = col.solve_mp([mpmath.mpf(float(b)) for b in bp])
            out[r + "c%d_fup" % j], out[r + "c%d_fdn" % j] = X._round(fu), X._round(fd)
    return out


def deviations_exact(d, k, dps=X.DPS):
    em, hs, tmin = (float(v) for v in d[k + "ir_par"])
    args = (d[k + "tau"], d[k + "w0"], d[k + "g"], em, bool(hs), tmin)
    ups, dns = [], []
    for s in range(2):
        up, dn = X.exact_ir_response(*args, devs=list(zip(d[k + "dev_k"][s], d[k + "dev_db"][s])), dps=dps)
        ups.append(up)
        dns.append(dn)
    u, v = X.exact_unit_responses(*args, dps=dps)
    return {k + "dev_up": np.array(ups), k + "dev_dn": np.array(dns),
            k + "dev_umax": np.array([max(np.max(np.abs(u)), np.max(np.abs(v)))])}


def multi_exact(d, k, dps=X.DPS):
    n = len(d[k + "rsfc"])
    res = [X.exact_solar_sum(d[k + "tau"], d[k + "w0"], d[k + "g"], d[k + "zen_u"][c], d[k + "zen_w"][c],
                             float(d[k + "rsfc"][c]), dps=dps) for c in range(n)]
    return {k + "amean": np.array([r[0] for r in res]), k + "fup": np.array([r[1] for r in res]),
            k + "fdn": np.array([r[2] for r in res])}


def unit_exact(d, k, dps=X.DPS):
    em, hs, tmin = (float(v) for v in d[k + "ir_par"])
    up, dn = X.exact_unit_responses(d[k + "tau"], d[k + "w0"], d[k + "g"], em, bool(hs), tmin, dps=dps)
    return {k + "up": up, k + "dn": dn}


def generate(gold=None, dps=X.DPS, progress=False):
    """-> every array of the fixture, in the order it is stored"""
    gold = load("twostream_golden_*.npz") if gold is None else gold
    out = {}
    for n in range(int(gold["ncases"][0])):
        out.update(column_exact(gold, "c%02d_" % n, dps))
    if progress:
        print("golden columns done", flush=True)
    for m in range(int(gold["nresp"][0])):
        out.update(response_exact(gold, "r%02d_" % m, dps))
    if progress:
        print("response cases done", flush=True)
    new = new_inputs()
    out.update(new)
    for n in range(int(new["edge_n"][0])):
        k = "e%02d_" % n
        out.update(column_exact(new, k, dps))
        if k + "dev_k" in new:
            out.update(deviations_exact(new, k, dps))
    for m in range(int(new["multi_n"][0])):
        out.update(multi_exact(new, "m%02d_" % m, dps))
    for u in range(int(new["unit_n"][0])):
        out.update(unit_exact(new, "u%02d_" % u, dps))
    return out


# ------------------------------------------------------------------------------------------------ conditions

def reference_errors(d, O):
    """{name: true error of the reference algorithm on a new column} -- the larger of the oracle's two compilations
    against exact (exact_two_stream_cases has the measure), relative to the quantity's scale.  Raises where a compilation
    is not finite."""
    import exact_two_stream_cases as XC
    errs = {}
    for n in range(int(d["edge_n"][0])):
        k = "e%02d_" % n
        col = XC.Column(k, "", d, k, d, None, bool(d["edge_paired"][n]))
        ref, scale = col.ref_errors(O), col.scales()
        assert col.ref_finite, "the oracle is not finite on " + k
        tag = "%s%s nz=%d%s" % (k, d["edge_kind"][n], col.nz, " paired" if col.paired else "")
        for q in ("ir", "sol", "amean"):
            errs[tag + " " + q] = ref[q] / scale[q]
        if k + "dev_k" in d:
            ks = sorted(set(int(x) for x in d[k + "dev_k"][0]))
            both = XC.oracle_unit_responses(O, col.tau, col.w0, col.g, col.ir_par, ks)
            e_dev = 0.0
            for up, dn in both:
                assert np.all(np.isfinite(up)) and np.all(np.isfinite(dn)), "the oracle is not finite on " + k
                for s in range(2):
                    for j, (kk, db) in enumerate(zip(d[k + "dev_k"][s], d[k + "dev_db"][s])):
                        e = max(np.max(np.abs(db * up[:, kk] - d[k + "dev_up"][s, j])), np.max(np.abs(db * dn[:, kk] - d[k + "dev_dn"][s, j])))
                        e_dev = max(e_dev, float(e / (abs(db) * d[k + "dev_umax"][0])))
            errs[tag + " deviations"] = e_dev
    for m in range(int(d["multi_n"][0])):
        k = "m%02d_" % m
        per_case, finite = XC.multi_ref_errors(O, d, k)
        assert finite, "the oracle is not finite on " + k
        for c, (e_fl, e_am) in enumerate(per_case):
            tag = "%snz=%d nzen=%d case %d" % (k, len(d[k + "tau"]), d[k + "zen_u"].shape[1], c)
            errs[tag + " fluxes"] = e_fl / max(np.max(np.abs(d[k + "fup"][c])), np.max(np.abs(d[k + "fdn"][c])))
            errs[tag + " amean"] = e_am / np.max(np.abs(d[k + "amean"][c]))
    for u in range(int(d["unit_n"][0])):
        k = "u%02d_" % u
        s = max(np.max(np.abs(d[k + "up"])), np.max(np.abs(d[k + "dn"])))
        e = 0.0
        for up, dn in XC.oracle_unit_responses(O, d[k + "tau"], d[k + "w0"], d[k + "g"], d[k + "ir_par"]):
            assert np.all(np.isfinite(up)) and np.all(np.isfinite(dn)), "the oracle is not finite on " + k
            e = max(e, float(max(np.max(np.abs(up - d[k + "up"])), np.max(np.abs(dn - d[k + "dn"]))) / s))
        errs["%snz=%d hard=%d unit matrices" % (k, len(d[k + "tau"]), int(d[k + "ir_par"][1]))] = e
    return errs


def check_conditions(d, O, verbose=False):
    errs = reference_errors(d, O)
    if verbose:
        for k, v in errs.items():
            print("  %-60s %.2e" % (k, v))
    bad = {k: v for k, v in errs.items() if not v <= REF_ERR_MAX}
    assert not bad, "reference true error above %.0e on: %r" % (REF_ERR_MAX, bad)
    return errs


def main():
    from oracle import oracle as O
    O.build()
    out = generate(progress=True)
    errs = check_conditions(out, O, verbose="-v" in sys.argv)
    print("worst reference true error on the new columns: %.2e (%s)" % max((v, k) for k, v in errs.items()))
    for p in glob.glob(os.path.join(HERE, "exact_two_stream_*.npz")):
        os.remove(p)
    for i, part in enumerate(split_parts(out)):
        path = os.path.join(HERE, "exact_two_stream_%d.npz" % i)
        np.savez_compressed(path, **part)
        print("wrote", path, len(part), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
