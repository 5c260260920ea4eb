"""Seeded random sweep of the HIP path against the oracle: table inventories (which opacity
sources exist), g-point counts, layer counts, zenith counts, surface/scalar settings and columns
pushed beyond the table ranges (the clamps of clima_radtran_types.f90:655-656, :910, :937).

Conditioning note.  The IR source slope is b1 = (B_{i+1} - B_i)/tau for every layer with
tau > ir_tau_min (clima_radtran_twostream.f90:216-227), so rounding differences in the Planck
function are amplified by 1/tau, and in thin atmospheres the downward IR flux is itself a small
difference.  With the reference's default ir_tau_min = 1e-6 (clima_radtran.f90:62) GPU and
oracle agree to ~1e-10 or better; pushed down to 1e-9 the difference reaches 7e-7 in one case
here -- and so does the difference between two compilations of the oracle itself (FMA
contraction on / off: oracle/liborc_fma.so vs liborc.so).  That CPU-vs-CPU difference is the
yardstick: flux tolerances are max(stated tolerance, 10 x yardstick); the opacity tolerances
never move.  The per-bin comparison of test_gpu_parity._compare_once (every bin on its own scale) has a
yardstick of its own, the largest per-bin difference of the two compilations: on these 160 seeds at most
1.2e-11 (IR) and 8.2e-13 (solar) wherever ir_tau_min >= 1e-6, up to 1.5e-8 below that.
"""
import numpy as np
import pytest

from test_gpu_parity import _compare, _pair, per_bin_difference

pytestmark = pytest.mark.gpu

ALL_K = ("H2O", "CO2", "O2", "O3", "CH4")
ALL_CIA = (("N2", "N2"), ("O2", "O2"), ("CO2", "CO2"), ("O2", "N2"), ("CH4", "CH4"), ("CO2", "CH4"))
ALL_RAY = ("CO2", "O2", "N2", "CH4", "H2O")


def _case(seed):
    from clima_amd import synthetic as S
    rng = np.random.default_rng(1000 + seed)
    nk = int(rng.integers(1, 6))
    k_species = tuple(rng.permutation(ALL_K)[:nk])
    cia = tuple(ALL_CIA[i] for i in sorted(rng.permutation(len(ALL_CIA))[: int(rng.integers(0, 7))]))
    ray = tuple(ALL_RAY[i] for i in sorted(rng.permutation(len(ALL_RAY))[: int(rng.integers(0, 6))]))
    pxs = tuple(rng.permutation(ALL_K)[: int(rng.integers(0, 6))])
    particles = ("HCaer1",) if rng.random() < 0.5 else ()
    ng = 8 if rng.random() < 0.7 else int(rng.choice([2, 3, 5, 10]))
    tb = S.make_tables(nw=int(rng.integers(6, 20)), ng=ng, k_species=k_species, cia_pairs=cia, ray_species=ray,
                       pxs_species=pxs, particles=particles, water_continuum=bool(rng.random() < 0.6),
                       sorted_k=bool(rng.random() < 0.7), seed=int(rng.integers(1, 10**6)),
                       nP=int(rng.integers(2, 12)), nT=int(rng.integers(2, 12)), nT_cia=int(rng.integers(2, 8)))
    nz = int(rng.choice([1, 2, 4, 7, 16, 33, 64, 90, 128, 129, 192, 200, 256, 300]))
    nzen = int(rng.integers(1, 9))
    col = S.modern_earth_column(nz, n_particles=len(particles))
    # push parts of the column outside the (P, T) table ranges and thin / thicken it
    col["T"] = col["T"] * rng.uniform(0.15, 4.0) if rng.random() < 0.3 else col["T"] + rng.normal(0, 5, nz)
    col["T_surface"] = float(col["T"][0] + rng.uniform(-5, 30))
    scale = 10.0 ** rng.uniform(-3, 1.5)
    col["P"] = col["P"] * scale
    col["densities"] = np.asfortranarray(col["densities"] * scale * 10.0 ** rng.uniform(-1, 1, (1, col["densities"].shape[1])))
    if rng.random() < 0.3:
        col["densities"][:, int(rng.integers(0, col["densities"].shape[1]))] = 0.0
    if particles:
        col["radii"] = np.asfortranarray(col["radii"] * rng.uniform(0.5, 3.0))
        col["pdensities"] = np.asfortranarray(col["pdensities"] * 10.0 ** rng.uniform(-2, 3))
    if nz % 2 == 0 and rng.random() < 0.4:      # pair_reuse pattern
        col = S.doubled_column(S.Column({k: (v[: nz // 2] if isinstance(v, np.ndarray) else v) for k, v in col.items()}))
    scalars = dict(has_hard_surface=bool(rng.random() < 0.7), ir_tau_min=float(10.0 ** rng.uniform(-9, -2)),
                   diurnal_fac=float(rng.uniform(0.25, 1.0)), photon_scale_factor=float(rng.uniform(0.3, 2.0)))
    return tb, nz, nzen, float(rng.uniform(0.0, 0.9)), col, scalars, rng


def _yardstick(O, tb, nz, nzen, albedo, col, scalars, surf):
    """Largest scaled level-flux difference between the two CPU compilations of the oracle, and their largest per-bin
    difference in fup_a / fdn_a / amean, every bin on its own scale."""
    outs, spectra = [], []
    for variant in ("", "fma"):
        o = O.OracleRadtran(tb, nz, nzen, albedo, variant=variant)
        o.set_scalars(**scalars)
        if surf is not None:
            o.set_surface_albedo(surf[0])
            o.set_surface_emissivity(surf[1])
        o.radiate(*col.args())
        outs.append([np.array(x) for x in (o.wrk_ir.fup_n, o.wrk_ir.fdn_n, o.wrk_sol.fup_n, o.wrk_sol.fdn_n, o.f_total)])
        spectra.append([(w.fup_a, w.fdn_a, w.amean) for w in (o.wrk_ir, o.wrk_sol)])
    bin_yard = 0.0
    for (up, dn, am), (up2, dn2, am2) in zip(*spectra):
        bin_yard = max(bin_yard, float(np.max(per_bin_difference(up2, dn2, up, dn))), float(np.max(per_bin_difference(am2, am2, am, am))))
    yard = max(float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(a))), 1e-300)) for a, b in zip(*outs))
    # OLR and ISR are held to a RELATIVE tolerance of their own (test_gpu_parity.RTOL_TOA), and the OLR of a column without
    # a hard surface can be a twentieth of the profile's largest flux: the two compilations' relative difference in those
    # two numbers is part of the yardstick (seed 1288, ir_tau_min 3e-9: 2.0e-9 in OLR where the level rows show 4.8e-10)
    nz = len(outs[0][0]) - 1
    for up, dn in ((0, 1), (2, 3)):
        a = outs[0][dn][nz] - outs[0][up][nz]
        b = outs[1][dn][nz] - outs[1][up][nz]
        if a != 0.0:
            yard = max(yard, abs(a - b) / abs(a))
    return yard, bin_yard


def _seeds():
    """160 seeds in the suite; CLIMA_FUZZ_SEEDS=a:b runs another range (a longer one-off sweep)."""
    import os
    e = os.environ.get("CLIMA_FUZZ_SEEDS")
    if e:
        a, b = (int(x) for x in e.split(":"))
        return range(a, b)
    return range(160)


@pytest.mark.parametrize("seed", _seeds())
def test_random_inventory_and_column(O, seed):
    from test_gpu_parity import TOL_LEVEL
    tb, nz, nzen, albedo, col, scalars, rng = _case(seed)
    r, o = _pair(O, tb, nz, nzen, albedo, **scalars)
    if seed % 2:
        r.coop_items = 0    # odd seeds: the lane-per-item opacity kernel (fused grid where it applies); even: k_opacity_coop where the call is small
    surf = None
    if rng.random() < 0.5:   # per-bin surface arrays
        surf = (rng.uniform(0.0, 1.0, len(tb.sol_wavl) - 1), rng.uniform(0.5, 1.0, len(tb.ir_wavl) - 1))
        r.surface_albedo, r.surface_emissivity = surf
        o.set_surface_albedo(surf[0])
        o.set_surface_emissivity(surf[1])
    yard, bin_yard = _yardstick(O, tb, nz, nzen, albedo, col, scalars, surf)
    _compare(r, o, col, flux_tol_scale=max(1.0, 10.0 * yard / TOL_LEVEL), bin_tol_scale=max(1.0, 10.0 * bin_yard / TOL_LEVEL))


def _green_seeds():
    """40 seeds in the suite; CLIMA_FUZZ_GREEN_SEEDS=a:b runs another range."""
    import os
    e = os.environ.get("CLIMA_FUZZ_GREEN_SEEDS")
    if e:
        a, b = (int(x) for x in e.split(":"))
        return range(a, b)
    return range(40)


@pytest.mark.parametrize("seed", _green_seeds())
def test_random_ir_batches_in_the_response_form(O, seed):
    """radtran_radiate_ir_batch: random inventories, columns and batches -- every column a random number (0-11) of
    random temperature changes of random size on one profile, so sparse and dense columns mix, levels repeat across
    columns and within the top / bottom rows -- in the response form (ir_green.inc).  Held to the oracle's full solves
    with the yardstick of this file (the difference between the oracle's two compilations on the same column sets the
    scale: these columns are badly conditioned on purpose), and the general batch kernel is held to the same."""
    from clima_amd import synthetic as S
    from test_gpu_parity import TOL_LEVEL
    tb, nz, nzen, albedo, col, scalars, rng = _case(5000 + seed)
    if nz < 4:
        pytest.skip("fewer than 4 layers: the response form is not taken")
    r, o = _pair(O, tb, nz, nzen, albedo, **scalars)
    o2 = O.OracleRadtran(tb, nz, nzen, albedo, variant="fma")
    o2.set_scalars(**scalars)
    r.radiate(*col.args())
    o.radiate(*col.args())
    o2.radiate(*col.args())
    ncol = int(rng.integers(2, 40))
    T = np.repeat(np.asarray(col["T"], dtype=float)[:, None], ncol, axis=1)
    Ts = np.full(ncol, float(col["T_surface"]))
    for c in range(ncol):
        for _ in range(int(rng.integers(0, 12))):
            j = int(rng.integers(0, nz + 1))
            d = float(rng.choice([1e-6, 1e-3, 0.1, 3.0, 40.0])) * float(rng.choice([-1.0, 1.0]))
            if j == nz:
                Ts[c] += d
            else:
                T[j, c] = max(T[j, c] + d, 5.0)
    r.ir_green = 0
    gen = r.radiate_ir_batch(Ts, T)
    r.ir_green = 2
    got = r.radiate_ir_batch(Ts, T)
    assert all(np.all(np.isfinite(a)) for a in got)
    for c in sorted(set(int(x) for x in rng.integers(0, ncol, 4))):
        w = S.Column(col)
        w["T"] = T[:, c].copy()
        w["T_surface"] = Ts[c]
        want = []
        for oo in (o, o2):
            oo.radiate(*w.args(), compute_solar=False, compute_opacity=False)
            want.append([np.array(oo.wrk_ir.fup_n), np.array(oo.wrk_ir.fdn_n), np.array(oo.f_total)])
        # the up and down rows of the channel are measured on their common scale, as in test_gpu_parity._compare_once (they
        # come out of one solve as sums of terms of the size of the larger one: seed 2237 of the long sweep has a downward
        # flux of 0.44 under an upward one of 5.4e5, and 1.4e-8 -- 2.6e-14 of the channel's scale -- in both rows)
        ud_scale = max(float(np.max(np.abs(want[0][0]))), float(np.max(np.abs(want[0][1]))), 1e-300)
        for i in range(3):
            scale = ud_scale if i < 2 else max(float(np.max(np.abs(want[0][i]))), 1e-300)
            yard = float(np.max(np.abs(want[0][i] - want[1][i]))) / scale
            tol = max(TOL_LEVEL, 10.0 * yard)
            # ir_tau_min far below the reference's 1e-6 keeps the source slope dB / tau in layers of tau ~ 1e-8; a single
            # changed level is the worst case for it, and there the response form (forced here; the library's own choice
            # leaves such handles to the general kernel) loses digits faster: up to ~50 yardsticks in 800 seeds
            tol_r = tol if scalars["ir_tau_min"] >= 1e-7 else max(TOL_LEVEL, 100.0 * yard)
            assert float(np.max(np.abs(got[i][:, c] - want[0][i]))) / scale <= tol_r, (c, i, "response form")
            assert float(np.max(np.abs(gen[i][:, c] - want[0][i]))) / scale <= 5.0 * tol, (c, i, "general kernel")
