// sol_opr_sens.inc -- included by kernels.hip (inside namespace clima, after ir_opr_sens.inc; it calls ir_adjoint.inc's
// adjoint_eliminate and ir_green.inc's affine_scan) in its first compilation only.
//
// Gradient of a scalar loss on the SOLAR level values fup, fdn, amean with respect to the STORED optical properties tau,
// w0, g and to the surface albedo (radtran_sol_spectra_opr_vjp), under the handle's zenith angles and weights.  Per (bin,
// g-point) two_stream_solar (src/radtran/clima_radtran_twostream.f90:10-154) solves, for zenith angle z,
// M(theta) Y_z = E_z(theta, u0_z, Rsfc) and reads a level value as c(theta) . Y_z + s_z(theta): the rows and the c's are
// those of ir_adjoint.inc's header (the system is two_stream_ir's with other e's), s holds the layer's C+/C- and the direct
// beam direct(k) = u0 exp(-tauc(k) / u0), which adds to fdn, and direct / u0 to amean.  M and c do not depend on u0 and only
// the surface row holds Rsfc (solar_batch.inc), so with the zenith weights w_z, Ybar = sum_z w_z Y_z and M^T lambda = c
//     dL/dtheta = dc/dtheta . Ybar + sum_z w_z ds_z/dtheta + lambda . (sum_z w_z dE_z/dtheta - dM/dtheta Ybar):
// ONE adjoint and ONE forward solve (of M Ybar = sum_z w_z E_z, from the same factors) per (bin, g-point), however many
// angles and levels; the angles are a loop over the layer's source terms and their derivatives.
//
// The layer in the variables the derivative is taken in (sol_layer_of; D = 1 - w0 g^2, the delta-Eddington scaling :38-40
// is part of the function):
//     tau' = tau D,  h = w0'/2 = w0 (1 - g^2) / (2 D),  sa = sqrt(3) g' = sqrt(3) g / (1 + g),
//     dm = gam1 - gam2 = sqrt(3) (1 - w0) / D,  sp = gam1 + gam2 = sqrt(3) (1 - w0 g) / D      (both hold exactly),
//     lambda = sqrt(dm sp),  Gamma = gam2 / (gam1 + lambda),  x = exp(-lambda tau'),  e2, e4 from 1 - Gamma and 1 - x
// (ir_opr_sens.inc's forms), and per angle (iu = 1 / u0, R = 1 / (lambda^2 - iu^2), A = sp + sa, s = iu + sa dm u0)
//     facp / denom = h (A - s) R,  facm / denom = h (A + s) R        (solar_batch.inc's zA, zB, zH)
//     cp0, cm0 = exp(-tauc(n) iu) x these,  cpb, cmb = exp(-(tauc(n) + tau') iu) x these.
//
// k_sol_opr_adjoint: one wave per q = (bin, g-point).
//   0. lane = layer: tauc (prefix sums in segments of 64 with a carry), the sources summed over the angles with their
//      weights and the summed direct beam -> work rows.
//   1. adjoint_eliminate on this file's e's.
//   2. lambda of the combined functional.  amean(level k) = sqrt(3) (fup + fdn) + direct / u0 (:135-140; at the top
//      sqrt(3) fup + 1), so its cotangent folds into the up and down ones before the solve.
//   3. Ybar by two more affine scans.
//   4. lane = layer n, segments from the bottom: the adjoints of e1..e4 as in k_opr_adjoint, of the four source terms from
//      lambda and the functionals, per angle back through facp, facm, denom to h, sa, dm, sp and tau', then through Gamma,
//      exp(-lambda tau'), lambda, and the delta-Eddington chain to tau, w0, g.  A layer's sources carry exp(-tauc(n) / u0)
//      and direct(k) carries tauc(k): the adjoint of tauc(k) belongs to tau' of every layer above k -- an exclusive suffix
//      sum over the layers (affine_scan downwards per segment, the carry from the segments below: a fixed order).
//      The surface row gives d / d Rsfc = lambda(last row) x (the summed total downward flux at the ground); without any
//      scattering that lambda is taken from the upward cotangents alone (step 2 says why).
// k_sol_opr_sum_g adds the g-points of grad_g and of grad_albedo in g order (bitwise repeatable, no atomics).
// Where lambda = 1 / u0 exactly the derivative is unspecified (two_stream_solar divides by lambda^2 - 1 / u0^2 as well).
// Levels, layers, rows are TOA-first; the cotangents' levels arrive TOA-first (0..nz).

struct SolLayer {
  E4 e;
  double G, x, lam, rgl, dm, sp, h, sa, taup, D;
  bool real;
};
__device__ __forceinline__ SolLayer sol_layer_of(int nz, double tau, double w0, double g, int n, double Rsfc) {
  const double sqrt3 = 1.7320508075688772;
  SolLayer L;
  L.G = 0.0; L.x = 0.0; L.lam = 1.0; L.rgl = 0.0; L.dm = 0.0; L.sp = 0.0; L.h = 0.0; L.sa = 0.0; L.taup = 0.0; L.D = 1.0;
  L.real = false;
  if (n < 0) { L.e.e1 = 1.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = 0.0; return L; }
  if (n >= nz) { L.e.e1 = 0.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = Rsfc; return L; }
  L.D = 1.0 - w0 * g * g;
  const double rD = rcp_nr(L.D);
  L.taup = tau * L.D;
  L.h = 0.5 * (w0 * (1.0 - g * g)) * rD;
  L.sa = sqrt3 * g * rcp_nr(1.0 + g);
  L.dm = sqrt3 * (1.0 - w0) * rD;
  L.sp = sqrt3 * (1.0 - w0 * g) * rD;
  L.lam = sqrt_nr(L.dm * L.sp);
  const double gam1 = 0.5 * (L.sp + L.dm), gam2 = 0.5 * (L.sp - L.dm);
  L.rgl = rcp_nr(gam1 + L.lam);
  L.G = gam2 * L.rgl;
  L.x = fast_exp(-L.lam * L.taup);
  // e2 = 1 - G x and e4 = G - x from 1 - G and 1 - x where x >= 1/2 (ir_opr_sens.inc's forms: next to w0 = 1 and in a thin
  // layer the plain ones cancel); below that the plain ones, which make an opaque layer's rows (x = 0) exactly e = (1, 1,
  // G, G): what lies under it is then cut off exactly, as in the forward solve
  const double omG = (L.dm + L.lam) * L.rgl, omx = -expm1(-L.lam * L.taup);
  const bool plain = L.x < 0.5;
  L.e.e1 = 1.0 + L.G * L.x; L.e.e2 = plain ? 1.0 - L.G * L.x : omG + L.G * omx;
  L.e.e3 = L.G + L.x; L.e.e4 = plain ? L.G - L.x : omx - omG;
  L.real = true;
  return L;
}

__global__ __launch_bounds__(64) void k_sol_opr_adjoint(SolOprParams p) {
  const double sqrt3 = 1.7320508075688772;
  const int q = blockIdx.x, lane = threadIdx.x;
  const int nz = p.nz, N = 2 * nz, nseg = (N + 63) / 64, nlseg = (nz + 63) / 64, nsel = p.nsel, nzen = p.nzen;
  const int bi = q / p.ng, gi = q - bi * p.ng;
  const int ll = p.sol_lo + bi, l = p.sol_start + ll;
  const size_t qtau = ((size_t)l * p.ng + gi) * nz, qg = (size_t)l * nz;
  const double w = p.wbin[gi], Rsfc = p.albedo[ll];
  double *wk = p.work + (size_t)q * SOL_OPR_WORK_ROWS * N;
  double *w_c = wk, *w_rd = wk + N, *w_a = wk + (size_t)2 * N, *w_y = wk + (size_t)3 * N, *w_lam = wk + (size_t)4 * N,
         *w_Y = wk + (size_t)5 * N;
  double *s_cp0 = wk + (size_t)6 * N, *s_cpb = s_cp0 + nz, *s_cm0 = wk + (size_t)7 * N, *s_cmb = s_cm0 + nz;
  double *s_tauc = wk + (size_t)8 * N, *s_dir = s_tauc + nz;
  double *part_g = p.part_g + (size_t)q * nz;
  // the call's units: photons_sol x photon scale factor x diurnal_fac on all three, amean's unit factors on top
  const double fs = p.photons_sol[ll] * p.scale, fa = fs * p.am_f1[ll] * p.am_f2[ll] * p.am_dw[ll];
  const double width = (p.gn_up || p.gn_dn) ? p.sol_freq[ll] - p.sol_freq[ll + 1] : 0.0;
  // cotangents of level lv of this bin in the call's units: up, down, amean.  fdn(level 0) = u0 (:144) takes none.
  auto cot = [&](const int lv, double &cu, double &cd, double &ca) {
    cu = 0.0; cd = 0.0; ca = 0.0;
    for (int a = 0; a < nsel; a++) {
      if (p.level[a] != lv) continue;
      const size_t ia = (size_t)ll + (size_t)p.gs_ld * a;
      if (p.gs_up) cu = cu + p.gs_up[ia] * fs;
      if (p.gn_up) cu = cu + (p.gn_up[a] * width) * fs;
      if (p.gs_am) ca = ca + p.gs_am[ia] * fa;
      if (lv > 0) {
        if (p.gs_dn) cd = cd + p.gs_dn[ia] * fs;
        if (p.gn_dn) cd = cd + (p.gn_dn[a] * width) * fs;
      }
    }
  };
  // no cotangent on this bin: exact zeros, nothing solved
  {
    bool any = false;
    for (int a = 0; a < nsel; a++) {
      const size_t ia = (size_t)ll + (size_t)p.gs_ld * a;
      const bool dn_counts = p.level[a] > 0;
      if (p.gs_up && p.gs_up[ia] != 0.0) any = true;
      if (p.gn_up && p.gn_up[a] * width != 0.0) any = true;
      if (p.gs_am && p.gs_am[ia] != 0.0) any = true;
      if (dn_counts && p.gs_dn && p.gs_dn[ia] != 0.0) any = true;
      if (dn_counts && p.gn_dn && p.gn_dn[a] * width != 0.0) any = true;
    }
    if (!any) {
      for (int n = lane; n < nz; n += 64) {
        if (p.grad_tau) p.grad_tau[qtau + n] = 0.0;
        if (p.grad_w0) p.grad_w0[qtau + n] = 0.0;
        if (p.grad_g) part_g[n] = 0.0;
      }
      if (p.grad_albedo && lane == 0) p.part_alb[q] = 0.0;
      return;
    }
  }
  auto layer = [&](const int n) {     // layer n, or the virtual layer above / below the column
    const int nc = min(max(n, 0), nz - 1);
    return sol_layer_of(nz, p.tau[qtau + nc], p.w0[qtau + nc], p.g[qg + nc], n, Rsfc);
  };
  // one angle's source factors of a layer: facp / denom, facm / denom and what their adjoints need
  struct Src { double R, A, s, Sp, Sm; };
  auto src_of = [&](const SolLayer &L, const double u0, const double iu) {
    Src S;
    S.R = 1.0 / (L.dm * L.sp - iu * iu);
    S.A = L.sp + L.sa;
    S.s = iu + L.sa * L.dm * u0;
    S.Sp = L.h * (S.A - S.s) * S.R;
    S.Sm = L.h * (S.A + S.s) * S.R;
    return S;
  };

  // ---- 0. lane = layer: tauc, the summed sources, the summed direct beam at the layer's bottom
  {
    double carry = 0.0;
    for (int sg = 0; sg < nlseg; sg++) {
      const int n = sg * 64 + lane;
      const bool on = n < nz;
      const SolLayer L = layer(on ? n : nz);
      const double incl = wscan_sum(L.taup);
      const double tauc = carry + wave_shr1(incl);
      carry = carry + __shfl(incl, 63);
      double cp0 = 0.0, cpb = 0.0, cm0 = 0.0, cmb = 0.0, dir = 0.0;
      for (int z = 0; z < nzen; z++) {
        const double u0 = p.zen_u[z], wz = p.zen_w[z], iu = p.zen_iu[z];
        const Src S = src_of(L, u0, iu);
        const double et0 = fast_exp(-tauc * iu), etb = et0 * fast_exp(-L.taup * iu);
        cp0 = cp0 + wz * (et0 * S.Sp); cpb = cpb + wz * (etb * S.Sp);
        cm0 = cm0 + wz * (et0 * S.Sm); cmb = cmb + wz * (etb * S.Sm);
        dir = dir + wz * (u0 * etb);
      }
      if (on) { s_cp0[n] = cp0; s_cpb[n] = cpb; s_cm0[n] = cm0; s_cmb[n] = cmb; s_tauc[n] = tauc; s_dir[n] = dir; }
    }
  }

  // ---- 1. the transposed system's rows and their elimination, on this file's e's
  adjoint_eliminate(nz, lane, [&](const int n) { return layer(n).e; }, w_c, w_rd, w_a);
  // (c', D(r-1) and step 0's rows are read by other lanes from here on)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- 2. lambda of the combined functional (k_opr_adjoint's step 2 with amean folded in).  `down`: with the cotangents
  //         of the downward flux; `store`: lambda -> w_lam.  Returns lambda of the last row, the surface's.
  auto lambda_solve = [&](const bool down, const bool store) {
    double y_in = 0.0;
    for (int seg = 0; seg < nseg; seg++) {
      const int r = seg * 64 + lane, n = r >> 1;
      const bool on = r < N;
      const double rd = on ? w_rd[r] : 0.0, a = on ? w_a[r] : 0.0;
      double rhs = 0.0;
      if (on) {
        const E4 e = layer(n).e;
        double cu, cd, ca;
        cot(n + 1, cu, cd, ca);
        cu = cu + sqrt3 * ca; cd = down ? cd + sqrt3 * ca : 0.0;
        rhs = (r & 1) ? cu * e.e2 + cd * e.e4 : cu * e.e1 + cd * e.e3;
        if (n == 0) {
          double c0, unused, a0;
          cot(0, c0, unused, a0);
          c0 = c0 + sqrt3 * a0;
          rhs = rhs + ((r & 1) ? -(c0 * e.e4) : c0 * e.e3);
        }
      }
      const Affine m = affine_scan<false>({rhs * rd, on ? -a * rd : 1.0}, lane);
      const double y = m.al + m.be * y_in;
      if (on) w_y[r] = y;
      y_in = __shfl(y, 63);
    }
    double lam_in = 0.0, last = 0.0;
    for (int seg = nseg - 1; seg >= 0; seg--) {
      const int r = seg * 64 + lane;
      const bool on = r < N;
      const Affine m = affine_scan<true>({on ? w_y[r] : 0.0, on ? -w_c[r] : 1.0}, lane);
      const double lm = m.al + m.be * lam_in;
      if (on && store) w_lam[r] = lm;
      if (seg == nseg - 1) last = __shfl(lm, (N - 1) & 63);
      lam_in = __shfl(lm, 0);
    }
    return last;
  };
  double lam_last = lambda_solve(true, true);
  // A column in which no layer scatters (w0 = 0 throughout: Gamma = 0 and C+ = C- = 0 in every layer) carries the two streams
  // apart: what leaves the surface never turns back, so the downward cotangents do not reach the surface row.  In the
  // unknowns of the system that zero is a sum that cancels (y1 - y2 of every layer), and lambda of the last row comes out as
  // its rounding, 1e-17 of the others.  There the surface's lambda is solved for from the upward cotangents alone: the same
  // number to rounding where they are present, exactly 0 where they are not.
  {
    bool scat = false;
    for (int n = lane; n < nz; n += 64) scat = scat || p.w0[qtau + n] != 0.0;
    if (__ballot(scat) == 0) {
      lam_last = lambda_solve(false, false);
      // (one value of the surface row's lambda from here on: step 4 reads it from w_lam as the last layer's lower row too)
      if (lane == ((N - 1) & 63)) w_lam[N - 1] = lam_last;
    }
  }

  // ---- 3. Ybar of M Ybar = sum_z w_z E_z from the same factors (k_opr_adjoint's step 3 on step 0's sources)
  {
    // the summed sources of layer n; the virtual layer under the column carries Ssfc = Rsfc direct(nz) (:89) as its cp0
    auto src4 = [&](const int n, double &cp0, double &cpb, double &cm0, double &cmb) {
      cp0 = 0.0; cpb = 0.0; cm0 = 0.0; cmb = 0.0;
      if (n >= 0 && n < nz) { cp0 = s_cp0[n]; cpb = s_cpb[n]; cm0 = s_cm0[n]; cmb = s_cmb[n]; }
      else if (n == nz) cp0 = Rsfc * s_dir[nz - 1];
    };
    double z_in = 0.0;
    for (int seg = 0; seg < nseg; seg++) {
      const int r = seg * 64 + lane, n = r >> 1;
      const bool on = r < N;
      double E = 0.0;
      if (on) {
        const int la = n - 1 + (r & 1);
        const E4 u = layer(la).e, v = layer(la + 1).e;
        double ucp0, ucpb, ucm0, ucmb, vcp0, vcpb, vcm0, vcmb;
        src4(la, ucp0, ucpb, ucm0, ucmb);
        src4(la + 1, vcp0, vcpb, vcm0, vcmb);
        E = (r & 1) ? v.e2 * (vcp0 - ucpb) - v.e4 * (vcm0 - ucmb) : u.e3 * (vcp0 - ucpb) + u.e1 * (ucmb - vcm0);
      }
      const Affine m = affine_scan<false>({E, (on && r > 0) ? -w_c[r - 1] : (on ? 0.0 : 1.0)}, lane);
      const double z = m.al + m.be * z_in;
      if (on) w_y[r] = z;
      z_in = __shfl(z, 63);
    }
    double Y_in = 0.0;
    for (int seg = nseg - 1; seg >= 0; seg--) {
      const int r = seg * 64 + lane;
      const bool on = r < N;
      const double rd = on ? w_rd[r] : 0.0, an = (on && r + 1 < N) ? w_a[r + 1] : 0.0;
      const Affine m = affine_scan<true>({on ? w_y[r] * rd : 0.0, on ? -an * rd : 1.0}, lane);
      const double Yr = m.al + m.be * Y_in;
      if (on) w_Y[r] = Yr;
      Y_in = __shfl(Yr, 0);
    }
  }
  // (lambda and Ybar are read by other lanes of this wave from here on)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- 4. lane = layer n, the segments from the bottom: sfx_in = the adjoints of tauc of everything below the segment
  double sfx_in = 0.0;
  for (int sg = nlseg - 1; sg >= 0; sg--) {
    const int n = sg * 64 + lane;
    const bool on = n < nz;
    double Qt = 0.0, g_taup = 0.0, G_h = 0.0, G_sp = 0.0, G_dm = 0.0, G_sa = 0.0;
    SolLayer L = layer(on ? n : nz);
    if (on) {
      const E4 u = layer(n - 1).e, e = L.e, v = layer(n + 1).e;
      auto row = [&](const double *vv, const int r) { return (r >= 0 && r < N) ? vv[r] : 0.0; };
      const double lo_a = row(w_lam, 2 * n - 1), le_a = row(w_lam, 2 * n), lo_b = row(w_lam, 2 * n + 1), le_b = row(w_lam, 2 * n + 2);
      const double y1 = w_Y[2 * n], y2 = w_Y[2 * n + 1];
      // the adjoints of e1..e4 (k_opr_adjoint's step 4: the interface equations, which Ybar satisfies, reduce them)
      const double s14 = lo_a * e.e4 + le_a * u.e1, s23 = lo_b * v.e2 + le_b * e.e3;
      const double s32 = lo_a * e.e2 + le_a * u.e3, s41 = lo_b * v.e4 + le_b * e.e1;
      double Ge1 = -(y1 * (s14 + s23)), Ge2 = y2 * (s14 - s23);
      double Ge3 = y1 * (s32 + s41), Ge4 = y2 * (s41 - s32);
      double cu, cd, ca;
      cot(n + 1, cu, cd, ca);
      const double cuf = cu + sqrt3 * ca, cdf = cd + sqrt3 * ca;
      Ge1 = Ge1 + cuf * y1; Ge2 = Ge2 + cuf * y2;
      Ge3 = Ge3 + cdf * y1; Ge4 = Ge4 + cdf * y2;
      double c0 = 0.0;
      if (n == 0) {
        double unused, a0;
        cot(0, c0, unused, a0);
        c0 = c0 + sqrt3 * a0;
        Ge3 = Ge3 + c0 * y1; Ge4 = Ge4 - c0 * y2;
      }
      // the adjoints of the four source terms (rows 2n-1 .. 2n+2 and the functionals), of one angle's before its weight
      const double Gcp0 = lo_a * e.e2 + le_a * u.e3 + c0, Gcm0 = -(lo_a * e.e4) - le_a * u.e1;
      const double Gcpb = cuf - lo_b * v.e2 - le_b * e.e3, Gcmb = lo_b * v.e4 + le_b * e.e1 + cdf;
      // direct(n+1): fdn and amean / u0 of level n+1, and Ssfc = Rsfc direct(nz) on the last row
      const double Gsfc = n == nz - 1 ? lam_last * Rsfc : 0.0;
      const double tauc = s_tauc[n];
      for (int z = 0; z < nzen; z++) {
        const double u0 = p.zen_u[z], wz = p.zen_w[z], iu = p.zen_iu[z];
        const Src S = src_of(L, u0, iu);
        const double et0 = fast_exp(-tauc * iu), etb = et0 * fast_exp(-L.taup * iu);
        const double gSp = wz * (et0 * Gcp0 + etb * Gcpb), gSm = wz * (et0 * Gcm0 + etb * Gcmb);
        const double gR = (S.A - S.s) * gSp + (S.A + S.s) * gSm;       // adjoint of h R
        G_h = G_h + S.R * gR;
        const double hR = L.h * S.R;
        const double gA = hR * (gSp + gSm), gs = hR * (gSm - gSp), gden = -(hR * S.R * gR);
        G_dm = G_dm + (L.sp * gden + gs * (L.sa * u0));
        G_sp = G_sp + (L.dm * gden + gA);
        G_sa = G_sa + (gA + gs * (L.dm * u0));
        const double below = etb * (S.Sp * Gcpb + S.Sm * Gcmb), above = et0 * (S.Sp * Gcp0 + S.Sm * Gcm0);
        const double gdir = -(wz * etb) * (cd + ca * iu + Gsfc);       // adjoint of tauc(n+1) from direct(n+1)
        g_taup = g_taup - (wz * iu) * below + gdir;
        Qt = Qt - (wz * iu) * (above + below) + gdir;
      }
      // back through Gamma, exp(-lambda tau') and lambda = sqrt(dm sp); gam1, gam2 = (sp +- dm) / 2
      const double GG = (Ge1 - Ge2) * L.x + (Ge3 + Ge4);
      const double Gx = (Ge1 - Ge2) * L.G + (Ge3 - Ge4);
      g_taup = g_taup - Gx * (L.lam * L.x);
      const double Glam = -(Gx * (L.taup * L.x)) - GG * (L.G * L.rgl);
      const double hl = 0.5 / L.lam;
      G_sp = G_sp + 0.5 * (GG * ((1.0 - L.G) * L.rgl)) + Glam * (L.dm * hl);
      G_dm = G_dm - 0.5 * (GG * ((1.0 + L.G) * L.rgl)) + Glam * (L.sp * hl);
      // the surface row: d / d Rsfc of (Ssfc - cpb + Rsfc cmb) - (e1 - Rsfc e3) y1 - (e2 - Rsfc e4) y2
      if (n == nz - 1 && p.grad_albedo) p.part_alb[q] = w * (lam_last * ((y1 * e.e3 + y2 * e.e4) + s_cmb[n] + s_dir[n]));
    }
    // the adjoint of tauc of every level below the layer's top, this layer's bottom included (g_taup holds that part)
    const Affine m = affine_scan<true>({Qt, 1.0}, lane);
    double excl = __shfl_down(m.al, 1);
    if (lane == 63) excl = 0.0;
    g_taup = g_taup + (excl + sfx_in);
    sfx_in = sfx_in + __shfl(m.al, 0);
    if (on) {
      // the delta-Eddington chain: tau' = tau D, h = w0 (1 - g^2) / (2 D), sa = sqrt(3) g / (1 + g), dm = sqrt(3) (1 - w0) / D,
      // sp = sqrt(3) (1 - w0 g) / D, D = 1 - w0 g^2
      const double tau = p.tau[qtau + n], w0 = p.w0[qtau + n], g = p.g[qg + n];
      const double rD = 1.0 / L.D, r1g = 1.0 / (1.0 + g);
      const double G_D = g_taup * tau - (G_h * L.h + G_dm * L.dm + G_sp * L.sp) * rD;
      const double G_w0 = (G_h * (0.5 * (1.0 - g * g)) - sqrt3 * (G_dm + G_sp * g)) * rD - G_D * (g * g);
      const double G_g = G_sa * (sqrt3 * r1g * r1g) - (G_h * (w0 * g) + sqrt3 * (G_sp * w0)) * rD - 2.0 * (G_D * (w0 * g));
      if (p.grad_tau) p.grad_tau[qtau + n] = w * (g_taup * L.D);
      if (p.grad_w0) p.grad_w0[qtau + n] = w * G_w0;
      if (p.grad_g) part_g[n] = w * G_g;
    }
  }
}

// thread (bin, layer): the g-points of grad_g in g order; then thread bin: those of grad_albedo
__global__ __launch_bounds__(256) void k_sol_opr_sum_g(SolOprParams p) {
  const int nz = p.nz, ng = p.ng;
  const size_t n_g = p.grad_g ? (size_t)p.n_sol * nz : 0, total = n_g + (p.grad_albedo ? (size_t)p.n_sol : 0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double sum = 0.0;
    if (i < n_g) {
      const int bi = (int)(i / nz), n = (int)(i - (size_t)bi * nz);
      const double *src = p.part_g + (size_t)bi * ng * nz + n;
      for (int g = 0; g < ng; g++) sum = sum + src[(size_t)g * nz];
      p.grad_g[(size_t)(p.sol_start + p.sol_lo + bi) * nz + n] = sum;
    } else {
      const int bi = (int)(i - n_g);
      const double *src = p.part_alb + (size_t)bi * ng;
      for (int g = 0; g < ng; g++) sum = sum + src[g];
      p.grad_albedo[p.sol_lo + bi] = sum;
    }
  }
}

void launch_sol_opr_sens(const SolOprParams &p, hipStream_t s) {
  hipLaunchKernelGGL(k_sol_opr_adjoint, dim3(p.NQ), dim3(64), 0, s, p);
  const size_t total = (p.grad_g ? (size_t)p.n_sol * p.nz : 0) + (p.grad_albedo ? (size_t)p.n_sol : 0);
  if (total) hipLaunchKernelGGL(k_sol_opr_sum_g, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, s, p);
}
