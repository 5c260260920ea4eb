// solar_batch.inc -- k_twostream_sol_batch: many illumination cases (zenith angles with their weights, surface albedo,
// photon scale factor) on ONE set of stored optical properties (radtran_radiate_solar_batch).  Included by kernels.hip
// in its first compilation only.
//
// The solar counterpart of k_twostream_ir_batch, with the same decomposition: lane q owns layers [q nz/64, (q+1) nz/64),
// a short chunk is padded from the top with zero-thickness slots, L = ceil(nz/64) slots per lane, the g-points of a bin
// are the waves of a block and are summed in g order.  The g-points' sum (chunk_gsum) and the launch rules (batch_waves,
// batch_items_per_block) are kernels.hip's, called by both; the chunk steps below are this kernel's own text, equal to
// k_twostream_ir_batch's up to the last row (there the surface row, here the flux condition in every lane).
//
// In two_stream_solar (src/radtran/clima_radtran_twostream.f90:10-154) the delta-Eddington scaling, gam1, gam2, lambda,
// Gamma, exp(-lambda tau), the e's and the whole matrix above the surface row do not depend on u0 (twostream_p_body
// already sums the angles of a call into one right-hand side because of that).  Shared by the cases, once per (bin,
// g-point) and block: tau', lambda, Gamma, exp(-lambda tau'), the source constants zA / zB / zH, the optical depth above
// the chunk, the chunk's elimination coefficients, its 2x2 map of (Din, Uin) and the suffix products of these maps.
//
// The surface row (:89, :113-117) holds the case's albedo, so it stays OUT of the shared elimination: every chunk, the
// last one included, ends in the flux condition "e1 y1 + e2 y2 - Uin = -C+(tau)", and the surface is what lies under
// the last chunk: an interface of reflectance Rsfc and source Ssfc = Rsfc direct(nz+1).  The reflectance under chunk
// q is then the Moebius image of Rsfc under the product of the maps of the chunks q+1 .. 63,
//     rho_q = (s00 Rsfc + s02) / (s20 Rsfc + s22),
// one evaluation per lane and case where the single call runs a projective scan.  Rsfc = 0 gives the s02 / s22 of the
// IR kernel, Rsfc = 1 is an ordinary value of the map (s20 Rsfc + s22 = 1 - (reflectance from below) Rsfc > 0 while
// w0 <= MAX_W0).
//
// Per case: per zenith angle the attenuation at the chunk's top and down the chunk as a running product, summed with the
// angle's weight into the source sums (twostream_p_body's `zen`); C+/C- from them; the right-hand-side sweeps; the two
// affine wave scans (their multipliers hold rho, so each is a full scan); the level values; the g-point weight; then
// photons_sol * photon_scale_factor * diurnal_fac and amean's unit factors (clima_radtran_radiate.f90:164-179), applied
// to the sum over the g-points as the single call applies them.

// LDS bytes of the instance of nw waves
static size_t solb_lds(int nz, int nw) { return sizeof(double) * (size_t)2 * 3 * nw * ((size_t)nz + 2); }

template <int L, int NW>
__global__ __launch_bounds__(64 * NW, 1) void k_twostream_sol_batch(SolBatchParams p) {
  extern __shared__ __align__(16) double lds[];   // [2 cases][3][NW][nl + 1] weighted level values (+ a dump entry per row)
  __shared__ double s_e2[EXP2_N];
  const int nz = p.nz, ng = p.ng, nl = nz + 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ll = p.sol_lo + (int)blockIdx.x;
  const int l = p.sol_start + ll;
  const int a = (lane * nz) >> 6, b = ((lane + 1) * nz) >> 6, pad = L - (b - a);
  const bool is_toa = lane == 0, is_sfc = lane == 63, empty = pad == L;
  const int c_begin = (int)blockIdx.z * p.cases_per_block;
  const int c_end = min(p.ncase, c_begin + p.cases_per_block);
  const double sqrt3 = 1.7320508075688772;
  if ((int)threadIdx.x < EXP2_N) s_e2[threadIdx.x] = EXP2_TAB[threadIdx.x];
  __syncthreads();
  // the bin's unit factors (radiate.f90:167-180)
  const double photons = p.photons_sol[ll], amf = p.am_f1[ll], amf2 = p.am_f2[ll], amdw = p.am_dw[ll];

  // (the 8-wave form covers ng <= 8 in one group, as in k_twostream_ir_batch)
  for (int g0 = 0; g0 < (NW == 8 ? 1 : ng); g0 += NW) {
  const bool col_on = g0 + wave < ng, last_group = NW == 8 || g0 + NW >= ng;
  const int cg = col_on ? g0 + wave : ng - 1;
  const double wcol = col_on ? p.wbin[cg] : 0.0;
  const double *tauL = p.tau + ((size_t)l * ng + cg) * nz;
  const double *w0L = p.w0 + ((size_t)l * ng + cg) * nz;
  const double *gL = p.g + (size_t)l * nz;

  // ---- what the optical properties alone decide ------------------------------------------
  double G[L], X[L], taup[L], lam2[L], zA[L], zB[L], zH[L];
  double rr[2 * L], ar[2 * L], cc[2 * L], be[2 * L], ga[2 * L];
  double tauc0;
  {
    double tot = 0.0;
#pragma unroll
    for (int t = 0; t < L; t++) {
      const bool real = t >= pad;
      const int i = min(max(a + t - pad, 0), nz - 1);
      const double tau_in = real ? tauL[i] : 0.0, w0_in = real ? w0L[i] : 0.0, gt_in = real ? gL[i] : 0.0;
      // delta-Eddington (:38-40), quadrature coefficients (:43-44), lambda, Gamma (:50-51): twostream_p_body's operations
      taup[t] = tau_in * (1.0 - w0_in * gt_in * gt_in);
      tot = tot + taup[t];
      const double w0p = w0_in * (1.0 - gt_in * gt_in) * rcp_nr(1.0 - w0_in * gt_in * gt_in);
      const double gtp = gt_in * rcp_nr(1.0 + gt_in);
      const double gam1 = sqrt3 * (2.0 - w0p * (1 + gtp)) / 2.0;
      const double gam2 = sqrt3 * w0p * (1.0 - gtp) / 2.0;
      const double lm = sqrt_nr(gam1 * gam1 - gam2 * gam2);
      G[t] = gam2 * rcp_nr(gam1 + lm);
      // a zero-thickness slot has w0' = 0, so its C+/C- vanish whatever lambda^2 - 1/u0^2 is -- as long as that is not 0
      // (its lambda is sqrt(3), u0 may be 1/sqrt(3)): lambda = 0 keeps it at -1/u0^2, and exp(-lambda tau') = 1 as before
      const double lmr = real ? lm : 0.0;
      lam2[t] = lmr * lmr;
      X[t] = exp_tab(-lmr * taup[t], s_e2);  // :56
      const double sa = sqrt3 * gtp;
      zA[t] = gam1 + gam2 + sa;
      zB[t] = sa * (gam2 - gam1);
      zH[t] = 0.5 * w0p;
    }
    tauc0 = wave_shr1(wscan_sum(tot));   // optical depth above the chunk (tauc, :64-67)
    // the chunk's rows, eliminated downward; row 0 is the TOA row (:93-96) in lane 0 and the flux condition
    // "-Din + e1 y1 - e2 y2 = -C-(0)" elsewhere, the last row the flux condition "e1 y1 + e2 y2 - Uin = -C+(tau)" in EVERY
    // lane (the surface row is the case's)
    E4 u = make_e(G[0], X[0]);
    double cp, lp;
    {
      const double A = is_toa ? 0.0 : -1.0;
      const double r = rcp_nr(u.e1);
      rr[0] = r; ar[0] = A * r;
      cp = (-u.e2) * r; lp = A * r;
      cc[0] = cp; ga[0] = lp;
    }
#pragma unroll
    for (int t = 1; t < L; t++) {
      const E4 v = make_e(G[t], X[t]);
      double A = v.e2 * u.e1 - u.e3 * v.e4, B = u.e2 * v.e2 - u.e4 * v.e4, D = v.e1 * v.e4 - v.e2 * v.e3;
      double r = rcp_nr(B - A * cp);
      rr[2 * t - 1] = r; ar[2 * t - 1] = A * r;
      const double cn = D * r, ln = (-A * lp) * r;
      cc[2 * t - 1] = cn; ga[2 * t - 1] = ln;
      A = u.e2 * u.e3 - u.e4 * u.e1; B = u.e1 * v.e1 - u.e3 * v.e3; D = u.e3 * v.e4 - u.e1 * v.e2;
      r = rcp_nr(B - A * cn);
      rr[2 * t] = r; ar[2 * t] = A * r;
      cp = D * r; lp = (-A * ln) * r;
      cc[2 * t] = cp; ga[2 * t] = lp;
      u = v;
    }
    {
      const double r = rcp_nr(u.e2 - u.e1 * cp);
      rr[2 * L - 1] = r; ar[2 * L - 1] = u.e1 * r;
      cc[2 * L - 1] = -r; ga[2 * L - 1] = (-u.e1 * lp) * r;
    }
  }
  // upward sweep of the Uin / Din coefficients (ga holds the l_r of the downward pass on entry)
  {
    double bev = 1.0, gav = 0.0;
#pragma unroll
    for (int r = 2 * L - 1; r >= 0; r--) {
      const double c_ = cc[r], lc = ga[r];
      bev = -c_ * bev; gav = -lc - c_ * gav;
      be[r] = bev; ga[r] = gav;
    }
  }
  // the chunk as a map of (Din, Uin) (a chunk without a real layer is the identity exactly)
  const E4 ea = make_e(G[0], X[0]), eb = make_e(G[L - 1], X[L - 1]);
  const double ea3 = ea.e3, ea4 = ea.e4, eb3 = eb.e3, eb4 = eb.e4;
  const double uD = empty ? 0.0 : ga[0] * ea3 - ga[1] * ea4, uU = empty ? 1.0 : be[0] * ea3 - be[1] * ea4;
  const double dD = empty ? 1.0 : ga[2 * L - 2] * eb3 + ga[2 * L - 1] * eb4, dU = empty ? 0.0 : be[2 * L - 2] * eb3 + be[2 * L - 1] * eb4;
  // suffix products of the chunks' reflectance maps; s = the product over the chunks BELOW this one (the identity under
  // the last): the reflectance under the chunk is its image of Rsfc
  double s00, s02, s20, s22;
  {
    double m00 = uU * dD - uD * dU, m02 = uD, m20 = -dU, m22 = 1.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double r00 = __shfl_down(m00, d), r02 = __shfl_down(m02, d), r20 = __shfl_down(m20, d), r22 = __shfl_down(m22, d);
      if (lane + d < 64) {
        const double n00 = m00 * r00 + m02 * r20, n02 = m00 * r02 + m02 * r22;
        const double n20 = m20 * r00 + m22 * r20, n22 = m20 * r02 + m22 * r22;
        m00 = n00; m02 = n02; m20 = n20; m22 = n22;
      }
    }
    s00 = __shfl_down(m00, 1); s02 = __shfl_down(m02, 1); s20 = __shfl_down(m20, 1); s22 = __shfl_down(m22, 1);
    if (is_sfc) { s00 = 1.0; s02 = 0.0; s20 = 0.0; s22 = 1.0; }
  }

  // ---- the cases ----------------------------------------------------------------------------
  for (int c = c_begin; c < c_end; c++) {
    // the case's angles, albedo and scale: the same addresses for the whole block and nothing writes them while the
    // kernel runs, so these are scalar loads (BoundsPtr)
    const BoundsPtr zq = (BoundsPtr)(p.zen + (size_t)c * 3 * p.nzen);
    const double Rsfc = ((BoundsPtr)(p.albedo + (size_t)c * p.alb_stride))[ll];
    double cp0[L], cm0[L], cpb[L], cmb[L], dir[L], diru[L];
#pragma unroll
    for (int t = 0; t < L; t++) cp0[t] = cm0[t] = cpb[t] = cmb[t] = dir[t] = diru[t] = 0.0;
    // ---- C+/C- and direct beam (:73-87) summed over the case's angles with their weights
    double wsum = 0.0, dir0 = 0.0;
    for (int z = 0; z < p.nzen; z++) {
      const double u0 = zq[z], wz = zq[p.nzen + z], iu = zq[2 * p.nzen + z];
      wsum = wsum + wz;
      dir0 = dir0 + wz * u0;
      const double iu2 = iu * iu, wzu = wz * u0;
      const double kz = -iu * EXP2_PER_E;   // exp(-tau'/u0) = 2^(tau' kz / 256)
      double et = exp_tab_any(tauc0, kz, s_e2);
#pragma unroll
      for (int t = 0; t < L; t++) {
        const double ex = exp_tab_any(taup[t], kz, s_e2);  // :79
        const double R = wz * rcp_n1(lam2[t] - iu2);        // w_z / denom (:80)
        const double sR = __builtin_fma(-zB[t], u0, iu) * R;
        const double etb = et * ex;
        cp0[t] = __builtin_fma(et, R, cp0[t]);
        cpb[t] = __builtin_fma(etb, R, cpb[t]);
        cm0[t] = __builtin_fma(et, sR, cm0[t]);
        cmb[t] = __builtin_fma(etb, sR, cmb[t]);
        dir[t] = __builtin_fma(wzu, etb, dir[t]);   // direct(i+1) = u0 etb (:82)
        diru[t] = __builtin_fma(wz, etb, diru[t]);  // direct(i+1) / u0
        et = etb;
      }
    }
#pragma unroll
    for (int t = 0; t < L; t++) {
      const double a0 = zA[t] * cp0[t], s0 = cm0[t], ab = zA[t] * cpb[t], sb = cmb[t];
      cp0[t] = zH[t] * (a0 - s0); cm0[t] = zH[t] * (a0 + s0);
      cpb[t] = zH[t] * (ab - sb); cmb[t] = zH[t] * (ab + sb);
    }
    const double Ssfc = Rsfc * dir[L - 1];  // :89 (the surface lies under the last lane's last slot)
    // ---- right-hand side: downward, then upward (alpha_r overwrites dd)
    double dd[2 * L];
    const double cp0_top = cp0[0];
    {
      double dpv = (0.0 - cm0[0]) * rr[0];
      dd[0] = dpv;
      E4 u = make_e(G[0], X[0]);
#pragma unroll
      for (int t = 1; t < L; t++) {
        const E4 v = make_e(G[t], X[t]);
        const double E1 = v.e2 * (cp0[t] - cpb[t - 1]) - v.e4 * (cm0[t] - cmb[t - 1]);
        const double dn = E1 * rr[2 * t - 1] - ar[2 * t - 1] * dpv;
        dd[2 * t - 1] = dn;
        const double E2 = u.e3 * (cp0[t] - cpb[t - 1]) + u.e1 * (cmb[t - 1] - cm0[t]);
        dpv = E2 * rr[2 * t] - ar[2 * t] * dn;
        dd[2 * t] = dpv;
        u = v;
      }
      dd[2 * L - 1] = (0.0 - cpb[L - 1]) * rr[2 * L - 1] - ar[2 * L - 1] * dpv;
      double al = 0.0;
#pragma unroll
      for (int r = 2 * L - 1; r >= 0; r--) {
        al = dd[r] - cc[r] * al;
        dd[r] = al;
      }
    }
    const double uS = empty ? 0.0 : dd[0] * ea3 - dd[1] * ea4 + cp0_top;
    const double dS = empty ? 0.0 : dd[2 * L - 2] * eb3 + dd[2 * L - 1] * eb4 + cmb[L - 1];
    // ---- the case's surface: reflectance under every chunk, then the two scans
    const double rho = (s00 * Rsfc + s02) * rcp_nr(s20 * Rsfc + s22);
    const double mm = rcp_nr(1.0 - rho * dU);
    // bottom-up (a prefix scan in lane-reversed order): source seen from above each interface,
    // sig_above_q = (uS + uU mm rho dS) + uU mm sig_below_q, Ssfc under the last chunk
    double sig;
    {
      const double bq = uU * mm;
      double av = uS + bq * rho * dS;
      av = is_sfc ? av + bq * Ssfc : av;
      double sgr = wave_reverse(av), sgb = wave_reverse(bq), unused[WSCAN_STEPS];
      wscan_build(sgr, sgb, unused);
      sig = wave_reverse(wave_shr1(sgr));
      sig = is_sfc ? Ssfc : sig;
    }
    // top-down: diffuse flux entering each chunk from above, Din_{q+1} = sa_q + sb_q Din_q
    double sa = dS + dU * mm * (rho * dS + sig);
    {
      double sb = dD * (1.0 + dU * mm * rho), unused[WSCAN_STEPS];
      wscan_build(sa, sb, unused);
    }
    const double Din = wave_shr1(sa);
    const double Uin = mm * (rho * dS + sig + rho * dD * Din);
    // ---- level fluxes (:143-148), mean intensity (:135-140), g-point weight; consecutive cases alternate the buffers
    const int buf = (c - c_begin) & 1;
    double *sF = lds + (size_t)buf * 3 * NW * (nl + 1);
    double *sFu = sF + (size_t)(0 * NW + wave) * (nl + 1), *sFd = sF + (size_t)(1 * NW + wave) * (nl + 1), *sFa = sF + (size_t)(2 * NW + wave) * (nl + 1);
#pragma unroll
    for (int t = 0; t < L; t++) {
      const int i = a + t - pad;
      const E4 e = make_e(G[t], X[t]);
      const double y1 = dd[2 * t] + be[2 * t] * Uin + ga[2 * t] * Din;
      const double y2 = dd[2 * t + 1] + be[2 * t + 1] * Uin + ga[2 * t + 1] * Din;
      // (no branch per slot: a zero-thickness slot's values go to a dump entry behind the wave's rows)
      const int lv = t >= pad ? i + 1 : nl;
      sFu[lv] = wcol * (y1 * e.e1 + y2 * e.e2 + cpb[t]);
      sFd[lv] = wcol * ((y1 * e.e3 + y2 * e.e4 + cmb[t]) + dir[t]);
      sFa[lv] = wcol * (sqrt3 * (y1 * (e.e1 + e.e3) + y2 * (e.e2 + e.e4) + cpb[t] + cmb[t]) + diru[t]);
      if (t == 0 && is_toa) {   // the column's top (zero-thickness slots above the first real layer hand the fluxes through)
        const double top = (y1 * e.e3 - y2 * e.e4) + cp0_top;
        sFu[0] = wcol * top;
        sFd[0] = wcol * dir0;                    // direct(1) = u0 (:73)
        sFa[0] = wcol * (sqrt3 * top + wsum);    // direct(1) / u0 = 1
      }
    }
    __syncthreads();
    // ---- sum over the g-points in g order (a later group continues the sum the earlier ones stored), then the unit
    //      factors (radiate.f90:167-180) on the whole sum, reversal to ground-first (:140-154)
    const double scale = photons * ((BoundsPtr)p.scale)[c];  // clima_radtran.f90:302
    for (int n = threadIdx.x; n < nl; n += blockDim.x) {
      const size_t o = (size_t)c * p.out_stride + (size_t)ll * nl + (nz - n);
      double fu = 0.0, fd = 0.0, am = 0.0;
      if (g0 > 0) { fu = p.fup[o]; fd = p.fdn[o]; am = p.amean[o]; }
      fu = chunk_gsum<NW>(sF, 0, nl, n, fu); fd = chunk_gsum<NW>(sF, 1, nl, n, fd); am = chunk_gsum<NW>(sF, 2, nl, n, am);
      if (last_group) {
        fu = fu * scale * p.diurnal_fac;
        fd = fd * scale * p.diurnal_fac;
        am = am * scale * p.diurnal_fac;
        am = am * amf;
        am = am * amf2 * amdw;
      }
      p.fup[o] = fu; p.fdn[o] = fd; p.amean[o] = am;
    }
  }
  __syncthreads();   // the next g-point group reuses the staging buffers
  }
}

// The launcher's rule for the cases of a block (tests size their batches by it)
constexpr int SOLB_TILE = 8;
int solar_batch_cases_per_block(int ncase) { return batch_items_per_block(ncase, SOLB_TILE); }

// false when the configuration is outside what the kernel covers: more than 8 layer slots per lane (nz > 512), more
// than MAX_ZEN angles or an LDS image beyond 160 KiB.  force_nw: batch_waves'.
bool launch_twostream_sol_batch(SolBatchParams &p, hipStream_t s, int force_nw) {
  const int lmax = (p.nz + 63) / 64;
  if (lmax > 8 || p.n_sol <= 0 || p.ncase <= 0 || p.ng < 1 || p.nzen < 1 || p.nzen > MAX_ZEN) return false;
  const int nw = batch_waves(lmax, p.ng, force_nw);
  const size_t lds = solb_lds(p.nz, nw);
  constexpr int LDS_MAX = 160 * 1024 - (int)sizeof(double) * EXP2_N;   // (the exp table is static LDS on top)
  if (lds > (size_t)LDS_MAX) return false;
  using Kern = void (*)(SolBatchParams);
  static const Kern kern8[4] = {k_twostream_sol_batch<1, 8>, k_twostream_sol_batch<2, 8>, k_twostream_sol_batch<3, 8>, k_twostream_sol_batch<4, 8>};
  static const Kern kern4[8] = {k_twostream_sol_batch<1, 4>, k_twostream_sol_batch<2, 4>, k_twostream_sol_batch<3, 4>, k_twostream_sol_batch<4, 4>,
                                k_twostream_sol_batch<5, 4>, k_twostream_sol_batch<6, 4>, k_twostream_sol_batch<7, 4>, k_twostream_sol_batch<8, 4>};
  const Kern k = nw == 8 ? kern8[lmax - 1] : kern4[lmax - 1];
  if (!ensure_max_lds((const void *)k, LDS_MAX)) return false;
  p.cases_per_block = solar_batch_cases_per_block(p.ncase);
  const dim3 grid(p.n_sol, 1, (p.ncase + p.cases_per_block - 1) / p.cases_per_block), blk(64 * nw);
  hipLaunchKernelGGL(k, grid, blk, lds, s, p);
  return true;
}
