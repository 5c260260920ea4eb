// ir_opr_sens.inc -- included by kernels.hip (inside namespace clima, after ir_adjoint.inc, whose elimination
// (adjoint_eliminate) it calls, with the row helpers and scans of ir_green.inc) in its first compilation only.
//
// Gradient of a scalar loss on the IR level fluxes with respect to the STORED optical properties tau, w0, g
// (radtran_ir_spectra_opr_vjp), at fixed temperatures.  Per (bin, g-point) two_stream_ir
// (src/radtran/clima_radtran_twostream.f90:156-295) solves M(theta) Y = E(theta, bplanck) and reads a level flux as
// F = c(theta) . Y + s(theta) (ir_adjoint.inc's header has c and s).  For any layer parameter theta
//     dF/dtheta = dc/dtheta . Y + ds/dtheta + lambda . (dE/dtheta - dM/dtheta Y),     M^T lambda = c
// and the adjoint solve is linear in c: ONE solve with the cotangent-weighted sum of the requested functionals' c serves
// any number of levels.  A layer's tau, w0, g reach the system through its e1..e4 and its source terms cp0, cpb, cm0, cmb
// (and, without a hard surface, the bottom layer's tau through Ssfc) -- nine intermediates that sit on the four interface
// rows of the layer alone (rows 2n-1 .. 2n+2; with the virtual layers of ir_green.inc rows 0 and 2nz-1 are interface rows
// like the others).  So the last step is a reverse sweep of ONE layer: the adjoints of e1..e4 and of the source slope from
// lambda, Y and the direct terms, then back through Gamma, exp(-lambda tau), lambda, gam1, gam2 and 1/(gam1+gam2).
//
// k_opr_adjoint: one wave per q = (bin, g-point), lane = row (64 at a time), then lane = layer.
//   1. the transposed system's rows and their elimination: adjoint_eliminate (c', 1 / pivot, D(r-1) -> work rows).
//   2. the combined right-hand side  sum over a, direction of cotangent(bin, a) x that functional's two non-zeros, and
//      lambda by k_adjoint_rows' two affine scans.
//   3. the forward solution Y of M Y = E(bplanck) from the factors already held: M^T = L' U' (L' = pivots and D(r-1),
//      U' = unit upper with c'), so M = U'^T L'^T:  z_r = E_r - c'_{r-1} z_{r-1} downwards, Y_r = (z_r - D(r) Y_{r+1}) /
//      pivot_r upwards -- two more affine scans (affine_scan), no second elimination.
//   4. lane = layer n: the reverse sweep above; wbin(g) x the result -> grad_tau / grad_w0 (n, g, bin) and the g-point's
//      part of grad_g.
// k_opr_sum_g adds the g-points of grad_g in g order (bitwise repeatable, no atomics).
// Three forms differ from the forward kernels' on purpose (opr_layer_of and step 4 say why): lambda is 2 sqrt((1 - w0)
// (1 - w0 g)) -- gam1 - gam2 = 2 (1 - w0) and gam1 + gam2 = 2 (1 - w0 g) hold exactly -- not sqrt(gam1^2 - gam2^2); e2 and
// e4 come from 1 - Gamma and 1 - x; and the adjoint of the source slope is taken from the adjoint equation, not summed.
// The derivative is that of the function, a thin layer (tau <= ir_tau_min) inside its thin branch.
// Levels, layers, rows and k are TOA-first as in ir_green.inc; the cotangents' levels arrive TOA-first (0..nz).

struct OprLayer {
  E4 e;
  double G, x, lam, rgl, rq, tau, dm, sp;    // Gamma, exp(-lambda tau), lambda, 1 / (gam1 + lambda), 1 / (gam1 + gam2), gam1 -+ gam2
  double sig;                                // e2 + e4 = (1 + Gamma)(1 - x)
  double cp0, cpb, cm0, cmb, b1;             // source terms (opr_source), the slope of the source
  bool thin, real;
};
__device__ __forceinline__ OprLayer opr_layer_of(const GreenParams &p, double tau, double w0, double gt, int n, double Rsfc) {
  OprLayer L;
  L.sig = 0.0; L.G = 0.0; L.x = 0.0; L.lam = 1.0; L.rgl = 0.0; L.rq = 0.0; L.tau = 1.0; L.dm = 0.0; L.sp = 0.0;
  L.cp0 = 0.0; L.cpb = 0.0; L.cm0 = 0.0; L.cmb = 0.0; L.b1 = 0.0; L.thin = true; L.real = false;
  if (n < 0) { L.e.e1 = 1.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = 0.0; return L; }
  if (n >= p.nz) { L.e.e1 = 0.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = Rsfc; return L; }
  const double gam1 = 2.0 - w0 * (1.0 + gt), gam2 = w0 * (1.0 - gt);
  L.dm = 2.0 * (1.0 - w0); L.sp = 2.0 * (1.0 - w0 * gt);
  L.lam = sqrt_nr(L.dm * L.sp);
  L.rgl = rcp_nr(gam1 + L.lam);
  L.G = gam2 * L.rgl;
  L.x = fast_exp(-L.lam * tau);
  // e2 = 1 - G x and e4 = G - x from 1 - G = (gam1 - gam2 + lambda) / (gam1 + lambda) and 1 - x = -expm1(-lambda tau): next to
  // w0 = 1 (G -> 1) and in a thin layer (x -> 1) the plain forms cancel
  const double omG = (L.dm + L.lam) * L.rgl, omx = -expm1(-L.lam * tau);
  L.e.e1 = 1.0 + L.G * L.x; L.e.e2 = omG + L.G * omx; L.e.e3 = L.G + L.x; L.e.e4 = omx - omG;
  L.sig = (1.0 + L.G) * omx;
  L.rq = rcp_nr(L.sp);
  L.tau = tau;
  L.thin = tau <= p.ir_tau_min;
  L.real = true;
  return L;
}
// the layer's source terms (:215-234) from the Planck values at its top (B0) and its bottom (B1)
__device__ __forceinline__ void opr_source(OprLayer &L, double B0, double B1) {
  if (!L.real) return;
  double b0 = B0, b1 = 0.0;
  if (L.thin) b0 = 0.5 * (B0 + B1);
  else b1 = (B1 - B0) / L.tau;
  L.b1 = b1;
  L.cp0 = PI * (b0 + b1 * L.rq);
  L.cpb = PI * (b0 + b1 * (L.tau + L.rq));
  L.cm0 = PI * (b0 - b1 * L.rq);
  L.cmb = PI * (b0 + b1 * (L.tau - L.rq));
}

__global__ __launch_bounds__(64) void k_opr_adjoint(IrOprParams p) {
  const GreenParams &gp = p.g;
  const int q = blockIdx.x, lane = threadIdx.x;
  const int nz = gp.nz, N = 2 * nz, nseg = (N + 63) / 64, nsel = p.nsel;
  const GreenQ Q = green_q(gp, q);
  const size_t qtau = Q.qtau, qg = Q.qg;
  const int bi = Q.bi;
  const bool hard = Q.hard;
  const double emis = Q.emis, w = Q.w;
  double *wk = p.work + (size_t)q * OPR_WORK_ROWS * N;
  double *w_c = wk, *w_rd = wk + N, *w_a = wk + (size_t)2 * N, *w_y = wk + (size_t)3 * N, *w_lam = wk + (size_t)4 * N,
         *w_Y = wk + (size_t)5 * N;
  double *part_g = p.part_g + (size_t)q * nz;
  // the bin's width for the cotangents of the sums over the bins (null: none of them was given)
  const double width = (p.gn_up || p.gn_dn) ? gp.ir_freq[gp.ir_lo + bi] - gp.ir_freq[gp.ir_lo + bi + 1] : 0.0;
  // cotangent of (level lv, direction) of this bin: the requested levels in their order, the spectrum's before the sum's.
  // fdn(level 0) = 0 (:289) takes none.
  auto cot = [&](const int lv, double &cu, double &cd) {
    cu = 0.0; cd = 0.0;
    for (int a = 0; a < nsel; a++) {
      if (p.level[a] != lv) continue;
      const size_t ia = (size_t)(gp.ir_lo + bi) + (size_t)p.gs_ld * a;
      if (p.gs_up) cu = cu + p.gs_up[ia];
      if (p.gn_up) cu = cu + p.gn_up[a] * width;
      if (lv > 0) {
        if (p.gs_dn) cd = cd + p.gs_dn[ia];
        if (p.gn_dn) cd = cd + p.gn_dn[a] * width;
      }
    }
  };
  // no cotangent on this bin: exact zeros, nothing solved
  {
    bool any = false;
    for (int a = 0; a < nsel; a++) {
      const size_t ia = (size_t)(gp.ir_lo + bi) + (size_t)p.gs_ld * a;
      const bool dn_counts = p.level[a] > 0;
      if (p.gs_up && p.gs_up[ia] != 0.0) any = true;
      if (p.gn_up && p.gn_up[a] * width != 0.0) any = true;
      if (dn_counts && p.gs_dn && p.gs_dn[ia] != 0.0) any = true;
      if (dn_counts && p.gn_dn && p.gn_dn[a] * width != 0.0) any = true;
    }
    if (!any) {
      for (int n = lane; n < nz; n += 64) {
        if (p.grad_tau) p.grad_tau[qtau + n] = 0.0;
        if (p.grad_w0) p.grad_w0[qtau + n] = 0.0;
        if (p.grad_g) part_g[n] = 0.0;
      }
      return;
    }
  }
  const double avg_freq = p.bplanck ? 0.0 : 0.5 * (gp.freq[gp.ir_start + gp.ir_lo + bi] + gp.freq[gp.ir_start + gp.ir_lo + bi + 1]);
  auto planck = [&](const int k) {     // the Planck value at level k (clamped: what lies outside is not used)
    const int kc = min(max(k, 0), nz);
    return p.bplanck ? p.bplanck[kc] : planck_fcn(avg_freq, kc < nz ? p.T[nz - 1 - kc] : p.Ts[0]);   // (radiate.f90:65-69: level k is layer nz-1-k)
  };
  auto layer = [&](const int n) {     // layer n, or the virtual layer above / below the column
    const GreenLayerIn in = green_layer_in(gp, Q, n);
    return opr_layer_of(gp, in.tau, in.w0, in.g, n, Q.Rsfc);
  };
  // the surface term (:236-247), the upper source value of the virtual layer under the column; Lb = layer nz-1
  auto surface = [&](const OprLayer &Lb, const double Bs) {
    return hard ? emis * PI * Bs : PI * (Bs + 0.5 * Lb.b1);
  };

  // ---- 1. the transposed system's rows and their elimination, on this file's e's
  adjoint_eliminate(nz, lane, [&](const int n) { return layer(n).e; }, w_c, w_rd, w_a);
  // (c' and D(r-1) are read by the neighbouring lanes from here on)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- 2. lambda of the combined functional: rows 2n, 2n+1 carry (cu e1 + cd e3, cu e2 + cd e4) of level n+1, rows 0, 1
  //         also cu(level 0) (e3, -e4)
  {
    double y_in = 0.0;
    for (int seg = 0; seg < nseg; seg++) {
      const int r = seg * 64 + lane, n = r >> 1;
      const bool on = r < N;
      const double rd = on ? w_rd[r] : 0.0, a = on ? w_a[r] : 0.0;
      double rhs = 0.0;
      if (on) {
        const E4 e = layer(n).e;
        double cu, cd;
        cot(n + 1, cu, cd);
        rhs = (r & 1) ? cu * e.e2 + cd * e.e4 : cu * e.e1 + cd * e.e3;
        if (n == 0) {
          double c0, unused;
          cot(0, c0, unused);
          rhs = rhs + ((r & 1) ? -(c0 * e.e4) : c0 * e.e3);
        }
      }
      const Affine m = affine_scan<false>({rhs * rd, on ? -a * rd : 1.0}, lane);       // y_r = al + be y(last row before this lane's prefix)
      const double y = m.al + m.be * y_in;
      if (on) w_y[r] = y;
      y_in = __shfl(y, 63);
    }
    double lam_in = 0.0;
    for (int seg = nseg - 1; seg >= 0; seg--) {
      const int r = seg * 64 + lane;
      const bool on = r < N;
      const Affine m = affine_scan<true>({on ? w_y[r] : 0.0, on ? -w_c[r] : 1.0}, lane);   // lambda_r = al + be lambda(first row after this lane's suffix)
      const double lm = m.al + m.be * lam_in;
      if (on) w_lam[r] = lm;
      lam_in = __shfl(lm, 0);
    }
  }

  // ---- 3. Y of M Y = E(bplanck) from the same factors
  {
    double z_in = 0.0;
    for (int seg = 0; seg < nseg; seg++) {
      const int r = seg * 64 + lane, n = r >> 1;
      const bool on = r < N;
      double E = 0.0;
      if (on) {
        // the row's two layers: (n-1, n) for an even row, (n, n+1) for an odd one; layer la has levels la, la+1
        const int la = n - 1 + (r & 1);
        OprLayer u = layer(la), v = layer(la + 1);
        const double Bm = planck(la + 1);
        opr_source(u, planck(la), Bm);
        opr_source(v, Bm, planck(la + 2));
        if (la + 1 == nz) v.cp0 = surface(u, Bm);
        E = (r & 1) ? v.e.e2 * (v.cp0 - u.cpb) - v.e.e4 * (v.cm0 - u.cmb) : u.e.e3 * (v.cp0 - u.cpb) + u.e.e1 * (u.cmb - v.cm0);
      }
      // z_r = al + be z(last row before this lane's prefix)
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
      // Y_r = al + be Y(first row after this lane's suffix)
      const Affine m = affine_scan<true>({on ? w_y[r] * rd : 0.0, on ? -an * rd : 1.0}, lane);
      const double Yr = m.al + m.be * Y_in;
      if (on) w_Y[r] = Yr;
      Y_in = __shfl(Yr, 0);
    }
  }
  // (lambda and Y are read by other lanes of this wave from here on)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- 4. lane = layer n: the adjoints of its e1..e4, of its source slope (and of Ssfc), then back to tau, w0, g
  for (int n0 = 0; n0 < nz; n0 += 64) {
    const int n = n0 + lane;
    if (n >= nz) continue;
    OprLayer L = layer(n);
    opr_source(L, planck(n), planck(n + 1));
    const E4 u = layer(n - 1).e, e = L.e, v = layer(n + 1).e;
    auto row = [&](const double *v, const int r) { return (r >= 0 && r < N) ? v[r] : 0.0; };
    const double lo_a = row(w_lam, 2 * n - 1), le_a = row(w_lam, 2 * n), lo_b = row(w_lam, 2 * n + 1), le_b = row(w_lam, 2 * n + 2);
    const double y1 = w_Y[2 * n], y2 = w_Y[2 * n + 1];
    // d (row) / d e_k of the layer on its four rows: the interface above (rows 2n-1, 2n; the layer is the lower one of the
    // pair (u, e)) and the one below (rows 2n+1, 2n+2; the upper one of (e, v)).  Four of the sixteen hold the neighbours'
    // unknowns and the source terms; the interface equations themselves (flux continuity, which Y satisfies) reduce them to
    //   d row(2n-1) / d e2 = e4 y2,  d row(2n-1) / d e4 = -e2 y2,  d row(2n+2) / d e3 = e1 y1,  d row(2n+2) / d e1 = -e3 y1
    // -- single products in place of sums that cancel (next to a thin layer the source terms in them are 1 / tau large)
    const double s14 = lo_a * e.e4 + le_a * u.e1, s23 = lo_b * v.e2 + le_b * e.e3;
    const double s32 = lo_a * e.e2 + le_a * u.e3, s41 = lo_b * v.e4 + le_b * e.e1;
    double Ge1 = -(y1 * (s14 + s23)), Ge2 = y2 * (s14 - s23);
    double Ge3 = y1 * (s32 + s41), Ge4 = y2 * (s41 - s32);
    const double GS = n == nz - 1 ? lo_b : 0.0;      // d (row 2nz-1) / d Ssfc = 1
    // the functionals themselves: level n+1 reads (e1, e2, cpb) up and (e3, e4, cmb) down, level 0 (e3, -e4, cp0) of layer 0
    double cu, cd;
    cot(n + 1, cu, cd);
    Ge1 = Ge1 + cu * y1; Ge2 = Ge2 + cu * y2;
    Ge3 = Ge3 + cd * y1; Ge4 = Ge4 + cd * y2;
    double c0 = 0.0;
    if (n == 0) {
      double unused;
      cot(0, c0, unused);
      Ge3 = Ge3 + c0 * y1; Ge4 = Ge4 - c0 * y2;
    }
    // back through the layer.  Sources (non-thin): d cp0 = d cpb = -s dtau + t drq, d cm0 = d cmb = +s dtau - t drq with
    // s = pi b1 rq / tau, t = pi b1; Ssfc = pi (B + b1 / 2) without a hard surface
    // With Gcp0 = lo_a e2 + le_a u.e3 [+ cu(level 0)], Gcm0 = -lo_a e4 - le_a u.e1, Gcpb = -lo_b v.e2 - le_b e3 + cu and
    // Gcmb = lo_b v.e4 + le_b e1 + cd the adjoints of the four source terms (rows 2n-1 .. 2n+2 and the functionals),
    // H = (Gcp0 + Gcpb) - (Gcm0 + Gcmb), the adjoint of +b1 rq on the four terms, is O(tau^2) in a layer just above
    // ir_tau_min and meets a factor pi dB rq / tau^2: summed as written it is a difference of O(1) numbers, whose
    // rounding that factor blows up.  Column 2n+1 of M^T lambda = c, which lambda satisfies, says
    //   e2 (H - lo_a sig) = sig (le_a u.e3 - lo_b v.e4 - le_b e1 - cd [+ cu(level 0)]),   sig = e2 + e4 = (1 + Gamma)(1 - x)
    // and the right-hand side has the small factor outside
    const double br = (le_a * u.e3 - lo_b * v.e4) - le_b * e.e1 - cd + c0;
    const double H = lo_a * L.sig + (L.sig / e.e2) * br;
    const double t = PI * L.b1, rtau = L.thin ? 0.0 : 1.0 / L.tau;
    double g_tau = -(t * L.rq * rtau) * H;
    if (!hard) g_tau = g_tau - GS * (0.5 * t * rtau);
    const double Grq = t * H;
    const double GG = (Ge1 - Ge2) * L.x + (Ge3 + Ge4);       // adjoint of Gamma
    const double Gx = (Ge1 - Ge2) * L.G + (Ge3 - Ge4);       // ... of exp(-lambda tau)
    g_tau = g_tau - Gx * (L.lam * L.x);
    const double Glam = -(Gx * (L.tau * L.x)) - GG * (L.G * L.rgl);
    const double rlam = 1.0 / L.lam;
    // adjoints of gam1 + gam2 and gam1 - gam2 (lambda^2 = their product, Gamma = gam2 / (gam1 + lambda), rq = 1 / (gam1 + gam2))
    const double Sg = GG * ((1.0 - L.G) * L.rgl) + Glam * (L.dm * rlam) - 2.0 * (Grq * (L.rq * L.rq));
    const double Dg = -(GG * ((1.0 + L.G) * L.rgl)) + Glam * (L.sp * rlam);
    const double w0 = gp.w0[qtau + n], gt = gp.g[qg + n];
    if (p.grad_tau) p.grad_tau[qtau + n] = w * g_tau;
    if (p.grad_w0) p.grad_w0[qtau + n] = w * (-Dg - gt * Sg);
    if (p.grad_g) part_g[n] = w * (-(w0 * Sg));
  }
}

// thread (bin, layer): the g-points of grad_g in g order
__global__ __launch_bounds__(256) void k_opr_sum_g(IrOprParams p) {
  const GreenParams &gp = p.g;
  const int nz = gp.nz, ng = gp.ng;
  const size_t total = (size_t)gp.n_ir * nz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int bi = (int)(i / nz), n = (int)(i - (size_t)bi * nz);
    const double *src = p.part_g + (size_t)bi * ng * nz + n;
    double sum = 0.0;
    for (int g = 0; g < ng; g++) sum = sum + src[(size_t)g * nz];
    p.grad_g[(size_t)(gp.ir_start + gp.ir_lo + bi) * nz + n] = sum;
  }
}

void launch_ir_opr_sens(const IrOprParams &p, hipStream_t s) {
  hipLaunchKernelGGL(k_opr_adjoint, dim3(p.g.NQ), dim3(64), 0, s, p);
  if (p.grad_g) {
    const size_t total = (size_t)p.g.n_ir * p.g.nz;
    hipLaunchKernelGGL(k_opr_sum_g, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, s, p);
  }
}
