// ir_adjoint.inc -- included by kernels.hip (inside namespace clima, after ir_green.inc, whose layer and row helpers
// it uses) in its first compilation only.
//
// Rows of the per-bin IR temperature Jacobian (radtran_ir_jacobian_spectral_rows) by the ADJOINT of two_stream_ir
// (src/radtran/clima_radtran_twostream.f90:156-295).  At fixed opacities the solver solves M Y = E, M = tridiag(A, B, D)
// of N = 2 nz rows; M does not see bplanck, E is linear in it, and bplanck(k) reaches the rows of layers k-1 and k only
// (ir_green.inc's header).  A level flux is F = c . Y + s . bplanck with two non-zeros in c (:288-293):
//     fup(level 0)    c = ( e3(0), -e4(0)) on rows 0, 1          s = cp0(0)
//     fup(level n+1)  c = ( e1(n),  e2(n)) on rows 2n, 2n+1      s = cpb(n)
//     fdn(level n+1)  c = ( e3(n),  e4(n)) on rows 2n, 2n+1      s = cmb(n)
//     fdn(level 0)    = 0
// so  dF / d bplanck(k) = lambda . dE/d bplanck(k) + ds/d bplanck(k)  with  M^T lambda = c:  ONE transposed solve per
// (bin, g-point, functional) gives the whole row, however many temperatures there are.  M^T is tridiagonal with
// sub-diagonal D(r-1), diagonal B(r), super-diagonal A(r+1); its pivots are M's.
//
// k_adjoint_rows: one wave per q = (bin, g-point), the rows 64 at a time (lane = row).
//   1. once per q: the rows' coefficients from the layers' e's (green_layer_of, green_row_even / _odd) and the
//      elimination c'_r = A(r+1) / (B(r) - D(r-1) c'_{r-1}) by k_green_factor's scan of 2 x 2 matrices (green_prefix_scan,
//      green_rcp_pivot); c', 1 / pivot and D(r-1) go to the wave's work rows (each lane reads back only what it wrote).
//   2. per functional: y_r = (c_r - D(r-1) y_{r-1}) / pivot_r, an affine scan (affine_scan) downwards from the segment that
//      holds c's two rows (y is 0 above it), then lambda_r = y_r - c'_r lambda_{r+1}, an affine scan upwards.
//   3. lane = level k: the six rows 2k-3 .. 2k+2 of dE/d bplanck(k), formed as k_green_unit forms them, against
//      every functional's lambda, plus ds/d bplanck(k), times the g-point's weight -> part[q][functional][k].
// k_adjoint_sum adds the g-points of a bin in g order (bitwise repeatable, no atomics), multiplies by the Planck
// derivative dB/dT(avg_freq(bin), T_k) -- adjoint_dbdt = planck_dbdt, NOT times the bin's width -- and writes
// out(bin, a, j), the bin fastest, j = nz - k ground-first (x(1) = T_surface).
// Levels, layers, rows and k are TOA-first as in ir_green.inc.  fun[f] = 2 level + (0 up | 1 down), the functionals of
// a requested level side by side: f = a ndir + (its place among the directions asked for).

// Step 1 of k_adjoint_rows, shared with k_opr_adjoint (ir_opr_sens.inc): the transposed system's rows from the layers' e's
// (layer_e(n): those of layer n, or of the virtual layer above / below the column) and their elimination; c', 1 / pivot and
// D(r-1) go to w_c, w_rd, w_a (N = 2 nz doubles each).  One wave, lane = row.
template <class LayerE>
__device__ __forceinline__ void adjoint_eliminate(const int nz, const int lane, LayerE layer_e, double *w_c, double *w_rd, double *w_a) {
  const int N = 2 * nz, nseg = (N + 63) / 64;
  double c_in = 0.0;
  for (int seg = 0; seg < nseg; seg++) {
    const int r = seg * 64 + lane, n = r >> 1;
    const bool on = r < N;
    // row r pairs the layers (n-1, n) when even, (n, n+1) when odd; so do its neighbours r-1, r+1 the other way round
    const E4 ea = layer_e(n - 1), eb = layer_e(n), ec = layer_e(n + 1);
    // (both kinds of row of both pairs, evaluated once for the whole wave as in k_green_factor)
    double Ae1, Be1, De1, Ao1, Bo1, Do1, Ae2, Be2, De2, Ao2, Bo2, Do2;
    green_row_even(ea, eb, Ae1, Be1, De1); green_row_odd(ea, eb, Ao1, Bo1, Do1);
    green_row_even(eb, ec, Ae2, Be2, De2); green_row_odd(eb, ec, Ao2, Bo2, Do2);
    double a = (r & 1) ? De1 : Do1;          // D(r-1)
    double B = (r & 1) ? Bo2 : Be1;          // B(r)
    double s = (r & 1) ? Ae2 : Ao2;          // A(r+1)
    if (r == 0) a = 0.0;
    if (r >= N - 1) s = 0.0;
    if (!on) { a = 0.0; B = 1.0; }
    GreenM P = {0.0, s, -a, B};
    if (!on) { P.m11 = 1.0; P.m12 = 0.0; P.m21 = 0.0; P.m22 = 1.0; }
    const double rd = green_rcp_pivot(green_prefix_scan(P, lane), c_in, a, B, lane);
    const double cp = on ? s * rd : 0.0;
    if (on) { w_c[r] = cp; w_rd[r] = rd; w_a[r] = a; }
    c_in = __shfl(cp, 63);
  }
}

__global__ __launch_bounds__(64) void k_adjoint_rows(IrAdjointParams p) {
  const GreenParams &gp = p.g;
  const int q = blockIdx.x, lane = threadIdx.x;
  const int nz = gp.nz, nl = nz + 1, N = 2 * nz, nseg = (N + 63) / 64, nfun = p.nfun;
  const GreenQ Q = green_q(gp, q);
  double *wk = p.work + (size_t)q * adjoint_work_rows(nfun) * N;
  double *w_c = wk, *w_rd = wk + N, *w_a = wk + (size_t)2 * N, *w_y = wk + (size_t)3 * N, *w_lam = wk + (size_t)4 * N;
  auto layer = [&](const int n) {     // layer n, or the virtual layer above / below the column (green_layer_of)
    const GreenLayerIn in = green_layer_in(gp, Q, n);
    return green_layer_of(gp, in.tau, in.w0, in.g, n, Q.Rsfc);
  };

  // ---- 1. the transposed system's rows and their elimination
  adjoint_eliminate(nz, lane, [&](const int n) { return layer(n).e; }, w_c, w_rd, w_a);

  // ---- 2. per functional: lambda
  for (int f = 0; f < nfun; f++) {
    const int code = p.fun[f], lv = code >> 1, dn = code & 1;
    double *lam = w_lam + (size_t)f * N;
    if (lv == 0 && dn) continue;       // fdn(level 0) = 0 (:289): no solve, the row is written as 0.0 below
    const int n0 = max(lv - 1, 0), r0 = 2 * n0, seg0 = r0 >> 6;
    const E4 e = layer(n0).e;
    const double c0 = lv == 0 ? e.e3 : dn ? e.e3 : e.e1, c1 = lv == 0 ? -e.e4 : dn ? e.e4 : e.e2;
    double y_in = 0.0;
    for (int seg = seg0; seg < nseg; seg++) {
      const int r = seg * 64 + lane;
      const bool on = r < N;
      const double rd = on ? w_rd[r] : 0.0, a = on ? w_a[r] : 0.0;
      const double rhs = r == r0 ? c0 : r == r0 + 1 ? c1 : 0.0;
      const Affine m = affine_scan<false>({rhs * rd, on ? -a * rd : 1.0}, lane);       // y_r = al + be y(last row before this lane's prefix)
      const double y = m.al + m.be * y_in;
      if (on) w_y[r] = y;
      y_in = __shfl(y, 63);
    }
    double lam_in = 0.0;
    for (int seg = nseg - 1; seg >= 0; seg--) {
      const int r = seg * 64 + lane;
      const bool on = r < N;
      const Affine m = affine_scan<true>({(on && seg >= seg0) ? w_y[r] : 0.0, on ? -w_c[r] : 1.0}, lane);   // lambda_r = al + be lambda(first row after this lane's suffix)
      const double lm = m.al + m.be * lam_in;
      if (on) lam[r] = lm;
      lam_in = __shfl(lm, 0);
    }
  }
  // (the lambdas are read by other lanes of this wave from here on)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- 3. lane = level k: dE/d bplanck(k) on its six rows (layers k-2 .. k+1 are slots 0..3, k_green_unit's), the sums
  double *part = p.part + (size_t)q * nfun * nl;
  for (int k0 = 0; k0 < nl; k0 += 64) {
    const int k = k0 + lane;
    if (k > nz) continue;
    GreenLayer Ly[4];
    double cp0[4], cpb[4], cm0[4], cmb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = k - 2 + j;
      Ly[j] = layer(n);
      double b0 = 0.0, b1 = 0.0;     // source rule (:215-227) for a unit bplanck[k]
      if (n >= 0 && n < nz) {
        if (j == 1) { if (Ly[j].thin) b0 = 0.5; else b1 = 1.0 / Ly[j].tau; }                 // layer k-1: its lower value
        if (j == 2) { if (Ly[j].thin) b0 = 0.5; else { b0 = 1.0; b1 = -1.0 / Ly[j].tau; } }  // layer k: its upper value
      }
      cp0[j] = PI * (b0 + b1 * Ly[j].rq);
      cpb[j] = PI * (b0 + b1 * (Ly[j].tau + Ly[j].rq));
      cm0[j] = PI * (b0 - b1 * Ly[j].rq);
      cmb[j] = PI * (b0 + b1 * (Ly[j].tau - Ly[j].rq));
    }
    // the virtual layer under the column carries the surface term as its upper source value (:236-247)
    if (k == nz) cp0[2] = Q.hard ? Q.emis * PI : PI * (1.0 + (Ly[1].thin ? 0.0 : 0.5 / Ly[1].tau));
    if (k == nz - 1 && !Q.hard) cp0[3] = PI * (Ly[2].thin ? 0.0 : -0.5 / Ly[2].tau);
    double E[6];
#pragma unroll
    for (int t = 0; t < 6; t++) {
      const int r = 2 * k - 3 + t, j = t >> 1;
      E[t] = 0.0;
      if (r >= 0 && r < N) {
        const E4 u = Ly[j].e, v = Ly[j + 1].e;
        const double dcp = cp0[j + 1] - cpb[j];
        E[t] = (t & 1) ? u.e3 * dcp + u.e1 * (cmb[j] - cm0[j + 1]) : v.e2 * dcp - v.e4 * (cm0[j + 1] - cmb[j]);
      }
    }
    for (int f = 0; f < nfun; f++) {
      const int code = p.fun[f], lv = code >> 1, dn = code & 1;
      double v = 0.0;
      if (!(lv == 0 && dn)) {
        const double *lam = w_lam + (size_t)f * N;
#pragma unroll
        for (int t = 0; t < 6; t++) {
          const int rc = min(max(2 * k - 3 + t, 0), N - 1);
          v = __builtin_fma(lam[rc], E[t], v);       // (E is 0 on the rows that do not exist)
        }
        // ds / d bplanck(k): level 0 reads cp0 of layer 0, level n+1 cpb / cmb of layer n = lv - 1
        double s = 0.0;
        if (lv == 0) s = k == 0 ? cp0[2] : k == 1 ? cp0[1] : 0.0;
        else if (k == lv - 1) s = dn ? cmb[2] : cpb[2];
        else if (k == lv) s = dn ? cmb[1] : cpb[1];
        v = Q.w * (v + s);
      }
      part[(size_t)f * nl + k] = v;
    }
  }
}

// dB/dT at (avg_freq, T), per Hz, under the name the adjoint family's kernels call it by: ir_green.inc's planck_dbdt
__device__ __forceinline__ double adjoint_dbdt(double avg_freq, double T) { return planck_dbdt(avg_freq, T); }

// thread (bin, functional, k), the bin fastest: the g-points in g order, the amplitude (1 when base_T is null: the
// test hook's unit amplitudes), out_up / out_dn (n_ir, nrow, nz+1) with j = nz - k
__global__ __launch_bounds__(256) void k_adjoint_sum(IrAdjointParams p) {
  const GreenParams &gp = p.g;
  const int nl = gp.nz + 1, ng = gp.ng, n_ir = gp.n_ir, nfun = p.nfun;
  const size_t total = (size_t)n_ir * nfun * nl;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int bi = (int)(i % n_ir), f = (int)((i / n_ir) % nfun), k = (int)(i / ((size_t)n_ir * nfun));
    const double *src = p.part + ((size_t)bi * ng * nfun + f) * nl + k;
    double sum = 0.0;
    for (int g = 0; g < ng; g++) sum = sum + src[(size_t)g * nfun * nl];
    double amp = 1.0;
    if (gp.base_T) {
      const int l = gp.ir_start + gp.ir_lo + bi;
      amp = adjoint_dbdt(0.5 * (gp.freq[l] + gp.freq[l + 1]), gp.base_T[k]);
    }
    const int a = f / p.ndir, which = p.ndir == 2 ? f % 2 : p.dir0;
    double *out = which ? p.out_dn : p.out_up;
    out[(size_t)bi + (size_t)n_ir * (a + (size_t)p.nrow * (gp.nz - k))] = sum * amp;
  }
}

void launch_ir_adjoint(const IrAdjointParams &p, hipStream_t s) {
  const size_t total = (size_t)p.g.n_ir * p.nfun * (p.g.nz + 1);
  hipLaunchKernelGGL(k_adjoint_rows, dim3(p.g.NQ), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_adjoint_sum, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65535)), dim3(256), 0, s, p);
}
