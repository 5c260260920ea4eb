// ir_rows_vjp.inc -- included by kernels.hip (inside namespace clima, after ir_rows_apply.inc, whose forward it
// differentiates, and after ir_adjoint.inc, whose adjoint_dbdt it uses) in its first compilation only.
//
// Temperature gradient of the IR spectra batch (radtran_ir_spectra_batch_vjp).  The forward is
//     f_d(l, a, c) = sum over j of W_d(l, a, j) B(avg_freq(l), x_c(j)),   fn_d(a, c) = sum over l of f_d(l, a, c) dfreq(l)
// with dfreq(l) = freq(l) - freq(l+1), so for cotangents gs_d (of f_d) and gn_d (of fn_d), either of them absent (null):
//     grad_x(j, c) = sum over l of dB/dT(avg_freq(l), x_c(j)) S(l, j, c)
//     S(l, j, c)   = sum over a, then d (up before down), of G_d(l, a, c) W_d(l, a, j)
//     G_d(l, a, c) = gs_d(l, a, c) + gn_d(a, c) dfreq(l)
// No solve and no row of the Jacobian: one dB/dT (adjoint_dbdt: an exp and an expm1) per (bin, level, column).
//
// k_vjp_rows<CT>: lane = bin, in strides of 64.  A wave owns one level j and a tile of CT columns, a block is 4 such waves
// (4 consecutive levels of the same columns, which read the same cotangents).  Per bin a lane loads the level's weights
// once (coalesced: the bin is fastest) and forms S with FMAs from 0.0 in the order (a ascending, up before down), then
// takes it into its partial sum with one FMA, bins ascending.  The 64 partial sums are added by the wave-wide DPP prefix
// sum (wscan_sum: the row_shr / row_bcast schedule, a fixed order) and lane 63 stores.  The order of every addition is a
// function of (n_ir, nsel, ndir) alone: the result for (j, c) is bitwise repeatable and does not depend on ncol, on the
// other columns, on CT or on the grid; no atomics, no LDS.  Lanes beyond n_ir add nothing, waves beyond nz+1 or ncol
// work on clamped indices and store nothing.

constexpr int VJP_WAVES = 4;       // waves (levels) per block of k_vjp_rows

template <int CT>
__global__ __launch_bounds__(64 * VJP_WAVES) void k_vjp_rows(IrRowsVjpParams p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_ir = p.n_ir, nsel = p.nsel, nz = p.nz, ncol = p.ncol, ndir = p.ndir;
  const int j_raw = blockIdx.y * VJP_WAVES + wave, j = min(j_raw, nz);
  const int c_first = blockIdx.x * CT;
  const size_t per_col = (size_t)n_ir * nsel;
  const double *w0 = p.w0 + per_col * j, *w1 = ndir == 2 ? p.w1 + per_col * j : nullptr;
  double x[CT], acc[CT];
  const double *gs0[CT], *gs1[CT], *gn0[CT], *gn1[CT];
#pragma unroll
  for (int c = 0; c < CT; c++) {
    const int col = min(c_first + c, ncol - 1);
    x[c] = j == 0 ? p.Ts[col] : p.T[(size_t)col * nz + (j - 1)];
    acc[c] = 0.0;
    gs0[c] = p.gs0 ? p.gs0 + per_col * col : nullptr;
    gs1[c] = p.gs1 ? p.gs1 + per_col * col : nullptr;
    gn0[c] = p.gn0 ? p.gn0 + (size_t)nsel * col : nullptr;
    gn1[c] = p.gn1 ? p.gn1 + (size_t)nsel * col : nullptr;
  }
  const bool sums = p.gn0 || p.gn1;
  for (int b0 = 0; b0 < n_ir; b0 += 64) {
    const int bin_raw = b0 + lane, bin = min(bin_raw, n_ir - 1);
    const int l = p.l0 + bin;
    const double avg_freq = 0.5 * (p.freq[l] + p.freq[l + 1]);
    const double dfreq = sums ? p.ir_freq[p.ir_lo + bin] - p.ir_freq[p.ir_lo + bin + 1] : 0.0;
    double s[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) s[c] = 0.0;
    for (int a = 0; a < nsel; a++) {
      const size_t at = (size_t)bin + (size_t)n_ir * a;
      const double wa0 = w0[at], wa1 = w1 ? w1[at] : 0.0;
#pragma unroll
      for (int c = 0; c < CT; c++) {
        {
          const double g = gs0[c] ? gs0[c][at] : 0.0;
          const double G = gn0[c] ? __builtin_fma(gn0[c][a], dfreq, g) : g;
          s[c] = __builtin_fma(G, wa0, s[c]);
        }
        if (w1) {
          const double g = gs1[c] ? gs1[c][at] : 0.0;
          const double G = gn1[c] ? __builtin_fma(gn1[c][a], dfreq, g) : g;
          s[c] = __builtin_fma(G, wa1, s[c]);
        }
      }
    }
    if (bin_raw < n_ir) {
#pragma unroll
      for (int c = 0; c < CT; c++) acc[c] = __builtin_fma(s[c], adjoint_dbdt(avg_freq, x[c]), acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < CT; c++) {
    const double total = wscan_sum(acc[c]);      // lane 63: all 64 partial sums, in the schedule's order
    const int col = c_first + c;
    if (lane == 63 && j_raw <= nz && col < ncol) {
      if (j == 0) p.grad_Ts[col] = total;
      else p.grad_T[(size_t)col * nz + (j - 1)] = total;
    }
  }
}

// column tile of a launch: decided by the number of columns in flight alone (the results do not depend on it)
int ir_rows_vjp_column_tile(int ncol) { return ncol >= 16 ? 4 : 1; }

void launch_ir_rows_vjp(const IrRowsVjpParams &p, hipStream_t s) {
  if (p.ncol < 1 || p.n_ir < 1) return;
  const int ct = ir_rows_vjp_column_tile(p.ncol);
  const dim3 grid((unsigned)((p.ncol + ct - 1) / ct), (unsigned)((p.nz + 1 + VJP_WAVES - 1) / VJP_WAVES));
  if (ct == 4) hipLaunchKernelGGL((k_vjp_rows<4>), grid, dim3(64 * VJP_WAVES), 0, s, p);
  else hipLaunchKernelGGL((k_vjp_rows<1>), grid, dim3(64 * VJP_WAVES), 0, s, p);
}
