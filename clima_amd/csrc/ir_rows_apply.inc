// ir_rows_apply.inc -- included by kernels.hip (inside namespace clima, after ir_adjoint.inc, whose weights it applies)
// in its first compilation only.
//
// IR spectra of many temperature profiles on one set of opacities (radtran_ir_spectra_batch).  At fixed opacities
// two_stream_ir is homogeneously linear in the Planck values of the levels (ir_adjoint.inc's header: M does not see
// bplanck, E and s are linear in it, and there is no other source), so a per-bin level flux is a fixed row of weights
// times Planck values:
//     f(bin, a, c) = sum over j of W(bin, a, j) B(avg_freq(bin), x_c(j))
// W is what launch_ir_adjoint writes with unit amplitudes (base_T == nullptr): (n_ir, nsel, nz+1) per direction, the bin
// fastest, j ground-first (x(0) = T_surface, x(1 + m) = T(m)).  After that one adjoint pass a column costs no solve.
//
// k_rows_apply<NF, CT>: lane = bin.  A wave owns 64 consecutive bins and a tile of CT columns, a block is 4 such waves
// (4 column tiles of the same bins).  The tile's temperatures go through LDS 64 levels at a time and are read back as
// broadcasts; per level each lane loads its NF weights once (coalesced: the bin is fastest), forms B once per column with
// planck_fcn -- the function the IR solves of the single call and of k_twostream_ir_batch use -- and does NF x CT FMAs
// into registers.  The sum of every (bin, a, c) starts at 0.0 and takes j = 0, 1, ... nz in that order whatever NF, CT,
// the grid or ncol are: a column's results do not depend on the other columns, bit for bit, and there are no cross-lane
// operations and no atomics.  Lanes beyond n_ir and waves beyond ncol work on clamped indices and store nothing.
// Functional F of the call is (direction place d = F / nsel, a = F % nsel); a pass takes NF of them from F0 on.
// k_rows_integrate: one thread per (a, direction, c): the bins in ascending order times freq(l) - freq(l+1).

constexpr int ROWS_WAVES = 4;      // waves (column tiles) per block of k_rows_apply
constexpr int ROWS_JCHUNK = 64;    // levels staged in LDS at a time

template <int NF, int CT>
__global__ __launch_bounds__(64 * ROWS_WAVES) void k_rows_apply(IrRowsApplyParams p) {
  __shared__ double sX[ROWS_WAVES][CT][ROWS_JCHUNK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_ir = p.n_ir, nsel = p.nsel, nz = p.nz, nl = nz + 1, ncol = p.ncol;
  const int bin_raw = blockIdx.x * 64 + lane, bin = min(bin_raw, n_ir - 1);
  const int c_first = (blockIdx.y * ROWS_WAVES + wave) * CT;
  const int l = p.l0 + bin;
  const double avg_freq = 0.5 * (p.freq[l] + p.freq[l + 1]);
  const size_t jstride = (size_t)n_ir * nsel;
  const double *wp[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const int F = p.F0 + f, d = F / nsel, a = F - d * nsel;
    wp[f] = (d ? p.w1 : p.w0) + (size_t)bin + (size_t)n_ir * a;
  }
  double acc[NF][CT];
#pragma unroll
  for (int f = 0; f < NF; f++)
#pragma unroll
    for (int c = 0; c < CT; c++) acc[f][c] = 0.0;

  for (int j0 = 0; j0 < nl; j0 += ROWS_JCHUNK) {
    __syncthreads();   // the previous levels' temperatures are no longer read
    {
      const int j = min(j0 + lane, nz);
#pragma unroll
      for (int c = 0; c < CT; c++) {
        const int col = min(c_first + c, ncol - 1);
        sX[wave][c][lane] = j == 0 ? p.Ts[col] : p.T[(size_t)col * nz + (j - 1)];
      }
    }
    __syncthreads();
    const int nj = min(ROWS_JCHUNK, nl - j0);
    for (int jj = 0; jj < nj; jj++) {
      double w[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) w[f] = wp[f][jstride * (size_t)(j0 + jj)];
#pragma unroll
      for (int c = 0; c < CT; c++) {
        const double B = planck_fcn(avg_freq, sX[wave][c][jj]);
#pragma unroll
        for (int f = 0; f < NF; f++) acc[f][c] = __builtin_fma(w[f], B, acc[f][c]);
      }
    }
  }
  if (bin_raw >= n_ir) return;
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const int F = p.F0 + f, d = F / nsel, a = F - d * nsel;
#pragma unroll
    for (int c = 0; c < CT; c++) {
      const int col = c_first + c;
      if (col < ncol) (d ? p.out1 : p.out0)[(size_t)bin + (size_t)n_ir * (a + (size_t)nsel * col)] = acc[f][c];
    }
  }
}

__global__ __launch_bounds__(256) void k_rows_integrate(IrRowsApplyParams p) {
  const int n_ir = p.n_ir, nsel = p.nsel, ndir = p.ndir;
  const size_t total = (size_t)nsel * ndir * p.ncol;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int a = (int)(i % nsel), d = (int)((i / nsel) % ndir);
  const size_t col = i / ((size_t)nsel * ndir);
  double *fn = d ? p.fn1 : p.fn0;
  if (!fn) return;
  const double *src = (d ? p.out1 : p.out0) + (size_t)n_ir * (a + (size_t)nsel * col);
  double sum = 0.0;
  for (int b = 0; b < n_ir; b++) sum = sum + src[b] * (p.ir_freq[p.ir_lo + b] - p.ir_freq[p.ir_lo + b + 1]);
  fn[(size_t)a + (size_t)nsel * col] = sum;
}

// column tile of a launch: decided by the number of columns in flight alone (the results do not depend on it)
int ir_rows_column_tile(int ncol) { return ncol >= 16 ? 4 : 1; }

template <int NF>
static void launch_rows_apply_nf(const IrRowsApplyParams &p, hipStream_t s) {
  const int ct = ir_rows_column_tile(p.ncol);
  const int tiles = (p.ncol + ct - 1) / ct;
  const dim3 grid((unsigned)((p.n_ir + 63) / 64), (unsigned)((tiles + ROWS_WAVES - 1) / ROWS_WAVES));
  if (ct == 4) hipLaunchKernelGGL((k_rows_apply<NF, 4>), grid, dim3(64 * ROWS_WAVES), 0, s, p);
  else hipLaunchKernelGGL((k_rows_apply<NF, 1>), grid, dim3(64 * ROWS_WAVES), 0, s, p);
}

// every functional of the call in passes of 8, 4, 2 or 1, then the sums over the bins where any is asked for
void launch_ir_rows_apply(const IrRowsApplyParams &p0, hipStream_t s) {
  if (p0.ncol < 1 || p0.n_ir < 1) return;
  IrRowsApplyParams p = p0;
  const int nfun = p.nsel * p.ndir;
  for (int F0 = 0; F0 < nfun;) {
    const int rem = nfun - F0;
    p.F0 = F0;
    if (rem >= 8) { launch_rows_apply_nf<8>(p, s); F0 += 8; }
    else if (rem >= 4) { launch_rows_apply_nf<4>(p, s); F0 += 4; }
    else if (rem >= 2) { launch_rows_apply_nf<2>(p, s); F0 += 2; }
    else { launch_rows_apply_nf<1>(p, s); F0 += 1; }
  }
  if (p.fn0 || p.fn1) {
    const size_t total = (size_t)p.nsel * p.ndir * p.ncol;
    hipLaunchKernelGGL(k_rows_integrate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
  }
}
