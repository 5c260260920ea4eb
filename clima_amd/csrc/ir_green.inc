// ir_green.inc -- included by kernels.hip (inside namespace clima, after the device helpers).
//
// The RCE Jacobian's batch as a RESPONSE problem.  With the opacities fixed, two_stream_ir
// (src/radtran/clima_radtran_twostream.f90:156-295) is LINEAR in the Planck values at its nz+1 levels: the
// right-hand side E of the tridiagonal system and the particular terms cp/cm are linear in bplanck, the matrix
// (A, B, D) does not see it.  The Jacobian's columns (src/adiabat/clima_adiabat_solve.f90:798-812) differ from a base
// profile in ONE or a few temperatures each, so
//     F(column c) = F(base) + sum over the deviations (k, T') of c:  R[:, k] * (B(T') - B(T_base,k))        per (bin, g-point)
// where R[:, k] is the response of the level fluxes to a unit change of bplanck[k].  A change of bplanck[k] touches the
// source terms of layers k-1 and k only, i.e. rows ra..rb = 2k-3..2k+2 of E.  With the Thomas elimination written as
//     c'_r = D_r / den_r,  den_r = B_r - A_r c'_{r-1},  d'_r = (E_r - A_r d'_{r-1}) / den_r,  Y_r = d'_r - c'_r Y_{r+1}
// a right-hand side that vanishes outside ra..rb gives
//     below (r >= rb):  Y_r = d'_rb * prod_{m=rb+1..r} phi_m * z_r,   phi_m = -A_m / den_m,  z_r = 1 - c'_r phi_{r+1} z_{r+1}, z_last = 1
//     above (r <= ra):  Y_r = Y_ra * prod_{m=r..ra-1} (-c'_m)
// and the level fluxes (:288-293) follow as  amplitude(k) * [P(level) / P(k)] * factor(level)  with P the running
// products of phi (of -c') down the rows, held as mantissa x 2^exponent (over hundreds of rows the products leave the
// range of a double; their ratios between a deviation and a level do not): the mantissas are folded into the level
// factors and the amplitudes, the exponents meet in an ldexp.  phi, c', z and the level factors depend on the opacities
// alone: one pass per (bin, g-point); a unit response costs a 6-row solve; what is left per (level, deviation, bin,
// g-point) is two FMAs (and one ldexp per 16 levels), where a column of the general batch kernel pays a whole
// right-hand-side sweep and two wave scans per (bin, g-point).  The two levels next to a deviation (and level 0 for
// k <= 1) are evaluated explicitly.
//
// Kernels: k_green_factor (wave per q: elimination, z, running products, level factors), k_green_unit (thread per (k, q):
// unit responses), k_green_local (level factors relative to their block's reference level), k_green_db (Planck
// differences), k_green_accum_far / k_green_accum_mixed (the sums), k_green_combine (columns).  The exact Jacobian
// (radtran_ir_jacobian) is the limit of a step to 0: k_green_dbdt (Planck derivatives) in place of k_green_db, every
// level one deviation, k_green_jacobian (the matrices) in place of k_green_combine.
// Layouts: q = (bin - ir_lo) * ng + g, NQ of them; every array is q-major.  Levels, layers and k are TOA-first as in
// the kernels above (k = nz is the surface); the result rows are ground-first like every level row of the library.

constexpr double GREEN_TINY = 1.0e-300;
constexpr int GREEN_NF = 3;       // explicit levels per deviation: level k, level k+1, level 0 (k <= 1)
// (the work arrays' per-q extents GREEN_RW / IS / FS / DS / D0: radtran_dev.h.  Level 0's explicit values, for k <= 1
// only, sit in D0[q][k][up, down]: as two more rows of DS for every k they were a fifth of what k_green_unit writes)
constexpr int GREEN_TILE = 16;

// gamma1 + gamma2 and the e's of one layer (:195-211).  The first and the last row of the system are the interface rows
// of two VIRTUAL layers: above layer 0 one with e = (1, ., 0, 0), below layer nz-1 one with e = (0, 1, 0, Rsfc) whose
// upper source value is the surface term -- with them every row is one of the two interface equations (:252-276).
struct GreenLayer { E4 e; double rq, tau; bool thin; };
// From the layer's three inputs already in registers (k_green_unit issues the loads of its four layers, and of
// everything else it reads, before the first use: one memory round trip instead of ~20 one behind the other)
__device__ __forceinline__ GreenLayer green_layer_of(const GreenParams &p, double tau, double w0, double gt, int n, double Rsfc) {
  GreenLayer L;
  L.rq = 0.0; L.tau = 0.0; L.thin = true;
  if (n < 0) { L.e.e1 = 1.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = 0.0; return L; }
  if (n >= p.nz) { L.e.e1 = 0.0; L.e.e2 = 1.0; L.e.e3 = 0.0; L.e.e4 = Rsfc; return L; }
  const double gam1 = 2.0 - w0 * (1.0 + gt), gam2 = w0 * (1.0 - gt);
  const double lam = sqrt_nr(gam1 * gam1 - gam2 * gam2);
  const double G = gam2 * rcp_nr(gam1 + lam);
  L.e = make_e(G, fast_exp(-lam * tau));
  L.rq = rcp_nr(gam1 + gam2);
  L.tau = tau;
  L.thin = tau <= p.ir_tau_min;
  return L;
}
// What every kernel of one q = (bin, g-point) starts from: where its layers' tau / w0 (qtau) and g (qg) stand, the bin's
// surface (emis and Rsfc are 0 without a hard surface) and the g-point's weight
struct GreenQ { size_t qtau, qg; int bi, g; bool hard; double emis, Rsfc, w; };
__device__ __forceinline__ GreenQ green_q(const GreenParams &p, int q) {
  GreenQ Q;
  Q.bi = q / p.ng; Q.g = q - Q.bi * p.ng;
  const int l = p.ir_start + p.ir_lo + Q.bi;
  Q.qtau = ((size_t)l * p.ng + Q.g) * p.nz;
  Q.qg = (size_t)l * p.nz;
  Q.hard = p.has_hard_surface != 0;
  Q.emis = Q.hard ? p.emissivity[p.ir_lo + Q.bi] : 0.0; Q.Rsfc = Q.hard ? 1.0 - Q.emis : 0.0;
  Q.w = p.wbin[Q.g];
  return Q;
}
// the three inputs of layer n on clamped indices: a virtual layer (n < 0, n >= nz) loads its neighbour's and uses none
struct GreenLayerIn { double tau, w0, g; };
__device__ __forceinline__ GreenLayerIn green_layer_in(const GreenParams &p, const GreenQ &Q, int n) {
  const int nc = min(max(n, 0), p.nz - 1);
  return {p.tau[Q.qtau + nc], p.w0[Q.qtau + nc], p.g[Q.qg + nc]};
}
// second equation of the interface (u above, v below): row 2n of layer n = v
__device__ __forceinline__ void green_row_even(const E4 &u, const E4 &v, double &A, double &B, double &D) {
  A = u.e2 * u.e3 - u.e4 * u.e1; B = u.e1 * v.e1 - u.e3 * v.e3; D = u.e3 * v.e4 - u.e1 * v.e2;
}
// first equation of the interface (u above, v below): row 2n+1 of layer n = u
__device__ __forceinline__ void green_row_odd(const E4 &u, const E4 &v, double &A, double &B, double &D) {
  A = v.e2 * u.e1 - u.e3 * v.e4; B = u.e2 * v.e2 - u.e4 * v.e4; D = v.e1 * v.e4 - v.e2 * v.e3;
}
// 2 x 2 matrix of the map c -> D / (B - A c) in homogeneous coordinates, scaled by a power of two
struct GreenM { double m11, m12, m21, m22; };
__device__ __forceinline__ void green_norm(GreenM &m) {
  const double big = fmax(fmax(fabs(m.m11), fabs(m.m12)), fmax(fabs(m.m21), fabs(m.m22)));
  if (big > 0.0) {
    const int e = -__builtin_amdgcn_frexp_exp(big);
    m.m11 = __builtin_ldexp(m.m11, e); m.m12 = __builtin_ldexp(m.m12, e);
    m.m21 = __builtin_ldexp(m.m21, e); m.m22 = __builtin_ldexp(m.m22, e);
  }
}
// Inclusive prefix scan of the rows' matrices over the wave's lanes, normalised at every step: lane's P becomes
// P(lane) ... P(1) P(0) (a later row multiplies from the left).  A lane past the last row brings the identity.
__device__ __forceinline__ GreenM green_prefix_scan(GreenM P, const int lane) {
  green_norm(P);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    GreenM T;
    T.m11 = __shfl_up(P.m11, d); T.m12 = __shfl_up(P.m12, d); T.m21 = __shfl_up(P.m21, d); T.m22 = __shfl_up(P.m22, d);
    if (lane >= d) {
      const GreenM o = P;
      P.m11 = o.m11 * T.m11 + o.m12 * T.m21; P.m12 = o.m11 * T.m12 + o.m12 * T.m22;
      P.m21 = o.m21 * T.m11 + o.m22 * T.m21; P.m22 = o.m21 * T.m12 + o.m22 * T.m22;
      green_norm(P);
    }
  }
  return P;
}
// 1 / pivot of this lane's row, B - A c'(row before): c' of every row by the scanned map applied to c_in (c' of the last
// row before the segment), the row before this lane's taken from its neighbour, then the recurrence's own step
__device__ __forceinline__ double green_rcp_pivot(const GreenM &P, const double c_in, const double A, const double B, const int lane) {
  const double c_scan = (P.m11 * c_in + P.m12) / (P.m21 * c_in + P.m22);
  double c_prev = __shfl_up(c_scan, 1);
  if (lane == 0) c_prev = c_in;
  return rcp_nr(B - A * c_prev);
}

// The affine map x -> al + be x, and its inclusive scan over the wave's lanes: upwards in the lane index (DOWN = false)
// lane's map becomes map(lane) o ... o map(0), the whole prefix as a map of what enters lane 0; downwards (DOWN = true)
// map(lane) o ... o map(63), the suffix as a map of what enters lane 63.
struct Affine { double al, be; };
template <bool DOWN>
__device__ __forceinline__ Affine affine_scan(Affine m, const int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double ta = DOWN ? __shfl_down(m.al, d) : __shfl_up(m.al, d), tb = DOWN ? __shfl_down(m.be, d) : __shfl_up(m.be, d);
    if (DOWN ? lane + d < 64 : lane >= d) { m.al = m.al + m.be * ta; m.be = m.be * tb; }
  }
  return m;
}

// dB/dT at (avg_freq, T), per Hz.  With x = h nu / k T and e = exp(-x), dB/dT = K (x / T) e^x / (e^x - 1)^2 =
// K (x / expm1(-x)) (e / expm1(-x)) / T: large x takes e to 0 (no overflow, no NaN), small x keeps its digits through expm1
__device__ __forceinline__ double planck_dbdt(double avg_freq, double T) {
  const double x = ((PLANK * avg_freq) / K_BOLTZ_SI) / T;
  const double K = 1.0e3 * ((2.0 * PLANK * (avg_freq * avg_freq * avg_freq)) / (C_LIGHT * C_LIGHT));
  const double e = exp(-x), em = expm1(-x);
  return K * ((x / em) * (e / em)) / T;
}

// mantissa in +-[0.5, 1) times 2^e (e integral, kept as a double beside the other level / row quantities)
struct GreenX { double m, e; };
__device__ __forceinline__ GreenX green_mul(const GreenX &a, const GreenX &b) {
  const double m = a.m * b.m;
  GreenX r;
  r.m = __builtin_amdgcn_frexp_mant(m);
  r.e = a.e + b.e + (double)__builtin_amdgcn_frexp_exp(m);
  return r;
}
__device__ __forceinline__ GreenX green_mul(const GreenX &a, double f) {
  const double m = a.m * f;
  GreenX r;
  r.m = __builtin_amdgcn_frexp_mant(m);
  r.e = a.e + (double)__builtin_amdgcn_frexp_exp(m);
  return r;
}
__device__ __forceinline__ double green_floor(double x) { return fabs(x) >= GREEN_TINY ? x : (x < 0.0 ? -GREEN_TINY : GREEN_TINY); }
// 2^x for an integral x held as a double (any magnitude: 0 below the range, a large finite value above it)
__device__ __forceinline__ double green_exp2i(double x) { return __builtin_ldexp(1.0, (int)fmin(fmax(x, -3000.0), 1000.0)); }

// 1. everything that depends on the opacities alone: one wave per q, the rows taken 64 at a time (lane = row), first
//    downwards, then upwards.  The elimination c'_r = D_r / (B_r - A_r c'_{r-1}) is a scan of 2 x 2 matrices over the
//    lanes (carried from segment to segment), z_r = 1 - c'_r phi_{r+1} z_{r+1} a scan of affine maps from the bottom,
//    the running products of phi and of -c' multiplicative scans in mantissa x 2^exponent form.
//    Writes RW[q][c', 1/den, z, prod phi (m, e), prod -c' (m, e)][row] and IS[q][e_a, AU, AD, e_b, BU, BD][level]:
//    the above form of level n+1 is (1 / prod_{m < 2n+1} (-c'_m)) x ((-c'_2n) e1 + e2, ... e3 + e4), the below form
//    (prod_{m <= 2n} phi_m) x (z_2n e1 + phi_{2n+1} z_{2n+1} e2, ...), mantissas folded into the factors, exponents beside.
__global__ __launch_bounds__(64) void k_green_factor(GreenParams p) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int nz = p.nz, nl = nz + 1, N = 2 * nz, nseg = (N + 63) / 64;
  const GreenQ Q = green_q(p, q);
  const size_t qtau = Q.qtau, qg = Q.qg;
  const double Rsfc = Q.Rsfc, w = Q.w;
  double *rw = p.RW + (size_t)q * GREEN_RW * N;
  double *is = p.IS + (size_t)q * GREEN_IS * nl;
  // ---- downwards: c', 1/den, phi (kept in z's place until the way back), the running products
  double c_in = 0.0;
  GreenX PLc = {1.0, 0.0}, QLc = {1.0, 0.0};      // products over the rows before the segment
  // (the inputs of a segment's layers are loaded while the segment before it is worked on)
  double nx_tau[2], nx_w0[2], nx_g[2];
  auto load_layers = [&](const int seg) {
    const int r = seg * 64 + lane, la = (r >> 1) - 1 + (r & 1);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const GreenLayerIn in = green_layer_in(p, Q, la + h);
      nx_tau[h] = in.tau; nx_w0[h] = in.w0; nx_g[h] = in.g;
    }
  };
  load_layers(0);
  for (int seg = 0; seg < nseg; seg++) {
    const int r = seg * 64 + lane, n = r >> 1;
    const bool on = r < N;
    double A = 0.0, B = 1.0, D = 0.0;
    {
      // the row's two layers: n - 1, n for an even row, n, n + 1 for an odd one -- evaluated once for the whole wave (as
      // two branches by parity the wave went through four evaluations, a sixth of the kernel's instructions)
      const int la = n - 1 + (r & 1);
      const E4 u = green_layer_of(p, nx_tau[0], nx_w0[0], nx_g[0], la, Rsfc).e, v = green_layer_of(p, nx_tau[1], nx_w0[1], nx_g[1], la + 1, Rsfc).e;
      if (seg + 1 < nseg) load_layers(seg + 1);
      double Ae, Be, De, Ao, Bo, Do;
      green_row_even(u, v, Ae, Be, De);
      green_row_odd(u, v, Ao, Bo, Do);
      if (on) { A = (r & 1) ? Ao : Ae; B = (r & 1) ? Bo : Be; D = (r & 1) ? Do : De; }
    }
    GreenM P = {0.0, D, -A, B};
    if (!on) { P.m11 = 1.0; P.m12 = 0.0; P.m21 = 0.0; P.m22 = 1.0; }
    const double rd = green_rcp_pivot(green_prefix_scan(P, lane), c_in, A, B, lane);
    const double cp = D * rd, ph = -A * rd;
    if (on) { rw[r] = cp; rw[(size_t)N + r] = rd; rw[(size_t)2 * N + r] = ph; }
    c_in = __shfl(cp, 63);
    // products: PL rows 1..r, QL rows < r
    GreenX X = {1.0, 0.0}, Y = {1.0, 0.0};
    X = green_mul(X, (on && r > 0) ? green_floor(ph) : 1.0);
    Y = green_mul(Y, on ? green_floor(-cp) : 1.0);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      GreenX tx, ty;
      tx.m = __shfl_up(X.m, d); tx.e = __shfl_up(X.e, d); ty.m = __shfl_up(Y.m, d); ty.e = __shfl_up(Y.e, d);
      if (lane >= d) { X = green_mul(X, tx); Y = green_mul(Y, ty); }
    }
    const GreenX PL = green_mul(PLc, X);
    GreenX Ye;
    Ye.m = __shfl_up(Y.m, 1); Ye.e = __shfl_up(Y.e, 1);
    if (lane == 0) { Ye.m = 1.0; Ye.e = 0.0; }
    const GreenX QL = green_mul(QLc, Ye);
    if (on) {
      rw[(size_t)3 * N + r] = PL.m; rw[(size_t)4 * N + r] = PL.e;
      rw[(size_t)5 * N + r] = QL.m; rw[(size_t)6 * N + r] = QL.e;
    }
    GreenX t63;
    t63.m = __shfl(PL.m, 63); t63.e = __shfl(PL.e, 63); PLc = t63;
    t63.m = __shfl(Y.m, 63); t63.e = __shfl(Y.e, 63); QLc = green_mul(QLc, t63);
  }
  // ---- upwards: z, and with it the level factors
  double z_in = 1.0, ph_in = 0.0;     // z and phi of the first row of the segment below (phi_N = 0: z_{N-1} = 1)
  // (a segment's seven inputs per lane -- c', phi, the running product of its parity (mantissa, exponent), its layer -- are
  // loaded while the segment below it is worked on; the rows were written on the way down, z overwrites phi in place
  // only behind its own segment's loads)
  double up_cp, up_ph, up_xm, up_xe, up_tau, up_w0, up_g;
  auto load_up = [&](const int seg) {
    const int r = min(seg * 64 + lane, N - 1), nc = min(r >> 1, nz - 1);
    const size_t xrow = (size_t)((r & 1) ? 5 : 3) * N;      // odd rows: product of -c' (above form); even: of phi (below form)
    up_cp = rw[r]; up_ph = rw[(size_t)2 * N + r];
    up_xm = rw[xrow + r]; up_xe = rw[xrow + N + r];
    up_tau = p.tau[qtau + nc]; up_w0 = p.w0[qtau + nc]; up_g = p.g[qg + nc];
  };
  load_up(nseg - 1);
  for (int seg = nseg - 1; seg >= 0; seg--) {
    const int r = seg * 64 + lane, n = r >> 1;
    const bool on = r < N;
    const double cp = on ? up_cp : 0.0, ph = on ? up_ph : 0.0;
    const double xm = up_xm, xe = up_xe;
    const E4 e = green_layer_of(p, up_tau, up_w0, up_g, min(n, nz - 1), Rsfc).e;
    if (seg > 0) load_up(seg - 1);
    double ph_next = __shfl_down(ph, 1);
    if (lane == 63) ph_next = ph_in;
    const double kap = (on && r < N - 1) ? cp * ph_next : 0.0;
    const Affine zm = affine_scan<true>({1.0, -kap}, lane);      // z_r = al + be z(first row after this lane's suffix)
    const double z = zm.al + zm.be * z_in;
    if (on) rw[(size_t)2 * N + r] = z;
    z_in = __shfl(z, 0); ph_in = __shfl(ph, 0);
    // level n+1: its above form sits on row 2n+1 (needs c' of row 2n), its below form on row 2n (needs phi z of row 2n+1)
    const double c_up = __shfl_up(cp, 1), pz_dn = __shfl_down(ph, 1) * __shfl_down(z, 1);
    if (on) {
      const int lv = n + 1;
      if (r & 1) {
        const double qm = xm, qe = xe;
        const double mc = -c_up, wq = w / qm;
        is[0 * nl + lv] = -qe;
        is[1 * nl + lv] = wq * (mc * e.e1 + e.e2);
        is[2 * nl + lv] = wq * (mc * e.e3 + e.e4);
        if (r == 1) {
          is[0] = -qe; is[1 * nl] = wq * (mc * e.e3 - e.e4); is[2 * nl] = 0.0;
          is[3 * nl] = 0.0; is[4 * nl] = 0.0; is[5 * nl] = 0.0;
        }
      } else {
        const double pm = xm, pe = xe;
        const double wp = w * pm;
        is[3 * nl + lv] = pe;
        is[4 * nl + lv] = wp * (z * e.e1 + pz_dn * e.e2);
        is[5 * nl + lv] = wp * (z * e.e3 + pz_dn * e.e4);
      }
    }
  }
}

// 2. unit responses: thread (k, q).  Layers k-2 .. k+1 are slots 0..3 (virtual layers at both ends included); the six
//    rows 2k-3+t, t = 0..5, pair the slots (t/2, t/2+1); those outside 0..N-1 do not exist.
__global__ __launch_bounds__(256) void k_green_unit(GreenParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  const int nz = p.nz, nl = nz + 1, N = 2 * nz;
  if (k > nz) return;
  const GreenQ Q = green_q(p, q);
  const bool hard = Q.hard;
  const double emis = Q.emis, Rsfc = Q.Rsfc;
  GreenLayer Ly[4];
  double cp0[4], cpb[4], cm0[4], cmb[4];
  // every load of the thread up front, on clamped indices (what lies outside is not used)
  const double *rw = p.RW + (size_t)q * GREEN_RW * N;
  double in_tau[4], in_w0[4], in_g[4], rd6[6], cp6[6];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const GreenLayerIn in = green_layer_in(p, Q, k - 2 + j);
    in_tau[j] = in.tau; in_w0[j] = in.w0; in_g[j] = in.g;
  }
#pragma unroll
  for (int t = 0; t < 6; t++) {
    const int rc = min(max(2 * k - 3 + t, 0), N - 1);
    rd6[t] = rw[(size_t)N + rc]; cp6[t] = rw[rc];
  }
  const int ra_c = min(max(2 * k - 3, 0), N - 1), rb_c = min(2 * k + 2, N - 1);
  const double z_last = rw[(size_t)2 * N + rb_c];       // z of the last existing row of the six (min(2k+2, N-1))
  const double in_qlm = rw[(size_t)5 * N + ra_c], in_qle = rw[(size_t)6 * N + ra_c];
  const double in_plm = rw[(size_t)3 * N + rb_c], in_ple = rw[(size_t)4 * N + rb_c];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int n = k - 2 + j;
    Ly[j] = green_layer_of(p, in_tau[j], in_w0[j], in_g[j], n, Rsfc);
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
  if (k == nz) cp0[2] = hard ? emis * PI : PI * (1.0 + (Ly[1].thin ? 0.0 : 0.5 / Ly[1].tau));   // slot 2 = layer nz
  if (k == nz - 1 && !hard) cp0[3] = PI * (Ly[2].thin ? 0.0 : -0.5 / Ly[2].tau);                 // slot 3 = layer nz
  double d[6], Y[6];
  double dprev = 0.0;
#pragma unroll
  for (int t = 0; t < 6; t++) {
    const int r = 2 * k - 3 + t, j = t >> 1;
    d[t] = 0.0;
    if (r >= 0 && r < N) {
      const E4 u = Ly[j].e, v = Ly[j + 1].e;
      const double dcp = cp0[j + 1] - cpb[j];
      double A, B, D, E;
      if (t & 1) { green_row_even(u, v, A, B, D); E = u.e3 * dcp + u.e1 * (cmb[j] - cm0[j + 1]); }
      else { green_row_odd(u, v, A, B, D); E = v.e2 * dcp - v.e4 * (cm0[j + 1] - cmb[j]); }
      dprev = (E - A * dprev) * rd6[t];
      d[t] = dprev;
    }
  }
  double ynext = 0.0;
  bool first = true;
#pragma unroll
  for (int t = 5; t >= 0; t--) {
    const int r = 2 * k - 3 + t;
    Y[t] = 0.0;
    if (r >= 0 && r < N) {
      ynext = first ? d[t] * z_last : d[t] - cp6[t] * ynext;
      first = false;
      Y[t] = ynext;
    }
  }
  const double w = Q.w;
  double *ds = p.DS + (size_t)q * GREEN_DS * nl + k;
  {
    // above: Y(ra) x prod_{m < ra} (-c'_m) against the level's 1 / prod_{m < 2n+1}; below: d'(rb) / prod_{m <= rb} phi_m
    // against the level's prod_{m <= 2n}: amplitude x mantissa here, the exponents meet in the accumulation
    const int ra = 2 * k - 3, rb = 2 * k + 2;
    double aa = 0.0, la = 0.0, ab = 0.0, lb = 0.0;
    if (ra >= 1) { aa = Y[0] * in_qlm; la = -in_qle; }
    if (rb <= N - 1) { ab = d[5] / in_plm; lb = in_ple; }
    // (amplitude, log) side by side: the accumulation kernels take the pair in one 16-byte load
    double *dp = p.DS + (size_t)q * GREEN_DS * nl + 2 * k;
    dp[0] = aa; dp[1] = la; dp[2 * nl] = ab; dp[2 * nl + 1] = lb;
  }
  // explicit levels: k (bottom of layer k-1 = slot 1, rows t = 1, 2), k+1 (slot 2, rows t = 3, 4), level 0 (k <= 1)
  double f[2 * GREEN_NF];
#pragma unroll
  for (int s2 = 0; s2 < 2; s2++) {
    const int j = 1 + s2, n = k - 1 + s2;
    const E4 e = Ly[j].e;
    const bool real = n >= 0 && n < nz;
    f[2 * s2] = real ? w * (Y[1 + 2 * s2] * e.e1 + Y[2 + 2 * s2] * e.e2 + cpb[j]) : 0.0;
    f[2 * s2 + 1] = real ? w * (Y[1 + 2 * s2] * e.e3 + Y[2 + 2 * s2] * e.e4 + cmb[j]) : 0.0;
  }
  {
    // level 0 (:288): layer 0 is slot 2 for k = 0 (rows t = 3, 4) and slot 1 for k = 1 (rows t = 1, 2)
    double v = 0.0;
    if (k == 0) v = w * (Y[3] * Ly[2].e.e3 - Y[4] * Ly[2].e.e4 + cp0[2]);
    if (k == 1) v = w * (Y[1] * Ly[1].e.e3 - Y[2] * Ly[1].e.e4 + cp0[1]);
    f[4] = v; f[5] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) ds[(size_t)(4 + i) * nl] = f[i];
  if (k <= 1) { p.D0[((size_t)q * 2 + k) * 2] = f[4]; p.D0[((size_t)q * 2 + k) * 2 + 1] = f[5]; }
}

// 3. far form, level side: within a block of GREEN_LB levels the factor of a level is taken relative to the block's
//    reference level -- the block's LAST level for the above form (the deviations lie below it), its FIRST for the below
//    form -- so that what is left per (deviation, block) is one exponential: exp(L(ref) - L(k)).  Both pieces are products
//    of |c'| (|phi|) over disjoint consecutive row ranges between the deviation and the level: no overflow.
//    FS[q][form][blk][slot]: slot 0 = L(ref), slot 2 + 2 j = up factor of the block's level j, 3 + 2 j = its down factor.  thread (level, q)
__global__ __launch_bounds__(256) void k_green_local(GreenParams p) {
  const int lv = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  const int nz = p.nz, nl = nz + 1, nblk = (nl + GREEN_LB - 1) / GREEN_LB;
  if (lv >= nblk * GREEN_LB) return;
  const int blk = lv / GREEN_LB, j = lv - blk * GREEN_LB;
  double *fa = p.FS + ((size_t)q * 2 * nblk + blk) * GREEN_FS, *fb = fa + (size_t)nblk * GREEN_FS;
  if (lv >= nl) {   // a short last block: its unused slots are read (and multiplied by amplitudes) all the same
    fa[2 + 2 * j] = 0.0; fa[3 + 2 * j] = 0.0; fb[2 + 2 * j] = 0.0; fb[3 + 2 * j] = 0.0;
    return;
  }
  const double *is = p.IS + (size_t)q * GREEN_IS * nl;
  const int ref_a = min(blk * GREEN_LB + GREEN_LB - 1, nz), ref_b = max(blk * GREEN_LB, 1);
  // (every load before the first store: IS and FS are plain pointers of one parameter block, so a load written behind a
  // store stays behind it -- four memory round trips one after the other)
  const double xra = is[ref_a], xrb = is[3 * nl + ref_b];
  const double la = is[lv], lb = is[3 * nl + lv];
  const double ua = is[1 * nl + lv], da = is[2 * nl + lv], ub = is[4 * nl + lv], db = is[5 * nl + lv];
  const double ea = green_exp2i(la - xra), eb = lv >= 1 ? green_exp2i(lb - xrb) : 0.0;
  fa[2 + 2 * j] = ea * ua;
  fa[3 + 2 * j] = ea * da;
  fb[2 + 2 * j] = eb * ub;
  fb[3 + 2 * j] = eb * db;
  if (j == 0) { fa[0] = xra; fb[0] = xrb; fa[1] = 0.0; fb[1] = 0.0; }
}

// 6. Planck differences of the deviations, times the bin's width (radiate.f90:184-192): DB[bin][dev]
__global__ __launch_bounds__(256) void k_green_db(GreenParams p) {
  const int dev = blockIdx.x * blockDim.x + threadIdx.x, bi = blockIdx.y;
  if (dev >= p.ndev_pad) return;
  double v = 0.0;
  if (dev < p.ndev) {
    const int l = p.ir_start + p.ir_lo + bi, ll = p.ir_lo + bi;
    const double avg_freq = 0.5 * (p.freq[l] + p.freq[l + 1]);
    // B(T1) - B(T0) without the cancellation of two nearly equal Planck values (a Jacobian's step can be 1e-8 T and
    // smaller): 1/(E1 - 1) - 1/(E0 - 1) = E1 expm1(x0 - x1) / ((E1 - 1)(E0 - 1)), E = exp(x), x = h nu / k T
    // (planck_fcn, src/clima_eqns.f90:64-73), and x0 - x1 = (h nu / k) (T1 - T0) / (T0 T1) carries the step itself
    const double T1 = p.dev_T[dev], T0 = p.base_T[p.dev_k[dev]];
    const double hk = (PLANK * avg_freq) / K_BOLTZ_SI;
    const double x1 = hk / T1, x0 = hk / T0;
    if (x0 < 700.0 && x1 < 700.0 && T0 > 0.0 && T1 > 0.0) {
      const double E1 = fast_exp(x1), E0 = fast_exp(x0);
      const double K = 1.0e3 * ((2.0 * PLANK * (avg_freq * avg_freq * avg_freq)) / (C_LIGHT * C_LIGHT));
      v = K * ((E1 * expm1(hk * (T1 - T0) / (T0 * T1))) / ((E1 - 1.0) * (E0 - 1.0)));
    } else {
      v = planck_fcn(avg_freq, T1) - planck_fcn(avg_freq, T0);
    }
    v *= p.ir_freq[ll] - p.ir_freq[ll + 1];
  }
  p.DB[(size_t)bi * p.ndev_pad + dev] = v;
}

// 6'. the exact Jacobian's amplitudes (radtran_ir_jacobian): the Planck DERIVATIVES at the deviations' base temperatures,
//     times the bin's width -- the limit of k_green_db's differences over the step (planck_dbdt).  DB[bin][dev]
__global__ __launch_bounds__(256) void k_green_dbdt(GreenParams p) {
  const int dev = blockIdx.x * blockDim.x + threadIdx.x, bi = blockIdx.y;
  if (dev >= p.ndev_pad) return;
  double v = 0.0;
  if (dev < p.ndev) {
    const int l = p.ir_start + p.ir_lo + bi, ll = p.ir_lo + bi;
    const double avg_freq = 0.5 * (p.freq[l] + p.freq[l + 1]);
    v = planck_dbdt(avg_freq, p.base_T[p.dev_k[dev]]);
    v *= p.ir_freq[ll] - p.ir_freq[ll + 1];
  }
  p.DB[(size_t)bi * p.ndev_pad + dev] = v;
}

// 7a. accumulation, far form: one wave = 64 deviations x one level block x one bin split.  A lane forms its deviation's
//     amplitude once per (bin, g-point) -- one exponential -- and adds it, times the block's 2 x 16 level factors, onto
//     its 32 sums; the level factors are the same for every lane: scalar loads, SGPR operands of the FMAs.
// The level factors of a (bin, g-point, block) -- 34 doubles, the same for every lane -- come in by ONE coalesced vector
// load per wave, a group of GREEN_U g-points ahead of their use, and reach the FMAs through LDS (broadcast reads).
// (As scalar loads straight into SGPR operands the kernel was bound by the scalar cache's few outstanding misses:
// 0.39 ms at 402 layers x 403 columns where the instruction stream needs ~0.12.)
constexpr int GREEN_U = 4;
struct GreenFarIn { double fsv[GREEN_U], d0[GREEN_U], dl[GREEN_U], dbv; };
template <int FORM>
__device__ __forceinline__ void green_far_pass(const GreenParams &p, bool mine, int k, int dev, int blk, int nblk, int b_lo, int b_hi,
                                               double *lds, double (&au)[GREEN_LB], double (&ad)[GREEN_LB]) {
  const int nl = p.nz + 1, ng = p.ng, lane = threadIdx.x;
  const size_t ds_q = (size_t)GREEN_DS * nl, fs_q = (size_t)2 * nblk * GREEN_FS;
  const double *__restrict__ dsa = p.DS + (size_t)(FORM == 1 ? 2 : 0) * nl + 2 * k;
  const double *__restrict__ fs0 = p.FS + (size_t)(FORM * nblk + blk) * GREEN_FS;
  const int gpb = (ng + GREEN_U - 1) / GREEN_U, ngroups = (b_hi - b_lo) * gpb;
  auto load = [&](int t, GreenFarIn &in) {
    const int b = b_lo + t / gpb, g0 = (t % gpb) * GREEN_U;
    in.dbv = mine ? p.DB[(size_t)b * p.ndev_pad + dev] : 0.0;
#pragma unroll
    for (int u = 0; u < GREEN_U; u++) {
      const size_t q = (size_t)b * ng + min(g0 + u, ng - 1);
      in.fsv[u] = lane < GREEN_FS ? fs0[q * fs_q + lane] : 0.0;
      in.d0[u] = dsa[q * ds_q]; in.dl[u] = dsa[q * ds_q + 1];
    }
  };
  // two input sets used in turn (no register copies): while the sums of one group run, the loads of the next are in flight
  auto work = [&](int t, const GreenFarIn &cur) {
    // (one wave per block: its LDS instructions execute in order, so the staging area needs no s_barrier -- and must
    // not have one: __syncthreads() waits for EVERY outstanding load first, the prefetch of the next group included)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < GREEN_FS) {
#pragma unroll
      for (int u = 0; u < GREEN_U; u++) lds[u * GREEN_FS + lane] = cur.fsv[u];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int g0 = (t % gpb) * GREEN_U;
    double a[GREEN_U];
#pragma unroll
    for (int u = 0; u < GREEN_U; u++)   // (no branch: a lane of the other class carries dbv = 0, and 2^min(x, 1000) is finite whatever its x)
      a[u] = cur.dbv * cur.d0[u] * green_exp2i(lds[u * GREEN_FS] - cur.dl[u]);
#pragma unroll
    for (int u = 0; u < GREEN_U; u++) {
      if (g0 + u < ng) {
        const double *fs = lds + u * GREEN_FS;
#pragma unroll
        for (int j = 0; j < GREEN_LB; j++) {
          au[j] = __builtin_fma(fs[2 + 2 * j], a[u], au[j]);
          ad[j] = __builtin_fma(fs[3 + 2 * j], a[u], ad[j]);
        }
      }
    }
  };
  GreenFarIn in0, in1;
  if (ngroups > 0) load(0, in0);
  for (int t = 0; t < ngroups; t += 2) {
    if (t + 1 < ngroups) load(t + 1, in1);
    work(t, in0);
    if (t + 1 < ngroups) {
      if (t + 2 < ngroups) load(t + 2, in0);
      work(t + 1, in1);
    }
  }
}
// Block index -> (deviation group, bin split, level block), XCD-aware: the level blocks of one (group, split) read the
// SAME amplitudes in the same order, and consecutive workgroup ids go round-robin over the 8 XCDs, each with its own L2.
// So a unit u = (group, split) lives on XCD u % 8 and its level blocks take consecutive ids there: they run at the same
// time and what one of them brings into that L2 the others find.
__global__ __launch_bounds__(64) void k_green_accum_far(GreenParams p) {
  const int nz = p.nz, nl = nz + 1, nblk = (nl + GREEN_LB - 1) / GREEN_LB;
  const int ngrp = (p.ndev + 63) / 64, nunit = ngrp * p.qsplit;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int blk = slot % nblk, unit = (slot / nblk) * 8 + xcd;
  if (unit >= nunit) return;
  const int grp = unit % ngrp, split = unit / ngrp;
  const int dev = grp * 64 + threadIdx.x;
  const bool on = dev < p.ndev;
  const int k = on ? p.dev_k[dev] : 0;
  const int cls = on ? green_block_class(k, blk, nz) : 3;
  const int per = (p.n_ir + p.qsplit - 1) / p.qsplit;
  const int b_lo = split * per, b_hi = min(p.n_ir, b_lo + per);
  double au[GREEN_LB], ad[GREEN_LB];
#pragma unroll
  for (int j = 0; j < GREEN_LB; j++) { au[j] = 0.0; ad[j] = 0.0; }
  __shared__ __align__(16) double lds[GREEN_U * GREEN_FS];
  if (__any(cls == 0)) green_far_pass<0>(p, cls == 0, k, min(dev, p.ndev_pad - 1), blk, nblk, b_lo, b_hi, lds, au, ad);
  if (__any(cls == 1)) green_far_pass<1>(p, cls == 1, k, min(dev, p.ndev_pad - 1), blk, nblk, b_lo, b_hi, lds, au, ad);
  if (cls < 2) {
    double *o = p.partial + (((size_t)split * p.ndev_pad + dev) * 2) * nl;
#pragma unroll
    for (int j = 0; j < GREEN_LB; j++) {
      const int lv = blk * GREEN_LB + j;
      if (lv < nl) { o[lv] = au[j]; o[nl + lv] = ad[j]; }
    }
  }
}

// 7a'. the far-form accumulation on the matrix cores.  For one level block and one form the sums are a matrix product
//        S[deviation, level] = sum over q of  amplitude[deviation, q] x factor[q, level]
//     with the amplitude's exponent taken against the block's reference level (so the left operand is FORMED per block,
//     five instructions per element, while the product itself -- 2 x 16 level factors per amplitude -- is
//     v_mfma_f64_16x16x4_f64: 1024 FMAs per instruction, one operand value per lane, where the vector form above feeds
//     every FMA a level factor through LDS).  One wave = up to 64 deviations (four 16-row tiles) x one level block (two
//     16-column tiles: up, down) x one bin split; a K step is four q.  Operand layout of the instruction: A[row, kq] in
//     lane row + 16 kq, B[kq, col] in lane col + 16 kq, D[row = (lane >> 4) + 4 r, col = lane & 15] in register r: the
//     levels are the columns, so a lane's stores of one register run along 16 consecutive levels of a deviation.
//     The deviations are sorted by k, so those that see a given block in the below form are a PREFIX of the list
//     (k <= first level - 2) and those that see it in the above form a SUFFIX (k >= last level + 1, k >= 2): a wave takes
//     64 consecutive deviations of one of the two ranges and is of one form throughout (the earlier cut -- fixed groups
//     of 64, a group around the block running both forms tile by tile -- left those waves three to four times longer
//     than the rest, and the kernel as long as its longest wave).
typedef double green_d4 __attribute__((ext_vector_type(4)));
// A wave takes TWO consecutive level blocks: the deviation-side inputs of a K step -- 16 bytes per (deviation, q), the
// bulk of what the kernel reads -- are loaded once for both, and only the exponent is formed per block.  (With one block
// per wave the loads ran at ~80 % of what a CU's L1 delivers, 64 bytes per clock: 110 us at 402 layers x 403 columns
// where the products alone take 60.)
constexpr int GREEN_NB = 2;
struct GreenMfmaStep { double2 da[4]; double lref[GREEN_NB], fu[GREEN_NB], fd[GREEN_NB]; };
struct GreenMfmaDb { double v[4]; };
// No branch inside a K step: every load is issued whatever the row (a row that does not take the form for a block gets
// the exponent -4000: ldexp(x, -4000) = 0 for any finite x; a row that does has an exponent <= 0), and the steps past
// the end of the split (its length need not be a multiple of four) take level factors of 0.
template <bool NG8>
__device__ __forceinline__ void green_far_pass_mfma(const GreenParams &p, const int form, const bool (&mine)[GREEN_NB][4], const int (&k)[4], int dev0,
                                                    int blk, int nblk, int q_lo, int q_hi, green_d4 (&cu)[GREEN_NB][4], green_d4 (&cd)[GREEN_NB][4]) {
  const int nl = p.nz + 1, ng = p.ng, lane = threadIdx.x, j = lane & 15, kq = lane >> 4;
  const size_t ds_q = (size_t)GREEN_DS * nl, fs_q = (size_t)2 * nblk * GREEN_FS;
  const int nfull = (q_hi - q_lo) >> 2, rest = (q_hi - q_lo) & 3;
  const unsigned ng_inv = 0xffffffffu / (unsigned)ng + 1u;
  const int fs_b1 = blk + 1 < nblk ? GREEN_FS : 0;      // the second block's row sits right behind the first one's (the last block of an odd count: itself again, unused)
  // this lane's q of step s is q_lo + kq + 4 s: row pointers of its first q
  const double *__restrict__ pfs = p.FS + (size_t)(form * nblk + blk) * GREEN_FS + (size_t)(q_lo + kq) * fs_q;
  const double *__restrict__ pfj = pfs + 2 + 2 * j;     // this lane's (up, down) pair of the row
  const double *__restrict__ pds[4];
#pragma unroll
  for (int i = 0; i < 4; i++) pds[i] = p.DS + (size_t)(2 * form) * nl + (size_t)(q_lo + kq) * ds_q + 2 * k[i];
  const double *__restrict__ pdb = p.DB + dev0;        // (rows have 64 doubles of slack behind the last one: tiles past the padded list)
  auto load_db = [&](const int s, auto tail, GreenMfmaDb &db) {
    constexpr bool TAIL = decltype(tail)::value;
    int q = q_lo + kq + 4 * s;
    if constexpr (TAIL) q = min(q, q_hi - 1);
    // q / ng (q < 65536, radtran_api.hip's guard on NQ; one g-point: ng_inv wraps to 0, q is the bin itself)
    const int b = ng == 1 ? q : (int)__umulhi((unsigned)q, ng_inv);
    const double *row = pdb + (size_t)b * p.ndev_pad;
#pragma unroll
    for (int i = 0; i < 4; i++) db.v[i] = row[16 * i];
  };
  auto load = [&](const int s, auto tail, GreenMfmaStep &in) {
    constexpr bool TAIL = decltype(tail)::value;
    // rows from the lane's first one: a wave-uniform count kept in a scalar register (opaque to the loop optimiser, which
    // otherwise carries one 64-bit induction pointer per load and input set in vector registers -- and spills them)
    size_t dq = (size_t)(unsigned)(4 * s);
    asm volatile("" : "+s"(dq));
    const double *fs = pfs + dq * fs_q, *fj = pfj + dq * fs_q;
    bool valid = true;
    size_t back = 0;
    if constexpr (TAIL) {
      const int q = q_lo + kq + 4 * s;
      valid = q < q_hi;
      back = valid ? 0 : (size_t)(q - (q_hi - 1));
      fs -= back * fs_q; fj -= back * fs_q;
    }
    in.lref[0] = fs[0]; in.lref[1] = fs[fs_b1];
    const double2 f0 = *reinterpret_cast<const double2 *>(fj), f1 = *reinterpret_cast<const double2 *>(fj + fs_b1);
    in.fu[0] = valid ? f0.x : 0.0; in.fd[0] = valid ? f0.y : 0.0;
    in.fu[1] = valid ? f1.x : 0.0; in.fd[1] = valid ? f1.y : 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) in.da[i] = *reinterpret_cast<const double2 *>(pds[i] + (dq - back) * ds_q);
  };
  auto work = [&](const GreenMfmaStep &in, const GreenMfmaDb &db) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double prod = db.v[i] * in.da[i].x;
#pragma unroll
      for (int b = 0; b < GREEN_NB; b++) {
        const int e = mine[b][i] ? (int)(in.lref[b] - in.da[i].y) : -4000;   // (sums of binary exponents: far inside the int range)
        const double a = __builtin_ldexp(prod, e);
        cu[b][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, in.fu[b], cu[b][i], 0, 0, 0);
        cd[b][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, in.fd[b], cd[b][i], 0, 0, 0);
      }
    }
  };
  using No = std::integral_constant<bool, false>;
  using Yes = std::integral_constant<bool, true>;
  // Two input sets used in turn: the loads of a step are issued before the products of the step before it.  The Planck
  // differences belong to a bin: with 8 g-points a PAIR of steps is one bin (q_lo is a multiple of ng) and they are loaded
  // once per pair, two sets of their own in turn; otherwise with every step.  A prefetch at the end of the split names
  // an existing step again rather than running past it.
  GreenMfmaStep S0, S1;
  GreenMfmaDb D0, D1;
  const int last = nfull - 1;
  // (the scheduling barriers keep the loads where they are written: left alone, the scheduler sinks a step's loads down to
  // their first use to save registers, and every step then waits a full memory round trip)
  if constexpr (NG8) {
    const int npair = nfull >> 1;     // (nfull is even, rest = 0)
    if (npair > 0) { load(0, No{}, S0); load_db(0, No{}, D0); }
    for (int i = 0; i < npair; i += 2) {
      load(2 * i + 1, No{}, S1);
      __builtin_amdgcn_sched_barrier(0);
      work(S0, D0);
      __builtin_amdgcn_sched_barrier(0);
      load(min(2 * i + 2, last), No{}, S0); load_db(min(2 * i + 2, last), No{}, D1);
      __builtin_amdgcn_sched_barrier(0);
      work(S1, D0);
      __builtin_amdgcn_sched_barrier(0);
      if (i + 1 < npair) {
        load(2 * i + 3, No{}, S1);
        __builtin_amdgcn_sched_barrier(0);
        work(S0, D1);
        __builtin_amdgcn_sched_barrier(0);
        load(min(2 * i + 4, last), No{}, S0); load_db(min(2 * i + 4, last), No{}, D0);
        __builtin_amdgcn_sched_barrier(0);
        work(S1, D1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
    if (nfull > 0) { load(0, No{}, S0); load_db(0, No{}, D0); }
    for (int s = 0; s < nfull; s += 2) {
      load(min(s + 1, last), No{}, S1); load_db(min(s + 1, last), No{}, D1);
      __builtin_amdgcn_sched_barrier(0);
      work(S0, D0);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < nfull) {
        load(min(s + 2, last), No{}, S0); load_db(min(s + 2, last), No{}, D0);
        __builtin_amdgcn_sched_barrier(0);
        work(S1, D1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (rest) {
      load(nfull, Yes{}, S0); load_db(nfull, Yes{}, D0);
      work(S0, D0);
    }
  }
}
// Block index -> (chunk of 64 deviations, bin split, pair of level blocks).  The
// chunks of a pair of blocks: first those of the below-form prefix (the second block's: it is the longer one; a row that is
// below the second block only sits out the first), then those of the above-form suffix (the first block's);
// ceil(ndev / 64) + 1 of them at most.
// (two waves per SIMD at least: with at most 256 registers the compiler keeps the accumulators of the products in
// VGPRs; allowed 512 it put them in AGPRs -- and copied all of them to VGPRs and back in every K step)
__host__ __device__ inline int green_far_chunks(int ndev) { return (ndev + 63) / 64 + 1; }
__global__ __launch_bounds__(64, 2) void k_green_accum_far_mfma(GreenParams p) {
  const int nz = p.nz, nl = nz + 1, nblk = (nl + GREEN_LB - 1) / GREEN_LB, nbp = (nblk + GREEN_NB - 1) / GREEN_NB;
  // consecutive workgroup ids go round-robin over the 8 XCDs (each with its own L2): the waves of one bin split -- all its
  // chunks, which read the SAME level factors, and all block pairs of a chunk, which read the same amplitudes -- take
  // consecutive ids on XCD split % 8
  // (fewer than 8 splits -- thousands of deviations: the chunks go round the XCDs instead, or 8 - qsplit of them would idle:
  // 4 836 deviations in 2 splits took 5.96 ms on two XCDs)
  const int nchunk = green_far_chunks(p.ndev);
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int bp = slot % nbp, w = slot / nbp;
  int chunk, split;
  if (p.qsplit >= 8) { chunk = w % nchunk; split = (w / nchunk) * 8 + xcd; }
  else { const int unit = w * 8 + xcd; chunk = unit % nchunk; split = unit / nchunk; }
  if (split >= p.qsplit) return;
  const int lane = threadIdx.x;
  const int blk = bp * GREEN_NB;
  const bool two = blk + 1 < nblk;
  // the ranges of the sorted list (green_block_class): below form k <= lv0 - 2, above form k >= max(2, lv1 + 1)
  int c1[GREEN_NB] = {0, 0}, c0[GREEN_NB] = {0, 0};
  for (int d0 = 0; d0 < p.ndev; d0 += 64) {
    const int d = d0 + lane;
    const int kd = d < p.ndev ? p.dev_k[d] : 0x7fffffff;
#pragma unroll
    for (int b = 0; b < GREEN_NB; b++) {
      const int lv0 = (blk + b) * GREEN_LB, lv1 = min(lv0 + GREEN_LB - 1, nz);
      c1[b] += __popcll(__ballot(kd <= lv0 - 2));
      c0[b] += __popcll(__ballot(kd < max(2, lv1 + 1)));
    }
  }
  if (!two) { c1[1] = 0; c0[1] = p.ndev; }     // no second block: no row takes it
  const int c1max = max(c1[0], c1[1]), c0min = min(c0[0], c0[1]);
  const int n1 = (c1max + 63) / 64;
  const int form = chunk < n1 ? 1 : 0;
  const int d_lo = form ? 64 * chunk : c0min + 64 * (chunk - n1), d_hi = form ? min(c1max, d_lo + 64) : min(p.ndev, d_lo + 64);
  if (d_lo >= d_hi) return;
  int k[4];
  bool mine[GREEN_NB][4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int d = d_lo + 16 * t + (lane & 15);
    k[t] = d < d_hi ? p.dev_k[d] : 0;
#pragma unroll
    for (int b = 0; b < GREEN_NB; b++) mine[b][t] = d < d_hi && (form ? d < c1[b] : d >= c0[b]);
  }
  const int per = (p.n_ir + p.qsplit - 1) / p.qsplit;
  const int b_lo = split * per, b_hi = min(p.n_ir, b_lo + per);
  green_d4 cu[GREEN_NB][4], cd[GREEN_NB][4];
#pragma unroll
  for (int b = 0; b < GREEN_NB; b++)
#pragma unroll
    for (int t = 0; t < 4; t++) { cu[b][t] = (green_d4){0.0, 0.0, 0.0, 0.0}; cd[b][t] = (green_d4){0.0, 0.0, 0.0, 0.0}; }
  if (b_hi > b_lo) {
    if (p.ng == 8) green_far_pass_mfma<true>(p, form, mine, k, d_lo + (lane & 15), blk, nblk, b_lo * p.ng, b_hi * p.ng, cu, cd);
    else green_far_pass_mfma<false>(p, form, mine, k, d_lo + (lane & 15), blk, nblk, b_lo * p.ng, b_hi * p.ng, cu, cd);
  }
#pragma unroll
  for (int b = 0; b < GREEN_NB; b++) {
    const int lv = (blk + b) * GREEN_LB + (lane & 15);
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int d = d_lo + 16 * t + (lane >> 4) + 4 * r;
        if (d < d_hi && (form ? d < c1[b] : d >= c0[b]) && lv < nl) {
          double *o = p.partial + (((size_t)split * p.ndev_pad + d) * 2) * nl;
          o[lv] = cu[b][t][r]; o[nl + lv] = cd[b][t][r];
        }
      }
    }
  }
}

// the value of lane N (0...15) of each 16-lane row, in every lane of the row (ds_swizzle, bit-mask mode: and 0x10, or N)
template <int N>
__device__ __forceinline__ double row16_lane(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_swizzle((int)b, 0x10 | (N << 5));
  const int hi = __builtin_amdgcn_ds_swizzle((int)(b >> 32), 0x10 | (N << 5));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// 7b. accumulation, the (deviation, level block) pairs of mixed class (the one or two blocks around a deviation's own
//     levels; listed by the host): a wave = four pairs x 16 levels, thread (pair, level) sums its bins and g-points with
//     the exponential per term; blockIdx.y = bin split
//     Consecutive pairs belong to neighbouring deviations -- the same one or two level blocks, neighbouring k -- and read
//     the same lines of IS and DS.  Consecutive workgroup ids go round-robin over the 8 XCDs, each with its own L2, so
//     the id is mapped to the group of pairs such that an XCD takes a CONTIGUOUS run of groups (as the ids came, every
//     group missed in its L2 for itself: 1.8 % hits, 536 MB fetched for ~250 MB of distinct data).
__global__ __launch_bounds__(64) void k_green_accum_mixed(GreenParams p) {
  const int per_xcd = (int)gridDim.x >> 3;      // (the grid's x extent is a multiple of 8: launch_green_accumulate)
  const int grp = ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
  const int pair = grp * 4 + (threadIdx.x >> 4), j = threadIdx.x & 15;
  const int nz = p.nz, nl = nz + 1, ng = p.ng;
  const int dev = pair < p.nmix ? p.mix_dev[pair] : -1;
  const int lv = pair < p.nmix ? p.mix_blk[pair] * GREEN_LB + j : nl;
  const bool on = dev >= 0 && lv < nl;
  const int k = on ? p.dev_k[dev] : 0;
  int cls = 3, slot = 0;
  if (on) cls = green_class(lv, k, slot);
  const int per = (p.n_ir + p.msplit - 1) / p.msplit;      // (its own, finer bin splits: few pairs, a long dependent loop each)
  const int b_lo = (int)blockIdx.y * per, b_hi = min(p.n_ir, b_lo + per);
  const size_t is_q = (size_t)GREEN_IS * nl, ds_q = (size_t)GREEN_DS * nl;
  // one branch-free body for the three classes (so that the loads of several g-points go out together): a far-form
  // level reads (log, up, down) of the level and (amplitude, log) of the deviation; an explicit level reads its two
  // values in place of the level factors and takes the amplitude as 1
  const bool far = cls < 2;
  const double *__restrict__ isx = p.IS + (size_t)(cls == 1 ? 3 : 0) * nl + (on ? lv : 0);   // XL, F_up, F_dn at +0, +nl, +2nl
  // (amplitude, its log) of the deviation in the two forms belong to the pair, not to the level: lanes 0 and 1 of the pair's
  // 16 load them and the others take them over the LDS crossbar -- as 16 identical loads per pair they were two fifths of
  // the bytes the kernel draws from its L1
  const double *__restrict__ dsa01 = p.DS + (size_t)(j == 1 ? 2 : 0) * nl + 2 * k;
  // (level 0's explicit values, slot 2, for k <= 1: D0[q][k][up, down])
  const double *__restrict__ fu = far ? isx + nl : slot == 2 ? p.D0 + 2 * min(k, 1) : p.DS + (size_t)(4 + 2 * slot) * nl + k;
  const double *__restrict__ fd = far ? isx + 2 * nl : slot == 2 ? p.D0 + 2 * min(k, 1) + 1 : p.DS + (size_t)(5 + 2 * slot) * nl + k;
  const size_t f_q = far ? is_q : slot == 2 ? (size_t)4 : ds_q;
  double up = 0.0, dn = 0.0;
  constexpr int U = 4;
  for (int b = b_lo; b < b_hi; b++) {
    const double dbv = on ? p.DB[(size_t)b * p.ndev_pad + dev] : 0.0;
    double su = 0.0, sd = 0.0;
    for (int g0 = 0; g0 < ng; g0 += U) {
      double x[U], am[U], vu[U], vd[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t q = (size_t)b * ng + min(g0 + u, ng - 1);
        double2 ld = {0.0, 0.0};
        if (j < 2) ld = *reinterpret_cast<const double2 *>(dsa01 + q * ds_q);    // lane 0: the above form's pair, lane 1: the below form's
        const double a0 = row16_lane<0>(ld.x), l0 = row16_lane<0>(ld.y), a1 = row16_lane<1>(ld.x), l1 = row16_lane<1>(ld.y);
        x[u] = isx[q * is_q] - (cls == 1 ? l1 : l0);
        am[u] = cls == 1 ? a1 : a0;
        vu[u] = fu[q * f_q]; vd[u] = fd[q * f_q];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const double ex = am[u] * green_exp2i(x[u]);
        const double a = (g0 + u < ng) ? (far ? ex : 1.0) : 0.0;
        su = __builtin_fma(a, vu[u], su);
        sd = __builtin_fma(a, vd[u], sd);
      }
    }
    up = __builtin_fma(dbv, su, up);
    dn = __builtin_fma(dbv, sd, dn);
  }
  if (on) {
    double *o = p.partial_m + (((size_t)blockIdx.y * p.ndev_pad + dev) * 2) * nl;
    o[lv] = up; o[nl + lv] = dn;
  }
}

// the response of level lv to deviation dev, its bin splits' partial sums added onto (up, dn) in split order (bitwise
// repeatable).  A level's sums sit where the kernel that formed them put them: far form or the mixed blocks' own splits.
__device__ __forceinline__ void green_split_sum(const GreenParams &p, int dev, int lv, double &up, double &dn) {
  const int nl = p.nz + 1;
  const bool mixed = green_block_class(p.dev_k[dev], lv / GREEN_LB, p.nz) == 2;
  const double *base = mixed ? p.partial_m : p.partial;
  const int ns = mixed ? p.msplit : p.qsplit;
  // eight splits' loads at a time, added in split order (one after the other each waited for the one before it:
  // 16 + 27 memory round trips per value)
  const size_t stride = (size_t)p.ndev_pad * 2 * nl;
  const double *pp0 = base + ((size_t)dev * 2) * nl + lv;
  for (int s0 = 0; s0 < ns; s0 += 8) {
    double u8[8], d8[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
      const double *pp = pp0 + (size_t)min(s0 + s, ns - 1) * stride;
      u8[s] = pp[0]; d8[s] = pp[nl];
    }
#pragma unroll
    for (int s = 0; s < 8; s++)
      if (s0 + s < ns) { up = up + u8[s]; dn = dn + d8[s]; }
  }
}

// 8. the columns: base rows + the responses of the column's deviations (splits in order), reversed to ground-first
//    (radiate.f90:140-154); f_total with the solar rows of the handle's last solar call (clima_radtran.f90:287).
//    A column that went through the general kernel (col_src >= 0) is copied.  out / gen_out: three arrays
//    [columns][nz+1] (up, down, f_total), out_arr / gen_arr elements apart.
__global__ __launch_bounds__(256) void k_green_combine(GreenParams p) {
  const int c = blockIdx.x, nl = p.nz + 1;
  const int src = p.col_src[c];
  double *o = p.out + (size_t)c * nl;
  for (int i = threadIdx.x; i < nl; i += blockDim.x) {
    if (src >= 0) {
      const double *s = p.gen_out + (size_t)src * nl;
      o[i] = s[i]; o[p.out_arr + i] = s[p.gen_arr + i]; o[2 * p.out_arr + i] = s[2 * p.gen_arr + i];
      continue;
    }
    const int lv = p.nz - i;
    double up = p.gen_out[i], dn = p.gen_out[p.gen_arr + i];    // column 0 of the general sub-batch is the base
    for (int j = p.col_ptr[c]; j < p.col_ptr[c + 1]; j++) green_split_sum(p, p.col_dev[j], lv, up, dn);
    o[i] = up; o[p.out_arr + i] = dn;
    o[2 * p.out_arr + i] = f_total_level(up, dn, p.flux_n[2 * nl + i], p.flux_n[3 * nl + i]);
  }
}

// 8'. the exact Jacobian (radtran_ir_jacobian): every level k = 0..nz is one deviation (dev_k sorted, one each), and its
//     responses to the Planck derivatives (k_green_dbdt) are the matrix's column j = nz - k (k TOA-first, the column of
//     x(1) = T_surface first), row i = nz - lv ground-first.  No base rows, no solar rows: the derivative of
//     f_total = (solar) + (dn - up) at fixed opacities is dn - up.  out: three (nz+1) x (nz+1) arrays column-major
//     (up, down, total), out_arr elements apart.  Block per deviation, thread per level.
__global__ __launch_bounds__(256) void k_green_jacobian(GreenParams p) {
  const int dev = blockIdx.x, nl = p.nz + 1;
  double *o = p.out + (size_t)(p.nz - p.dev_k[dev]) * nl;
  for (int i = threadIdx.x; i < nl; i += blockDim.x) {
    double up = 0.0, dn = 0.0;
    green_split_sum(p, dev, p.nz - i, up, dn);
    o[i] = up; o[p.out_arr + i] = dn; o[2 * p.out_arr + i] = dn - up;
  }
}

// 8''. the exact Jacobian in the caller's unknowns (radtran_ir_jacobian_reduced): group g's column is the sum of its
//     members' columns of 8', rows picked.  col_ptr / col_dev: the CSR of a group's deviations, members in ascending
//     column j (descending k); row_lv: the requested rows as levels, TOA-first.  Each member's entry is formed exactly as
//     k_green_jacobian forms it (green_split_sum from zero, splits in order) and then added onto the group's running
//     value, member after member: bitwise the caller's own loop over the full matrices, which are never written -- nor
//     is any level read that was not asked for.  blockIdx.y = group (at most nz + 1 of them), blockIdx.x = 64 rows;
//     threadIdx.y = four members whose split sums are in flight together (a zone of 400 levels is otherwise 400
//     dependent chains of loads, one after the other: with one member row a 201-member group at 402 layers took the
//     call from 0.89 to 1.27 ms, and the 1-4 member groups of a map without zones gained nothing from it, 0.644
//     against 0.635), thread row y = 0 adds them in member order.  out: (nrow, ngroup)
//     column-major -- up, down, total out_arr apart when `parts`, else the total alone.
constexpr int GREEN_RM = 4;
__global__ __launch_bounds__(64 * GREEN_RM) void k_green_jacobian_reduced(GreenParams p, const int *__restrict__ row_lv, int nrow, int parts) {
  const int g = blockIdx.y, a = blockIdx.x * 64 + threadIdx.x, y = threadIdx.y;
  const int m_lo = p.col_ptr[g], m_hi = p.col_ptr[g + 1];
  const int lv = a < nrow ? row_lv[a] : 0;
  __shared__ double su[GREEN_RM][64], sd[GREEN_RM][64];
  double gu = 0.0, gd = 0.0;
  for (int m0 = m_lo; m0 < m_hi; m0 += GREEN_RM) {      // (block-uniform bounds: every thread meets every barrier)
    double up = 0.0, dn = 0.0;
    if (m0 + y < m_hi && a < nrow) green_split_sum(p, p.col_dev[m0 + y], lv, up, dn);
    su[y][threadIdx.x] = up; sd[y][threadIdx.x] = dn;
    __syncthreads();
    if (y == 0) {
      const int n = min(GREEN_RM, m_hi - m0);
      for (int t = 0; t < n; t++) { gu = gu + su[t][threadIdx.x]; gd = gd + sd[t][threadIdx.x]; }
    }
    __syncthreads();
  }
  if (y == 0 && a < nrow) {
    double *o = p.out + (size_t)g * nrow + a;
    if (parts) { o[0] = gu; o[p.out_arr] = gd; o[2 * p.out_arr] = gd - gu; }
    else o[0] = gd - gu;
  }
}

// total = dn - up of a communicator handle's reduced Jacobian (radtran_ir_jacobian; a rank without IR bins runs this
// and no k_green_* kernel).  jac: three arrays of n doubles (up, down, total), arr elements apart.
__global__ __launch_bounds__(256) void k_jacobian_total(double *jac, size_t arr, size_t n) {
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x)
    jac[2 * arr + t] = jac[arr + t] - jac[t];
}
void launch_jacobian_total(double *jac, size_t arr, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_jacobian_total, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, s, jac, arr, n);
}

// f_total of a batch's columns from their (reduced) IR rows and the handle's solar rows (clima_radtran.f90:287): what a
// communicator handle runs after its all-reduce of the batch's up / down arrays.  out: three arrays [ncol][nz+1].
__global__ __launch_bounds__(256) void k_batch_ftotal(double *out, size_t out_arr, int ncol, int nl, const double *flux_n) {
  const size_t n = (size_t)ncol * nl;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(t % nl);
    out[2 * out_arr + t] = f_total_level(out[t], out[out_arr + t], flux_n[2 * nl + i], flux_n[3 * nl + i]);
  }
}
void launch_batch_ftotal(double *out, size_t out_arr, int ncol, int nz, const double *flux_n, hipStream_t s) {
  const size_t n = (size_t)ncol * (nz + 1);
  hipLaunchKernelGGL(k_batch_ftotal, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, s, out, out_arr, ncol, nz + 1, flux_n);
}

void launch_green_factor(const GreenParams &p, hipStream_t s) {
  const int nz = p.nz, nl = nz + 1, NQ = p.NQ;
  hipLaunchKernelGGL(k_green_factor, dim3(NQ), dim3(64), 0, s, p);
  hipLaunchKernelGGL(k_green_unit, dim3((nl + 255) / 256, NQ), dim3(256), 0, s, p);
  const int nblk = (nl + GREEN_LB - 1) / GREEN_LB;
  hipLaunchKernelGGL(k_green_local, dim3((nblk * GREEN_LB + 255) / 256, NQ), dim3(256), 0, s, p);
}
// the far accumulation's form: 0 the matrix form, 1 the vector form it replaced (the test hook of the parity test of the two)
static int g_green_vector_form = 0;
static bool green_vector_form() { return g_green_vector_form != 0; }
void green_vector_form_set(int vector_form) { g_green_vector_form = vector_form ? 1 : 0; }
// waves of the far accumulation that are resident at a time (the host cuts the bins into so many splits that the kernel's
// waves fill the machine once): 1024 SIMDs x 2 waves of <= 256 registers in the matrix form, x 3 of 152 in the vector form
int green_far_resident_waves() { return green_vector_form() ? 2900 : 2048; }
// waves of the far accumulation per bin split
int green_far_waves(int ndev, int nl) {
  const int nblk = (nl + GREEN_LB - 1) / GREEN_LB;
  return green_vector_form() ? (ndev + 63) / 64 * nblk : green_far_chunks(ndev) * ((nblk + GREEN_NB - 1) / GREEN_NB);
}
// bin splits: the accumulation's waves should fill the machine ONCE -- a few waves more than that and the kernel takes
// two rounds.  The matrix form puts a split's waves on one XCD (split % 8): a multiple of 8 splits, or some XCDs carry a
// split more than the others (19 splits: 150 us where 16 take 90).
int green_far_splits(int n_ir, int waves) {
  int q = std::max(1, std::min(std::min(n_ir, 64), green_far_resident_waves() / std::max(waves, 1)));
  if (!green_vector_form() && q >= 8) q &= ~7;
  return q;
}
// the two accumulation kernels (DB given)
void launch_green_accumulate(const GreenParams &p, hipStream_t s) {
  const int nl = p.nz + 1;
  const int nblk = (nl + GREEN_LB - 1) / GREEN_LB, nunit = ((p.ndev + 63) / 64) * p.qsplit;
  if (green_vector_form()) hipLaunchKernelGGL(k_green_accum_far, dim3((unsigned)((nunit + 7) / 8 * 8 * nblk)), dim3(64), 0, s, p);
  else {
    const int nchunk = green_far_chunks(p.ndev), nbp = (nblk + GREEN_NB - 1) / GREEN_NB;
    const int per_xcd = p.qsplit >= 8 ? ((p.qsplit + 7) / 8) * nchunk : (nchunk * p.qsplit + 7) / 8;   // units per XCD (k_green_accum_far_mfma's two mappings)
    hipLaunchKernelGGL(k_green_accum_far_mfma, dim3((unsigned)(8 * per_xcd * nbp)), dim3(64), 0, s, p);
  }
  if (p.nmix > 0) hipLaunchKernelGGL(k_green_accum_mixed, dim3(((p.nmix + 3) / 4 + 7) / 8 * 8, p.msplit), dim3(64), 0, s, p);
}
void launch_green_columns(const GreenParams &p, int ncol, hipStream_t s) {
  if (p.ndev > 0) {
    hipLaunchKernelGGL(k_green_db, dim3((p.ndev_pad + 255) / 256, p.n_ir), dim3(256), 0, s, p);
    launch_green_accumulate(p, s);
  }
  hipLaunchKernelGGL(k_green_combine, dim3(ncol), dim3(256), 0, s, p);
}
// the exact Jacobian from the opacity-only part: Planck derivatives, the two accumulations, the matrices (ndev = nz + 1)
void launch_green_jacobian(const GreenParams &p, hipStream_t s) {
  hipLaunchKernelGGL(k_green_dbdt, dim3((p.ndev_pad + 255) / 256, p.n_ir), dim3(256), 0, s, p);
  launch_green_accumulate(p, s);
  hipLaunchKernelGGL(k_green_jacobian, dim3(p.ndev), dim3(256), 0, s, p);
}
// the same in the caller's unknowns: ngroup columns of nrow rows (k_green_jacobian_reduced)
void launch_green_jacobian_reduced(const GreenParams &p, const int *row_lv, int nrow, int ngroup, bool parts, hipStream_t s) {
  hipLaunchKernelGGL(k_green_dbdt, dim3((p.ndev_pad + 255) / 256, p.n_ir), dim3(256), 0, s, p);
  launch_green_accumulate(p, s);
  hipLaunchKernelGGL(k_green_jacobian_reduced, dim3((nrow + 63) / 64, ngroup), dim3(64, GREEN_RM), 0, s, p, row_lv, nrow, parts ? 1 : 0);
}
