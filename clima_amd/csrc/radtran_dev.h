// radtran_dev.h -- device-facing parameter blocks shared by the kernels and the host API.
//
// HBM layout (all f64 unless noted; "TOA-first" = index 0 is the top layer, as
// OpticalPropertiesResult in src/radtran/clima_radtran_types.f90:242-247, :862-865):
//
//   tables   log10k[s]      [nw][nT][nP][ng]   (the on-disk order, types_create.f90:1349-1358;
//                                               one (P,T) node = ng contiguous doubles = 64 B)
//            xs 0-D         [nw]               Rayleigh / photolysis / constant CIA
//            xs 1-D         [nw][nT]           log10 CIA, photolysis, H2O self/foreign continuum
//            particles      [nw][nrad] x3      w0, qext, g
//   column   T,P,dz [nz]; dens [nsp][nz]; pdens,radii [np][nz]   (ground-first, as the API)
//   prep     log10P, cols [nsp][nz], foreign_col, src (pair_reuse source layer),
//            per interpolation slot: left index ix[slot][nz] (i32) and weight q[slot][nz]
//   opr      tau, w0        [nw][ng][nz]       TOA-first; == Fortran (nz,ng,nw) column-major
//            g, tau_band    [nw][nz]
//   results  fup_a, fdn_a, amean [nw_ch][nz+1]; tau_band [nw_ch][nz]   ground-first,
//            == Fortran (nz+1,nw_ch) column-major (ClimaRadtranWrk, clima_radtran.f90:11-25)
//            level rows     [5][nz+1] + 1      ir_up, ir_dn, sol_up, sol_dn, f_total, error words (level_rows below)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

namespace clima {

// Crossing windows of the window-form rebin (kernels.hip rb_lo / rb_hi), indexed by the output edge
// 1..7: element range that can contain the crossing of that edge.  The host checks a handle's weights
// against them (rebin_windows_fit, radtran_api.hip).
constexpr int RB_WIN_LO[8] = {0, 1, 5, 10, 18, 27, 39, 52};        // any order of the sums
constexpr int RB_WIN_HI[8] = {0, 11, 24, 36, 45, 53, 58, 62};
constexpr int RB_TIGHT_LO[8] = {0, 5, 12, 19, 27, 35, 45, 55};     // x and y ascending: prefixes are down-sets of the 8x8 grid
constexpr int RB_TIGHT_HI[8] = {0, 8, 18, 28, 36, 44, 51, 58};

constexpr int MAX_K = 8;      // k-distribution species
constexpr int MAX_XS = 16;    // per Xsection kind
constexpr int MAX_PART = 4;   // particle species
constexpr int MAX_ZEN = 16;   // zenith angles passed by value to the two-stream kernel
constexpr int MAX_SLOTS = 2 * MAX_K + 2 * MAX_XS + 1 + MAX_PART + 1;  // + custom optical properties axis

// src/clima_const.f90:9-21
constexpr double PLANK = 6.62607004e-34;
constexpr double C_LIGHT = 299792458.0;
constexpr double K_BOLTZ_SI = 1.380649e-23;
constexpr double PI = 3.14159265358979323846e0;
constexpr double SIGMA_SI = 5.670374419e-8;
// src/radtran/clima_radtran_types.f90:9-11
constexpr double MAX_W0 = 0.99999;
constexpr double MAX_GT = 0.999999;
constexpr double TAU_MIN = 1.0e-20;
constexpr double LN10 = 2.302585092994045684017991454684364207601;
constexpr double TINY = 2.2250738585072014e-308;  // tiny(0.0_dp), clima_radtran_types.f90:558-562

struct XsDev {
  const double *data;  // dim 0: [nw]; dim 1: [nw][nT]
  int dim, sp1, sp2, nT, slot;
};

// One term of the continuum absorption taua (types.f90:696-723), in the reference's
// summation order: CIA pairs, photolysis/absorption, H2O self and foreign continuum.
// tau = sigma(bin, T_layer) * weight(layer); the weight is bin-independent and is formed
// once per call by the prep kernel.
constexpr int ABS_BATCH = 8;          // the opacity tile takes continuum terms in batches of this many; the host pads the list
constexpr int MAX_ABS = 2 * 16 + 2 + 6;  // (2 MAX_XS + 2 real terms, rounded up to a multiple of ABS_BATCH)
enum { ABS_CIA = 0, ABS_COLUMN = 1, ABS_H2O_SELF = 2, ABS_H2O_FOREIGN = 3, ABS_ZERO = 4 };  // ABS_ZERO: padding, weight 0
struct AbsEntry {
  const double *data;  // nT == 0: xs[nw]; else log10 xs [nw][nT]
  int nT;              // 0 for constant (0-D) cross sections
  int slot;            // interpolation slot (any valid slot when nT == 0)
  int kind, a, b;      // weight: CIA dens_a*dens_b*dz | cols_a | dens_a*cols_a | dens_a*foreign_col
};

struct KDev {
  const double *log10k;  // [nw][nT][nP][ng]
  int sp, nP, nT, slotP, slotT;
};

struct PartDev {
  const double *w0, *qext, *gt;  // [nw][nrad]
  int p_ind, nrad, slot;
};

// One interpolation axis evaluated per layer by the prep kernel: clamp, bracket
// (dintrv semantics, linear_interpolation_module.F90:348-350), weight.
struct SlotDev {
  const double *axis;
  int n;
  int source;  // 0 = log10(P), 1 = T, 2+p = radius of particle column p, -1 = log10(P*1e6) of the layer itself (custom opacity)
  double lo, hi;
  int flag_clamp;  // particles: out-of-range radius is an error (types.f90:973-976)
};

// Flags of an entry of the compact source-layer list (ColumnDev::meta)
constexpr int SRC_PAIR = 1 << 30;    // layer j+1 reuses this layer (pair_reuse, types.f90:621-632)
constexpr int SRC_EXACT = 1 << 29;   // ... and every input of layer j+1 is bitwise equal to layer j's
constexpr int SRC_LAYER = 0xffff;

// ---- what the host and the kernels must agree on, each stated once ----

// futils is_close (fortran-stdlib form).  Every operation is rounded on its own, and no product feeds the difference.
__host__ __device__ inline bool is_close(double a, double b, double tol) {
#pragma clang fp contract(off)
  const double fa = fabs(a), fb = fabs(b);
  return fabs(a - b) <= fabs(tol * (fa < fb ? fb : fa));
}

// Column block [T_surface | T | P | dz | dens | pdens | radii | meta]: offsets in doubles (T_surface at 0), dens
// [nsp][nz], pdens / radii [np][nz]; meta is (2 nz + 1) ints (see ColumnDev::meta) and one int of padding.
struct ColumnLayout { size_t T, P, dz, dens, pdens, radii, meta, count; };
__host__ __device__ inline ColumnLayout column_layout(int nz, int nsp, int np) {
  ColumnLayout l;
  l.T = 1; l.P = l.T + nz; l.dz = l.P + nz; l.dens = l.dz + nz;
  l.pdens = l.dens + (size_t)nsp * nz; l.radii = l.pdens + (size_t)np * nz; l.meta = l.radii + (size_t)np * nz;
  l.count = l.meta + nz + 1;
  return l;
}

// Bounds block of one column of a batch (radtran_toa_fluxes_batch_bounds): [albedo | emissivity | u | w | 1/u | scale],
// offsets in doubles: surface_albedo [nw_sol] and surface_emissivity [nw_ir] in the channels' own bin order, the zenith
// cosines, their weights and the cosines' reciprocals [nzen] each, photon_scale_factor.  Built by the host beside the
// column blocks (pack_bounds) or by k_pack_bounds; read by the two-stream kernels in place of the handle's fields.
struct BoundsLayout { size_t albedo, emissivity, u, w, iu, scale, count; };
__host__ __device__ inline BoundsLayout bounds_layout(int nw_sol, int nw_ir, int nzen) {
  BoundsLayout l;
  l.albedo = 0; l.emissivity = l.albedo + nw_sol; l.u = l.emissivity + nw_ir; l.w = l.u + nzen; l.iu = l.w + nzen;
  l.scale = l.iu + nzen; l.count = l.scale + 1;
  return l;
}
// ... and the five arrays a caller gives (column after column in each: albedo (nw_sol, ncol), emissivity (nw_ir, ncol),
// zenith_u / zenith_w (nzen, ncol), scale (ncol)); a null array: every column takes the handle's value of that field.
// Host or device pointers.
struct BoundsArrays {
  const double *albedo, *emissivity, *zenith_u, *zenith_w, *scale;
  __host__ __device__ bool any() const { return albedo || emissivity || zenith_u || zenith_w || scale; }
};
// Element i of column c's block: the caller's value, or the handle's (`own`: its four arrays the same way, one column;
// own_scale: its photon_scale_factor)
__host__ __device__ inline double bounds_element(const BoundsLayout &l, size_t i, size_t c, const BoundsArrays &in, const BoundsArrays &own,
                                                 double own_scale) {
  const size_t nzen = l.w - l.u;
  if (i < l.emissivity) return in.albedo ? in.albedo[c * l.emissivity + i] : own.albedo[i];
  if (i < l.u) { const size_t k = i - l.emissivity, n = l.u - l.emissivity; return in.emissivity ? in.emissivity[c * n + k] : own.emissivity[k]; }
  if (i < l.w) { const size_t k = i - l.u; return in.zenith_u ? in.zenith_u[c * nzen + k] : own.zenith_u[k]; }
  if (i < l.iu) { const size_t k = i - l.w; return in.zenith_w ? in.zenith_w[c * nzen + k] : own.zenith_w[k]; }
  if (i < l.scale) { const size_t k = i - l.iu; return 1.0 / (in.zenith_u ? in.zenith_u[c * nzen + k] : own.zenith_u[k]); }   // a correctly rounded division on both sides
  return in.scale ? in.scale[c] : own_scale;
}

// A column as the callers hand it over (the ABI's order): T_surface a scalar, T / P / dz [nz], dens [nsp][nz], pdens /
// radii [np][nz] -- of a batch, column after column in each array (T_surface [ncol]).  Host or device pointers.
struct ColumnArrays {
  const double *T_surface, *T, *P, *dens, *dz, *pdens, *radii;
  __host__ __device__ bool has_particles() const { return pdens && radii; }
  // column c of a batch; the particle arrays come together or not at all (one without the other counts as none, and
  // so do both where the handle has no particle columns)
  __host__ __device__ ColumnArrays column(size_t c, int nz, int nsp, int np) const {
    const bool hp = np > 0 && has_particles();
    return ColumnArrays{T_surface + c, T + c * nz, P + c * nz, dens + c * nz * nsp, dz + c * nz,
                        hp ? pdens + c * nz * np : nullptr, hp ? radii + c * nz * np : nullptr};
  }
};

// Level-row block: [ir_up | ir_dn | sol_up | sol_dn | f_total][nl] doubles, nl = nz + 1, then one double that holds the
// two device error words (ints: opacity failure, expired fused hand-off wait).  The handle's d_small / h_small are one
// such block; a batch's arena holds `stride` doubles of it per column (no error words).  On a handle with a communicator
// the first double of the f_total row is the step's status word instead, and the all-reduce covers the four flux rows
// and that word (reduce_count); f_total itself is formed on the host from the fetched rows, or by k_batch_finish.
struct LevelRows {
  size_t nl;
  size_t ir_up, ir_dn, sol_up, sol_dn;   // row offsets: row a of the four at a * nl
  size_t f_total, status;                // the fifth row == the status word's slot
  size_t flux_count;                     // doubles of the four flux rows
  size_t err_words;                      // offset of the double that holds the two ints
  size_t stride;                         // doubles per column of an arena: the five rows
  size_t count;                          // doubles of the whole block
  size_t reduce_count;                   // doubles the all-reduce sums: the four rows and the status word
  __host__ __device__ size_t row(int a) const { return a * nl; }
};
__host__ __device__ inline LevelRows level_rows(int nz) {
  LevelRows l;
  l.nl = (size_t)nz + 1;
  l.ir_up = 0; l.ir_dn = l.nl; l.sol_up = 2 * l.nl; l.sol_dn = 3 * l.nl;
  l.f_total = l.status = 4 * l.nl; l.flux_count = 4 * l.nl;
  l.err_words = l.stride = 5 * l.nl;
  l.count = l.err_words + 1; l.reduce_count = l.flux_count + 1;
  return l;
}

// pair_reuse (clima_radtran_types.f90:621-632) of the pair (j-1, j), j odd (0-based), of a column with an even number
// of layers: layer j reuses layer j-1 when P, T, every column density * dz and (use_radii: the column comes with
// particles and the handle has particle opacities) every radius agree to 1e-12 (is_close).  The columns are stored
// products in the reference (opw%cols): each is rounded before the comparison, never fused into it.  exact: reused,
// and every input of layer j is bitwise equal to layer j-1's.  pdens / radii: [np][nz], or null (no particles given).
struct PairDecision { bool reuse, exact; };
__host__ __device__ inline PairDecision pair_decision(int j, int nz, int nsp, int np, const double *T, const double *P,
                                                      const double *dz, const double *dens, const double *pdens,
                                                      const double *radii, bool use_radii) {
#pragma clang fp contract(off)
  const double tol = 1.0e-12;
  bool reuse = is_close(P[j], P[j - 1], tol) && is_close(T[j], T[j - 1], tol);
  bool exact = P[j] == P[j - 1] && T[j] == T[j - 1] && dz[j] == dz[j - 1];
  for (int i = 0; i < nsp && reuse; i++) {
    const double nb = dens[(size_t)i * nz + j], na = dens[(size_t)i * nz + j - 1];
    const double cb = nb * dz[j], ca = na * dz[j - 1];   // opw%cols
    reuse = is_close(cb, ca, tol);
    exact = exact && nb == na;
  }
  if (use_radii)
    for (int i = 0; i < np && reuse; i++) reuse = is_close(radii[(size_t)i * nz + j], radii[(size_t)i * nz + j - 1], tol);
  if (reuse && pdens && radii)
    for (int i = 0; i < np; i++)
      exact = exact && pdens[(size_t)i * nz + j] == pdens[(size_t)i * nz + j - 1] &&
              radii[(size_t)i * nz + j] == radii[(size_t)i * nz + j - 1];
  return PairDecision{reuse, exact && reuse};
}

// f_total of a level from its four fluxes (clima_radtran.f90:287), in this association everywhere: the device batch
// is held byte for byte to the host batch
__host__ __device__ inline double f_total_level(double ir_up, double ir_dn, double sol_up, double sol_dn) {
  return (sol_dn - sol_up) + (ir_dn - ir_up);
}
// ... and ISR, OLR: the net solar and IR fluxes of the last level (clima_radtran.f90:339-340)
__host__ __device__ inline void toa_isr_olr(double ir_up, double ir_dn, double sol_up, double sol_dn, double &ISR, double &OLR) {
  ISR = sol_dn - sol_up; OLR = -(ir_dn - ir_up);
}

// Spectral integration (kernels.hip): bins per chunk, levels per block of the one-launch kernel, whose dynamic LDS
// holds the widths [nchunk * INT_CHUNK] and the chunk sums [nchunk][INT_LV]
constexpr int INT_CHUNK = 32;
constexpr int INT_LV = 16;
inline int integrate_chunks(int nbins) { return nbins <= 0 ? 1 : (nbins + INT_CHUNK - 1) / INT_CHUNK; }
inline size_t integrate_lds_bytes(int nchunk) { return sizeof(double) * (size_t)nchunk * (INT_CHUNK + INT_LV); }
// true when launch_integrate() takes the one-launch kernel (the form that can store into the host's block)
inline bool integrate_fits_one_launch(int nchunk) { return integrate_lds_bytes(nchunk) <= 64 * 1024; }

// Element strides from one column of a batch to the next (0 everywhere for a single call).  Every
// per-column array of a group lives in ONE block per column with the same internal layout, so a
// group needs one stride: the column inputs, the prep results, the optical properties, the per-bin
// spectra, the level fluxes, the bounds blocks (where the batch has them), the hand-off flags.
struct BatchStrides {
  size_t col, prep, opr, res, flux;
  int done, bnd;
};

struct ColumnDev {
  const double *T, *P, *dz, *dens, *pdens, *radii;  // dens [nsp][nz], pdens/radii [np][nz]
  // pair_reuse decided when the column block is built (pair_decision, by the host at upload or by
  // k_pack_columns): meta[0] = nsrc, meta[1 + m] = source layer m | SRC_* flags
  // (ascending), meta[1 + nz + j] = source layer of layer j (j, or j-1 for the second of a pair)
  const int *meta;
  double *log10P, *cols, *foreign_col;
  double *absw;    // [nabs][nz] per-layer weights of the absorption entries
  int *ix;         // [nslots][nz]
  double *q;       // [nslots][nz]
  int *err_flag;   // device error word: id of the last call that clamped a particle radius
  const double *T_surface;  // device scalar
};

// custom optical properties (types.f90:432-572): per bin, linear in log10(P cgs)
struct CustomDev {
  const double *dtau, *w0, *g0;  // [nw][nP]
  int nP, slot, on;
};

struct OpacityParams {
  int nz, nw, ng, nsp, np;
  int bin_lo, nbins;  // opacity bins handled by this launch
  int nsrc;           // source layers of the column (host count, == meta[0]); nz for a batch (upper bound)
  int coop, generic;  // unused (the launch plan says which opacity kernel runs); they keep the kernels' argument layout
  int nk, nray, npart;
  KDev k[MAX_K];
  XsDev ray[MAX_XS];
  int nabs;
  AbsEntry abs[MAX_ABS];
  PartDev part[MAX_PART];
  const double *wbin, *wbin_e, *wxy;      // Ksettings (types.f90:84-94)
  const double *wbin_e_pad;               // wbin_e followed by +inf sentinels (edge stream of the rebin)
  const double *rorr_tab;                 // ng = 8: [E_1..E_8, w_0..w_7, 1/(E_(k+1)-E_k)], read into scalar registers by rorr_xys_asm.inc
  ColumnDev col;
  double *tau, *w0, *g, *tau_band;        // opr
  double *scat;                           // [nw][nz] scattering optical depth tausg + tausp + tausc of a layer (every g-point's
                                          // w0 is min(MAX_W0, scat / tau)): written always
  int write_w0;                           // 0: the two-stream part of the same fused grid forms w0 from scat itself, the
                                          // 8 x nw x nz values are neither written nor read back (the host materialises
                                          // them when something else asks for them)
  long long *stamps;                      // diagnostic build only (-DCLIMA_STAMPS); null otherwise
  int rebin_mode;                         // 0 window form (the weights fit the compiled crossing windows), 1 streaming,
                                          // 2 streaming with max(wxy) > min(wbin): an element may span several output edges
  CustomDev cust;
};

struct PrepParams {
  int ncol;                  // gridDim.y: columns of a batch (1 for a single call)
  BatchStrides bs;
  int nz, nsp, np, nslots, has_cont, LH2O;
  int call_id;  // stamped into err_flag by a failing call (monotonic, so the flag never needs a reset)
  SlotDev slots[MAX_SLOTS];
  int nabs;
  int abs_kind[MAX_ABS], abs_a[MAX_ABS], abs_b[MAX_ABS];
  int nzero;                 // output arrays cleared by spare blocks of the prep launch (per column: + c*bs.res)
  double *zero_ptr[6];
  size_t zero_count[6];
  ColumnDev col;
};

struct TwoStreamParams {
  int nz, ng;
  int ncols, nchunks, nc_shift;            // g-point columns per block, chunks per column, log2(ncols) or -1 (launcher)
  int col_base, accumulate;                // wave kernel: first g-point of this launch; add into the outputs (launcher)
  // batched shared-opacity IR launches (wave kernel): gridDim.z = b_ncol temperature columns,
  // T + z*b_T, T_surface + z*b_Ts, IR spectra + z*b_out; all 0 for a single column
  int b_ncol, b_T, b_Ts;
  size_t b_out;
  // task list: blocks [0, n_sol) are solar bins sol_lo.., blocks [n_sol, n_sol+n_ir) IR bins
  int n_sol, sol_lo, n_ir, ir_lo;          // channel-local first bin of this launch
  int sol_start, ir_start;                 // channel -> opacity-bin offset (RTChannel%ind_start)
  const double *tau, *w0, *g, *tau_band;   // opr
  const double *scat;                      // see OpacityParams
  int w0_from_scat;                        // the layers' w0 = min(MAX_W0, scat / tau) instead of the stored array
  int bnd_nw_sol;                          // a bounds batch: the channels' bin counts (bounds_layout; bnd_nw_ir below)
  const double *wbin;
  const double *freq;                      // opacity grid [nw+1]
  // test hook (clima_test_two_stream): Planck values at the levels given directly [nz+1] TOA-first
  // instead of computed from T (null in production), and a slot count above ceil(nz/64) (0: none; the batched IR
  // launcher reads it, the other forms take theirs from the launch plan)
  const double *bplanck;
  int force_slots;
  // A bounds batch's launch (radtran_toa_fluxes_batch_bounds): 1 when `albedo` below is the (first) column's bounds block
  // (bounds_layout(bnd_nw_sol, bnd_nw_ir, nzen), whose first array is the albedo; column c of a chunk at + c *
  // BatchStrides::bnd), read in place of albedo, emissivity, the zenith arrays and photon_scale_factor.  0: the
  // handle's fields (every single call, the plain batches).  The block's address and these three ints sit in fields and
  // alignment gaps the block already had: its size, and with it the place of the hidden arguments behind it, is what
  // it was -- one more field changed how hipcc schedules the kernels of the calls WITHOUT bounds (the 8-slot ones began to spill).
  int bounds;
  // IR
  const double *T, *T_surface;
  const double *emissivity;                // [nw_ir]
  int has_hard_surface;
  int bnd_nw_ir;
  double ir_tau_min;
  // solar
  int nzen;
  const double *zen_u, *zen_w, *zen_iu;    // cos(zenith), weights, 1/cos (device arrays)
  // the same by value (kernarg segment -> scalar loads in the zenith loop); valid for nzen <= MAX_ZEN
  double zen_u_v[MAX_ZEN], zen_w_v[MAX_ZEN], zen_iu_v[MAX_ZEN];
  const double *albedo;                    // [nw_sol]; bounds: the bounds block
  const double *photons_sol;               // [nw_sol], unscaled
  double photon_scale_factor, diurnal_fac;
  const double *am_f1, *am_f2, *am_dw;     // per solar bin amean unit factors (radiate.f90:174-178)
  // outputs (channel-local bin index)
  double *ir_fup_a, *ir_fdn_a, *ir_tau_band;
  double *sol_fup_a, *sol_fdn_a, *sol_amean, *sol_tau_band;
};

// fused opacity + two-stream launch (k_fused), one workgroup per item.  Items of column c are the
// blocks [c*(n_op+n_ts), (c+1)*(n_op+n_ts)): first its n_op opacity tiles, then its n_ts two-stream
// items (one per (bin, g-point group), ordered by readiness).
struct FusedParams {
  int ncol;        // columns in this launch
  int n_op;        // opacity tiles per column (launcher; an upper bound when layers are reused)
  int n_ts;        // two-stream items per column (launcher)
  int call_id;     // value an opacity tile publishes in done[c][tile] when its results are out
  int max_spins;   // bound of a two-stream item's wait
  int *done;       // [ncol][n_op]
  int *timeout_flag;  // id of the last call in which a two-stream item's wait expired
  int slots;       // layers per lane of the two-stream part: ceil(nz/64) (launcher)
  int sol_early;   // solar bins whose opacities the first round of opacity tiles produces (launcher)
  BatchStrides bs;
};

// (TwoStreamParams::bounds: the calls without bounds keep their kernels only while these hold)
static_assert(sizeof(TwoStreamParams) == 720 && offsetof(TwoStreamParams, bounds) == 148 && offsetof(TwoStreamParams, bnd_nw_sol) == 116 &&
              offsetof(TwoStreamParams, bnd_nw_ir) == 180 && offsetof(TwoStreamParams, albedo) == 608,
              "TwoStreamParams has moved: the plain kernels' register allocation depends on its layout (see `bounds`)");
static_assert(sizeof(BatchStrides) == 48 && offsetof(BatchStrides, bnd) == 44, "BatchStrides has grown: see TwoStreamParams::bounds");

struct IntegrateParams {
  int ncol;                                // gridDim.z
  BatchStrides bs;
  int nz;
  int nw_ir, nw_sol;
  int ir_lo, ir_n, sol_lo, sol_n;          // bins owned by this rank (all when unsharded)
  int do_solar;
  const double *ir_fup_a, *ir_fdn_a, *sol_fup_a, *sol_fdn_a;
  const double *ir_freq, *sol_freq;        // channel freq [nw_ch+1]
  double *flux_n;                          // [4][nz+1]
  double *flux_part;                       // bin-sharded handles: this rank's partial rows (flux_n is all-reduced in place); else null
  double *unused;                          // (f_total is formed on the host, fetch_small, or by k_batch_finish); keeps the kernels' argument layout
  double *partial;                         // [4][nchunk][nz+1] chunk sums
  int nchunk;
  // handles with a communicator (radtran_comm_init_rank): one more word rides on the all-reduce behind the four
  // level rows -- 1 when this rank's fused hand-off timed out in the opacity pass `id_opr`, + 1024 when it did in
  // the pass of the last solar computation `id_sol` -- so that EVERY rank learns it and repeats the step unfused
  double *timeout_out;
  const int *timeout_flag;
  int id_opr, id_sol;
  // synchronous entry points (radtran_radiate_wrapper): the four level rows and the two device error words are
  // ALSO stored straight into the host's pinned result block (device address of it), so that the call ends with a
  // stream synchronise instead of a copy launch + synchronise.  Null otherwise.
  double *host_out;
  const int *err_words;
};

struct BatchIntegrateParams {
  int nz, ir_lo, ir_n, nchunk, col0;
  const double *fup_a, *fdn_a;   // [ncol][nw_ir][nz+1]
  size_t spec_stride;
  const double *freq;            // IR channel freq [nw_ir+1]
  double *partial;               // [ncol][2][nchunk][nz+1]
  const double *flux_n;          // the handle's [4][nz+1] (solar rows of the last solar call)
  double *out;                   // three arrays [ncol_total][nz+1], out_arr elements apart: fup_n, fdn_n, f_total
  size_t out_arr;
};

// Column batches whose inputs are device arrays (radtran_toa_fluxes_batch_device): k_pack_columns builds column c's block
// (column_layout(nz, nsp, np), pair-reuse table included) at blocks + c * its count out of the caller's arrays, which
// carry the column as their last dimension.
struct PackParams {
  int ncol, nz, nsp, np;
  int has_particles;         // pdens and radii are given (np > 0)
  int use_radii;             // ... and the handle has particle opacities: the radii take part in the pair decision
  ColumnArrays in;           // the caller's device arrays, column after column
  double *blocks;
  int *nsrc;                 // [ncol] every column's source-layer count once more, contiguous (null: not wanted)
};
// ... and k_batch_finish ends the batch on the device: f_total into the fifth row of every column's level rows (flux,
// level_rows(nz).stride apart), ISR / OLR (ncol), and the five rows into fluxes (nz+1, 5, ncol) when that is given.
struct BatchFinishParams {
  int ncol, nz;
  double *flux;
  double *ISR, *OLR, *fluxes;
};
// ... and k_batch_spectra takes the per-bin rows a caller asked for (radtran_toa_fluxes_batch_spectra) out of the `ncol`
// columns of one launch before the next launch overwrites them: of up to four per-column arrays [nw[k]][nl] (src[k],
// the columns src_stride doubles apart; dst[k] null: not wanted) the levels level[0 .. nsel) (0-based, ground-first)
// into dst[k] (nw[k], nsel, ncol), the bin fastest.  A copy: the values are the ones the integration sums.
struct BatchSpectraParams {
  int ncol, nsel, nl;
  const int *level;
  size_t src_stride;
  const double *src[4];
  double *dst[4];
  int nw[4];
};
// ... and k_pack_bounds the bounds blocks (bounds_layout) at blocks + c * its count: bounds_element of the caller's device
// arrays and the handle's device copies of its fields
struct PackBoundsParams {
  int ncol;
  BoundsLayout l;
  BoundsArrays in, own;
  double own_scale;
  double *blocks;
};
void launch_pack_columns(const PackParams &p, hipStream_t s);
void launch_pack_bounds(const PackBoundsParams &p, hipStream_t s);
void launch_batch_finish(const BatchFinishParams &p, hipStream_t s);
void launch_batch_spectra(const BatchSpectraParams &p, hipStream_t s);

// The response form's work arrays (ir_green.inc), per (bin, g-point) q
constexpr int GREEN_LB = 16;                 // levels per block of the far form
constexpr int GREEN_RW = 7;                  // per (q, row): c', 1/den, z, running products of phi and of -c' (mantissa, exponent each)
constexpr int GREEN_IS = 6;                  // per (q, level): above form (log, up, down) and below form
constexpr int GREEN_FS = 2 * GREEN_LB + 2;   // per (q, form, level block): reference log, pad, 16 (up factor, down factor) pairs
constexpr int GREEN_DS = 4 + 2 * 2;          // per (q, k): above amplitude, its log, below amplitude, its log, explicit values of the levels k and k + 1
constexpr int GREEN_D0 = 2 * 2;              // per q: level 0's explicit values (up, down) for k = 0, 1
// Which form a level takes for a deviation at k.  A unit change of bplanck[k] reaches the source terms of layers k-1 and
// k, i.e. the rows 2k-3 .. 2k+2 of E (those that exist); the levels k and k+1 (the bottoms of these two layers) and, for
// k <= 1, level 0 are evaluated explicitly; the levels above take the above form, those below the below form.
//   0 above, 1 below, 2 explicit (slot: 0 level k, 1 level k+1, 2 level 0)
__host__ __device__ inline int green_class(int lv, int k, int &slot) {
  slot = 0;
  if (lv >= k + 2) return 1;
  if (lv == 0 && k <= 1) { slot = 2; return 2; }
  if (lv <= k - 1) return 0;
  slot = lv - k;
  return 2;
}
// class of (deviation k, level block): 0 every level of the block takes the above form, 1 the below form, 2 mixed
__host__ __device__ inline int green_block_class(int k, int blk, int nz) {
  const int lv0 = blk * GREEN_LB, lv1 = lv0 + GREEN_LB - 1 < nz ? lv0 + GREEN_LB - 1 : nz;
  if (k >= 2 && lv1 <= k - 1) return 0;
  if (lv0 >= k + 2) return 1;
  return 2;
}

// The RCE Jacobian's batch as a response problem (ir_green.inc): columns that differ from a base profile in a few
// temperatures are F(base) + sum of unit responses times Planck differences.  q = (bin - ir_lo) * ng + g.
struct GreenParams {
  int nz, ng, n_ir, ir_lo, ir_start, NQ;
  const double *tau, *w0, *g, *wbin;       // opr (TOA-first layers), g-point weights
  const double *freq, *ir_freq;            // opacity grid [nw+1], IR channel [nw_ir+1]
  const double *emissivity;                // [nw_ir]
  int has_hard_surface;
  double ir_tau_min;
  // from the opacities alone (k_green_factor, k_green_unit, k_green_local), all q-major
  double *RW;                              // [NQ][7][2 nz] per row: c', 1/den, z, running products of phi and of -c' (mantissa, exponent)
  double *IS;                              // [NQ][6][nz+1]: per level, above form (log, up, down) and below form
  double *FS;                              // [NQ][2][blocks of 16 levels][34]: the same relative to a block's reference level
  double *DS;                              // [NQ][8][nz+1]: per k, (amplitude, log) pairs of the two forms, explicit values of the levels k, k+1
  double *D0;                              // [NQ][2][2]: level 0's explicit values (up, down) for k = 0, 1
  // deviations (sorted by k), padded to a multiple of 16
  int ndev, ndev_pad;
  const int *dev_k;
  const double *dev_T, *base_T;            // base_T[k], k TOA-first, k = nz: surface
  double *DB;                              // [n_ir][ndev_pad] + 64 doubles of slack (k_green_accum_far_mfma's tiles past the list)
  int qsplit;
  int nmix;                                // (deviation, level block) pairs of mixed class
  const int *mix_dev, *mix_blk;
  double *partial;                         // [qsplit][ndev_pad][2][nz+1] (levels TOA-first)
  int msplit;                              // bin splits of the mixed blocks' kernel
  double *partial_m;                       // [msplit][ndev_pad][2][nz+1]: its sums (only the mixed (deviation, level) pairs are written)
  // columns
  const int *col_src, *col_ptr, *col_dev;  // row of gen_out (or -1: base + responses), CSR of a column's deviations
  const double *gen_out;                   // [3][1 + dense columns][nz+1] (arrays gen_arr apart): column 0 = the base profile
  size_t gen_arr, out_arr;
  const double *flux_n;                    // the handle's level rows (solar rows of the last solar call)
  double *out;                             // [3][ncol][nz+1] (arrays out_arr apart)
};
// RW | IS | FS | DS | D0 of NQ (bin, g-point) pairs laid over `base`; count: doubles in all.  A null base gives the
// count alone.
struct GreenWork { double *RW, *IS, *FS, *DS, *D0; size_t count; };
inline GreenWork green_work_views(int nz, int NQ, double *base) {
  const size_t nl = (size_t)nz + 1, nblk = (nl + GREEN_LB - 1) / GREEN_LB;
  GreenWork v{};
  auto take = [&](size_t n) { double *p = base ? base + v.count : nullptr; v.count += n * NQ; return p; };
  v.RW = take(GREEN_RW * 2 * (size_t)nz); v.IS = take(GREEN_IS * nl); v.FS = take(2 * nblk * GREEN_FS);
  v.DS = take(GREEN_DS * nl); v.D0 = take(GREEN_D0);
  return v;
}
// the deviation list's padded length (the accumulation kernels take it in tiles of 16)
inline int green_ndev_pad(int ndev) { return ndev <= 16 ? 16 : (ndev + 15) / 16 * 16; }
void launch_green_factor(const GreenParams &p, hipStream_t s);
void launch_green_columns(const GreenParams &p, int ncol, hipStream_t s);
void launch_batch_ftotal(double *out, size_t out_arr, int ncol, int nz, const double *flux_n, hipStream_t s);
void launch_green_accumulate(const GreenParams &p, hipStream_t s);   // the accumulation alone (test hook: DB given)
void launch_green_jacobian(const GreenParams &p, hipStream_t s);     // Planck derivatives, accumulation, the three matrices
void launch_green_jacobian_reduced(const GreenParams &p, const int *row_lv, int nrow, int ngroup, bool parts, hipStream_t s);   // ... summed over groups of columns, rows picked
void launch_jacobian_total(double *jac, size_t arr, size_t n, hipStream_t s);
// Rows of the per-bin IR temperature Jacobian by adjoint solves (ir_adjoint.inc, radtran_ir_jacobian_spectral_rows): a
// block of its own beside the response form's.  `g` carries the opacities, the surface fields and base_T (null: unit
// amplitudes, the test hook) -- none of the response form's work arrays.  fun[f] = 2 level + (0 up | 1 down), levels
// TOA-first, the ndir directions of requested level a side by side at f = a ndir (dir0: the one direction of ndir = 1).
struct IrAdjointParams {
  GreenParams g;
  int nfun, nrow, ndir, dir0;
  const int *fun;
  double *work;                            // [NQ][4 + nfun][2 nz]: c', 1 / pivot, sub-diagonal, y, the functionals' lambdas
  double *part;                            // [NQ][nfun][nz+1]: a g-point's weighted row, levels TOA-first
  double *out_up, *out_dn;                 // (n_ir, nrow, nz+1), the bin fastest, x ground-first (null: not asked for)
};
// work rows of 2 nz doubles per q; doubles of `work` (then `part` behind it) in all
__host__ __device__ inline size_t adjoint_work_rows(int nfun) { return 4 + (size_t)nfun; }
inline size_t ir_adjoint_work_count(int nz, int NQ, int nfun) { return (size_t)NQ * adjoint_work_rows(nfun) * 2 * nz; }
inline size_t ir_adjoint_part_count(int nz, int NQ, int nfun) { return (size_t)NQ * nfun * (nz + 1); }
void launch_ir_adjoint(const IrAdjointParams &p, hipStream_t s);
// Gradient of a loss on the IR level fluxes in the stored tau, w0, g (ir_opr_sens.inc, radtran_ir_spectra_opr_vjp): one
// adjoint and one forward solve per (bin, g-point) on the adjoint's factors.  `g` carries the opacities and the surface
// fields as in IrAdjointParams (base_T is not read); the test hook gives `bplanck` in place of the temperatures.
struct IrOprParams {
  GreenParams g;
  const double *T, *Ts;                    // the column: (nz) ground-first layers, (1)
  const double *bplanck;                   // [nz+1] TOA-first, the same for every bin, or null: planck_fcn(avg_freq(bin), T)
  int nsel, gs_ld;                         // requested levels; the cotangent spectra's leading dimension (nw_ir)
  const int *level;                        // [nsel] TOA-first, 0..nz
  const double *gs_up, *gs_dn;             // (gs_ld, nsel) cotangents of the spectra, indexed by the IR channel's bin, or null
  const double *gn_up, *gn_dn;             // (nsel) cotangents of the sums over the bins (times the bin's width), or null
  double *work;                            // [NQ][OPR_WORK_ROWS][2 nz]: c', 1 / pivot, sub-diagonal, y / z, lambda, Y
  double *part_g;                          // [NQ][nz]: a g-point's part of grad_g
  double *grad_tau, *grad_w0, *grad_g;     // the optical properties' own layouts (radtran_opr_get), or null: not asked for
};
constexpr int OPR_WORK_ROWS = 6;
inline size_t ir_opr_work_count(int nz, int NQ) { return (size_t)NQ * OPR_WORK_ROWS * 2 * nz; }
inline size_t ir_opr_part_count(int nz, int NQ) { return (size_t)NQ * nz; }
void launch_ir_opr_sens(const IrOprParams &p, hipStream_t s);
// Gradient of a loss on the solar level values fup, fdn, amean in the stored tau, w0, g and in the surface albedo
// (sol_opr_sens.inc, radtran_sol_spectra_opr_vjp): one adjoint and one forward solve per (bin, g-point) whatever the
// numbers of zenith angles and levels.  q = (bin - sol_lo) * ng + g; the per-bin arrays are indexed by the solar channel's bin.
struct SolOprParams {
  int nz, ng, n_sol, sol_lo, sol_start, NQ;  // this launch's solar bins sol_lo ..; channel -> opacity-bin offset
  int nzen;
  const double *tau, *w0, *g, *wbin;       // opr (TOA-first layers), g-point weights
  const double *zen_u, *zen_w, *zen_iu;    // [nzen] each: u0, its weight, 1 / u0
  const double *albedo;                    // [nw_sol]
  const double *photons_sol;               // [nw_sol], unscaled
  const double *am_f1, *am_f2, *am_dw;     // per solar bin amean unit factors (radiate.f90:174-178)
  double scale;                            // photon scale factor x diurnal_fac
  const double *sol_freq;                  // solar channel [nw_sol+1] (the widths of the sums' cotangents)
  int nsel, gs_ld;                         // requested levels; the cotangent spectra's leading dimension (nw_sol)
  const int *level;                        // [nsel] TOA-first, 0..nz
  const double *gs_up, *gs_dn, *gs_am;     // (gs_ld, nsel) cotangents of the three spectra, or null
  const double *gn_up, *gn_dn;             // (nsel) cotangents of the sums over the bins (times the bin's width), or null
  double *work;                            // [NQ][SOL_OPR_WORK_ROWS][2 nz]: k_opr_adjoint's six rows, (cp0 | cpb), (cm0 | cmb), (tauc | direct)
  double *part_g, *part_alb;               // [NQ][nz], [NQ]: a g-point's part of grad_g and of grad_albedo
  double *grad_tau, *grad_w0, *grad_g;     // the optical properties' own layouts (radtran_opr_get), or null: not asked for
  double *grad_albedo;                     // [nw_sol], or null
};
constexpr int SOL_OPR_WORK_ROWS = 9;
inline size_t sol_opr_work_count(int nz, int NQ) { return (size_t)NQ * SOL_OPR_WORK_ROWS * 2 * nz; }
inline size_t sol_opr_part_count(int nz, int NQ) { return (size_t)NQ * (nz + 1); }
void launch_sol_opr_sens(const SolOprParams &p, hipStream_t s);
// IR spectra of many temperature profiles from the adjoint's unit-amplitude rows (ir_rows_apply.inc,
// radtran_ir_spectra_batch): f(bin, a, c) = sum over j of w(bin, a, j) B(avg_freq(bin), x_c(j)).  The ndir directions
// asked for stand at places 0 and 1 (w0 / out0 / fn0, then w1 / out1 / fn1); functional F = place nsel + a.
struct IrRowsApplyParams {
  int n_ir, nsel, nz, ncol, ndir, F0;      // F0: the pass's first functional (the launcher's)
  int l0, ir_lo;                           // opacity-grid bin of the first IR bin here; its place in the IR channel
  const double *freq, *ir_freq;            // opacity grid [nw+1], IR channel [nw_ir+1]
  const double *T, *Ts;                    // (nz, ncol) ground-first layers, (ncol)
  const double *w0, *w1;                   // (n_ir, nsel, nz+1), the bin fastest, j ground-first
  double *out0, *out1;                     // (n_ir, nsel, ncol)
  double *fn0, *fn1;                       // (nsel, ncol): out summed over the bins times their widths (null: not asked for)
};
void launch_ir_rows_apply(const IrRowsApplyParams &p, hipStream_t s);
int ir_rows_column_tile(int ncol);         // the launcher's rule: columns per wave
// Temperature gradient of that batch (ir_rows_vjp.inc, radtran_ir_spectra_batch_vjp): with gs the cotangent of out and gn
// that of fn (either null: 0),  grad_x(j, c) = sum over d, a, l of (gs_d(l, a, c) + gn_d(a, c) (ir_freq(l) - ir_freq(l+1)))
// w_d(l, a, j) dB/dT(avg_freq(l), x_c(j)).  The ndir directions that have a cotangent stand at places 0 and 1, as above.
struct IrRowsVjpParams {
  int n_ir, nsel, nz, ncol, ndir;
  int l0, ir_lo;                           // as in IrRowsApplyParams
  const double *freq, *ir_freq;
  const double *T, *Ts;                    // (nz, ncol) ground-first layers, (ncol)
  const double *w0, *w1;                   // (n_ir, nsel, nz+1)
  const double *gs0, *gs1;                 // (n_ir, nsel, ncol) or null
  const double *gn0, *gn1;                 // (nsel, ncol) or null
  double *grad_T, *grad_Ts;                // (nz, ncol), (ncol): every element is written
};
void launch_ir_rows_vjp(const IrRowsVjpParams &p, hipStream_t s);
int ir_rows_vjp_column_tile(int ncol);     // the launcher's rule: columns per wave
int green_far_resident_waves();
void green_vector_form_set(int vector_form);   // test hook: the far accumulation's vector form (1) or matrix form (0)
int green_far_waves(int ndev, int nl);   // per bin split
int green_far_splits(int n_ir, int waves);

// ---- what a handle holds between calls, stated once (host only, no HIP call: clima_test_handle_holds replays it without
// a device).  The member functions are the transitions and the only writers of the fields; refused() alone says what
// cannot run on what is held.  After a batch the handle holds what n single calls would have left, but for the column
// and, after one launch per chunk, the optical properties (they stayed in the arena).  DESIGN.md section 4: the table ----
struct Holds {
  bool column = false, column_particles = false;   // the resident column (d_col): loaded, given with particles
  long uploads = 0;                                // ... columns uploaded so far
  bool opr = false, w0_stored = true;   // the handle's own optical-property block: valid; w0 stored, or still to be formed from scat (ensure_w0)
  long opr_upload = 0;                  // ... the upload it was computed from
  int opr_lo = 0, opr_n = 0;            // ... the opacity bins [opr_lo, opr_lo + opr_n) it was computed for
  bool rows_on_host = false, rows_in_pinned = false;   // the level rows: h_small is current; the last integration stored them there itself
  bool rows = false;                                   // ... some call has left level rows on the handle at all
  // Two call slots (the handle's buffer members ARE the current slot's): whether work enqueued on
  // the other one's stream has not been joined yet, and whether the previous call was a pipelined resident call that
  // nobody has waited for or joined since (only then may the next one take the other slot)
  bool other_in_flight = false, unjoined = false;
  long overlapped = 0;                                 // calls enqueued on a slot while the other's call had not been joined

  void call_pipelined(bool took_other) {               // a resident call that may have a successor beside it
    if (took_other) { other_in_flight = true; overlapped++; }
    unjoined = true;
  }
  void joined() { other_in_flight = false; unjoined = false; }

  void uploaded(bool has_particles) { column = true; column_particles = has_particles; uploads++; }
  void opacities_written(bool own_block, bool w0, bool from_resident, int lo, int n) {
    if (!own_block) return;   // (a chunk of a one-launch batch wrote the arena's blocks)
    opr = true; w0_stored = w0; opr_lo = lo; opr_n = n;
    if (from_resident) opr_upload = uploads;
  }
  void w0_formed() { w0_stored = true; }
  void rows_enqueued(bool in_pinned) { rows = true; rows_on_host = false; rows_in_pinned = in_pinned; }
  void rows_changed() { rows = true; rows_on_host = rows_in_pinned = false; }   // on the device, behind the host's back: fetch them
  void rows_fetched() { rows_on_host = true; }
  void batch_left(bool one_launch, int np) { column = false; column_particles = np > 0; opr = !one_launch; }
  void batch_repeated() { opr = true; }                     // one call per column: the handle's own block holds the last column's
  void results_dropped() { rows_changed(); rows = false; opr = false; }   // a graph replay: nothing on the handle is a call's result
  bool opr_from_resident_column() const { return opr_upload == uploads; }
};
enum { NEED_COLUMN = 1, NEED_OPACITIES = 2, NEED_SPECTRUM = 4 };
// What keeps a call with these needs from running on the shard's opacity bins [op_lo, op_lo + op_n) (null: nothing); a
// text that begins with a blank follows the entry point's name.  Opacities: valid AND computed for the bins asked for.
inline const char *refused(const Holds &h, int needs, int shard_world, bool has_comm, int op_lo, int op_n) {
  if ((needs & NEED_COLUMN) && !h.column) return "no column has been uploaded";
  if ((needs & NEED_OPACITIES) && !(h.opr && op_lo >= h.opr_lo && op_lo + op_n <= h.opr_lo + h.opr_n))
    return " needs opacities: call radiate with compute_opacity first";
  if ((needs & NEED_SPECTRUM) && shard_world != 1 && !has_comm) return " is not available on a bin-sharded handle";
  return nullptr;
}

// ---- the launch plan of one radiate call: decided once by plan_radiate (kernels.hip, beside the kernels whose limits
// it applies), executed by the launchers, which decide nothing ----
struct PlanIn {
  // the call
  int nz, ng, nzen;
  int n_ir, n_sol, op_n;   // this rank's bins (n_sol = 0: a call without solar fluxes)
  int nsrc;                // source layers of the column; nz for a batch (upper bound)
  int ncol;                // columns in the launch
  bool batch;              // ... of a one-launch batch (radtran_toa_fluxes_batch)
  bool ir_batch;           // temperature columns on the stored opacities (radiate_ir_batch's general form): the wave forms
                           // whatever the block-mode switch says, and the caller clears the per-column spectra
  int rebin_mode;
  bool cust_on, compute_opacity;
  bool all_pairs;          // the call computes its opacities from a column of exact pairs (the doubled radiative grid)
  // the handle's and the process's switches
  bool fused, allow_fused, ts_block_mode, no_half;
  long coop_items;
  int force_slots;         // test hook: whole-wave slots above ceil(nz/64); rules out the half-wave kernel
};
enum { OP_NONE = 0, OP_TILE, OP_COOP, OP_UNSUPPORTED };   // stored opacities | lane per item | group of lanes
enum { TS_NONE = 0, TS_WAVE, TS_HALF, TS_PAIRED, TS_BLOCK };          // whole wave | half wave | exact pairs (fused grid only) | workgroup per bin
struct TsPlan {
  int form;
  int slots;               // layers per lane (TS_BLOCK: chunks per g-point column)
  int cols;                // g-point columns per workgroup
  int groups, per_launch;  // g-point groups of a bin (> 1: their partial sums are ADDED into cleared outputs), groups per launch
  int threads;             // TS_BLOCK
  size_t lds;              // dynamic LDS bytes
  bool zero_launch;        // a k_zero launch clears the outputs first
};
struct LaunchPlan {
  int opacity, coop_ng;    // OP_*, lanes per item of the group-of-lanes kernel (8, 16, 32)
  TsPlan fused;            // TS_NONE: separate launches
  TsPlan ts;               // the stand-alone wave forms: when no fused grid runs (or the runtime refuses it its LDS); TS_NONE: none applies
  TsPlan block;            // the workgroup-per-bin form: when no wave form runs; TS_NONE: the column does not fit
  bool prep_clears;        // spare blocks of the prep launch clear the outputs
  bool caller_clears;      // ir_batch: the caller clears its per-column spectra
  bool write_w0;           // the opacity tiles store w0 (false: the fused grid's two-stream part forms it from scat)
};
LaunchPlan plan_radiate(const PlanIn &in);
// the ranges a form that adds partial sums needs cleared: this launch's bins of the five spectra; returns their number
int ts_clear_ranges(const TwoStreamParams &p, double *ptr[6], size_t count[6]);

// launchers (kernels.hip): they take their part of the plan, pick the kernel, fill the fields marked (launcher) and launch
void launch_prep(const PrepParams &p, hipStream_t s);
// false: OP_UNSUPPORTED (the compiled kernels cover 1..32 g-points)
bool launch_opacity(const OpacityParams &p, const LaunchPlan &pl, hipStream_t s);
// false: the plan has no such form, or the runtime refused the kernel its dynamic LDS (the caller goes on to the next form)
bool launch_twostream(TwoStreamParams &p, const TsPlan &t, hipStream_t s);
bool launch_twostream_w(TwoStreamParams &p, const TsPlan &t, hipStream_t s);
// T + c*b_T, T_surface + c*b_Ts, IR spectra + c*b_out for column c of ncol
bool launch_twostream_ir_batch(TwoStreamParams &p, int ncol, hipStream_t s, int force_nw = 0);
// Illumination cases on the stored opacities (k_twostream_sol_batch, solar_batch.inc): a block of its own, so that
// TwoStreamParams and the kernels that take it stay what they are.  Case c reads zen + c * 3 * nzen ([u0 | weight | 1/u0]
// [nzen]), albedo + c * alb_stride ([nw_sol], the channel's bin order; stride 0: one albedo for every case) and scale[c],
// and writes its three spectra ([nw_sol][nz+1], ground-first) at out_stride doubles from the previous case's.
struct SolBatchParams {
  int nz, ng;
  int n_sol, sol_lo, sol_start;            // blocks = solar bins sol_lo .. ; channel -> opacity-bin offset
  int ncase, nzen;
  int cases_per_block;                     // (launcher)
  const double *tau, *w0, *g, *wbin;       // opr, g-point weights
  const double *zen, *albedo, *scale;
  size_t alb_stride;
  const double *photons_sol;               // [nw_sol], unscaled
  const double *am_f1, *am_f2, *am_dw;     // per solar bin amean unit factors (radiate.f90:174-178)
  double diurnal_fac;
  double *fup, *fdn, *amean;
  size_t out_stride;
};
// false: outside what the kernel covers (nz > 512, nzen > MAX_ZEN, LDS); force_nw = 4: blocks of four waves at every slot count
bool launch_twostream_sol_batch(SolBatchParams &p, hipStream_t s, int force_nw = 0);
int solar_batch_cases_per_block(int ncase);   // the launcher's rule (tests size their batches by it)
int fused_tiles(const OpacityParams &op);   // opacity tiles per column (size of a column's done[] slice)
bool launch_fused(const OpacityParams &op, TwoStreamParams ts, FusedParams fp, const TsPlan &f, hipStream_t s);
// the same three launchers for a launch with bounds blocks (TwoStreamParams::bounds; kernels_bounds.hip): launch_fused,
// launch_twostream_w and launch_twostream hand such a launch on to them
bool launch_fused_bounds(const OpacityParams &op, TwoStreamParams ts, FusedParams fp, const TsPlan &f, hipStream_t s);
bool launch_twostream_w_bounds(TwoStreamParams &p, const TsPlan &t, hipStream_t s);
bool launch_twostream_bounds(TwoStreamParams &p, const TsPlan &t, hipStream_t s);
// test hook: the two-stream blocks of the fused grid alone (no opacity blocks), on opacities already in HBM
// (meta_nsrc: a device int, any value >= 1)
bool launch_fused_twostream_only(TwoStreamParams &ts, int slots, const int *meta_nsrc, hipStream_t s, bool half = false, bool paired = false);
void launch_integrate(const IntegrateParams &p, hipStream_t s);
// what launch_integrate launches where integrate_fits_one_launch() does not hold (k_integrate_partial, k_integrate_final)
void launch_integrate_two(const IntegrateParams &p, hipStream_t s);
// one call's integration and the next call's prep pass as ONE grid (k_prep_integrate), where prep_integrate_merges() holds
bool prep_integrate_merges(const PrepParams &pp, const IntegrateParams &ip);
void launch_prep_integrate(const PrepParams &pp, const IntegrateParams &ip, hipStream_t s);
void launch_integrate_batch(const BatchIntegrateParams &p, int ncol, hipStream_t s);
void launch_scale(double *a, size_t n, double f, hipStream_t s);
void launch_copy(double *dst, const double *src, size_t n, hipStream_t s);  // src may be pinned host memory
void launch_test_rcp(const double *x, double *y, int n, hipStream_t s);
void launch_test_wscan(const double *a, const double *b, double *out, int nwaves, hipStream_t s);
void launch_w0_from_scat(const double *tau, const double *scat, double *w0, int nw, int ng, int nz, hipStream_t s);
void launch_test_exp(const double *x, double *y, int n, hipStream_t s);
void launch_test_exp_tab(const double *x, double *y, int n, int base10, hipStream_t s);

}  // namespace clima
