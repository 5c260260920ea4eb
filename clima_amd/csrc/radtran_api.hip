// radtran_api.hip -- host side of the C ABI declared in include/clima_radtran_hip.h.
//
// Mirrors `type Radtran` (src/radtran/clima_radtran.f90:31-85): the handle owns the
// tables and work arrays in HBM, a HIP stream, and host mirrors of the small results.
// There is no CPU fallback anywhere in this file: if HIP is unavailable every compute
// entry point reports the HIP error in `err`.
#include "../../include/clima_radtran_hip.h"
#include "radtran_dev.h"

#include <rccl/rccl.h>   // the bin-sharded step's one collective; backend "nccl" on ROCm IS RCCL
#include <sys/stat.h>
#include <unistd.h>
#include <ctime>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <utility>
#include <limits>
#include <vector>

using namespace clima;

namespace {

constexpr unsigned MAGIC = 0xC11AAD17u;

void set_err(char *err, const std::string &msg) {
  if (!err) return;
  std::strncpy(err, msg.c_str(), CLIMA_ERR_LEN);
  err[CLIMA_ERR_LEN] = 0;
}
void clear_err(char *err) {
  if (err) err[0] = 0;
}

struct HipFail {
  std::string msg;
};
#define HIPCHK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      throw HipFail{std::string("HIP error in " #call ": ") + hipGetErrorString(e_)};        \
  } while (0)
#define NCCLCHK(call)                                                                        \
  do {                                                                                       \
    ncclResult_t e_ = (call);                                                                \
    if (e_ != ncclSuccess)                                                                   \
      throw HipFail{std::string("RCCL error in " #call ": ") + ncclGetErrorString(e_)};      \
  } while (0)

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  bool owned = true;
  void view(T *ptr, size_t count) {  // a window into another buffer (not freed here)
    release();
    p = ptr; n = count; owned = false;
  }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) HIPCHK(hipMalloc((void **)&p, count * sizeof(T)));
  }
  bool reserve(size_t count) {  // grow-only; true: a new allocation (its contents undefined)
    const bool grow = n < count;
    if (grow) alloc(count);
    return grow;
  }
  void upload(const std::vector<T> &v) {
    if (!(p && owned && n == v.size())) alloc(v.size());   // (same size: the allocation is kept)
    if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  void zero(hipStream_t s = nullptr) {
    if (n) HIPCHK(hipMemsetAsync(p, 0, n * sizeof(T), s));
  }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    n = 0;
    owned = true;
  }
  void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(owned, o.owned); }   // (no copy: each allocation keeps one owner)
  ~DevBuf() { release(); }
};

// Pinned host memory that only grows: at least `count` elements, `count + spare` when it has to be allocated anew
template <class T>
struct PinnedBuf {
  T *p = nullptr;
  size_t n = 0;
  T *reserve(size_t count, size_t spare = 0) {
    if (n < count) {
      if (p) (void)hipHostFree(p);
      p = nullptr; n = 0;
      HIPCHK(hipHostMalloc((void **)&p, sizeof(T) * (count + spare), hipHostMallocDefault));
      n = count + spare;
    }
    return p;
  }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

struct KTabHost {
  int sp, ng, nP, nT;
  std::vector<double> weights, log10P, temp, log10k;
  DevBuf<double> d_log10k, d_log10P, d_temp;
};
struct XsHost {
  int type, dim, sp1, sp2, nT;
  std::vector<double> temp, data;
  DevBuf<double> d_data, d_temp;
};
struct PartHost {
  int p_ind, nrad;
  std::vector<double> radii, w0, qext, gt;
  DevBuf<double> d_radii, d_w0, d_qext, d_gt;
};

struct Radtran;
struct ChannelObj {  // RTChannel, clima_radtran_types.f90:263-269
  Radtran *parent = nullptr;
  int which = 0;
  int ind_start = 0, ind_end = -1, nw = 0;  // 0-based, inclusive end
  std::vector<double> wavl, freq;
  DevBuf<double> d_freq;
};
struct WrkObj {  // ClimaRadtranWrk, clima_radtran.f90:11-25
  Radtran *parent = nullptr;
  int which = 0;
  DevBuf<double> fup_a, fdn_a, amean, tau_band;
};

// A column batch in flight (radtran_toa_fluxes_batch and its device-array form): the launch form batch_form decided
// for its n columns, once -- one launch of each kernel per chunk of CH columns, or the columns' calls back to back --,
// the id of its first call, and its sink: the caller's device arrays (k_batch_finish forms f_total / ISR / OLR
// there), or `rows`, n blocks [5][nz+1] on the host (which forms them itself).
// The spectral sinks (radtran_toa_fluxes_batch_spectra and its device-array form; nsel = 0: none): the rows
// spec_level[0 .. nsel) (device, 0-based, ground-first) of every column's ir fup_a / ir fdn_a / sol fup_a / sol fdn_a
// go to spec[k] (device, (nw, nsel, n); null: not wanted) -- the caller's arrays, or, with `rows`, slices of the
// handle's staging buffer, whose spec_count doubles come back into spec_host beside the rows.
// A bounds batch (radtran_toa_fluxes_batch_bounds): `bounds`, its n bounds blocks (bounds_layout) behind the column
// blocks in d_cols_arena, where they stay for a repeat; null: every column under the handle's fields.
struct BatchRun {
  int n = 0, first_call = 0, CH = 0;
  bool one_launch = false, pending = false;
  double *ISR = nullptr, *OLR = nullptr, *fluxes = nullptr;
  double *rows = nullptr;
  const double *bounds = nullptr;
  size_t bounds_count = 0;   // doubles per block, as laid out when the batch was enqueued (a repeat steps by the same)
  int nsel = 0;
  const int *spec_level = nullptr;
  double *spec[4] = {nullptr, nullptr, nullptr, nullptr};
  double *spec_host = nullptr;
  size_t spec_count = 0;
};

// The buffers of the call slot that is NOT the handle's current one ("Two resident calls in
// flight"): everything a resident call writes.  The current slot's are the handle's own members of the same names;
// swap_slot() exchanges the two sets, so every entry point sees "the handle's buffers" whichever slot the last call took.
// Allocated (ensure_other_slot) the first time an upload or a call goes there.
struct CallSlot {
  bool allocated = false;
  DevBuf<double> d_col, d_prep, d_opr, d_tau, d_w0, d_g, d_tau_band, d_scat;
  DevBuf<double> spec[8];    // wrk_ir, then wrk_sol: fup_a, fdn_a, amean, tau_band
  DevBuf<double> d_small, d_flux_n;
  DevBuf<int> d_done;
  long col_upload = 0;       // the upload (Holds::uploads) its column block holds
  // the integration its latest call kept back (Radtran::int_pending): plain device pointers into the buffers above, which
  // swap_slot hands over without moving memory
  bool int_pending = false, pending_pipelined = false;
  IntegrateParams pending_ip;
};

struct Radtran {
  unsigned magic = MAGIC;
  int state = 0;  // 0 allocated, 1 begun, 2 finalized
  int nz = 0, nsp = 0, np = 0, nw = 0, ng = 0;
  std::vector<double> wavl, freq;
  std::vector<KTabHost *> k;
  std::vector<XsHost *> cia, ray, pxs;
  std::vector<PartHost *> part;
  std::vector<int> part_slot;
  bool has_cont = false;
  int LH2O = -1, cont_nT = 0;
  std::vector<double> cont_temp, cont_H2O, cont_foreign;
  DevBuf<double> d_cont_temp, d_cont_H2O, d_cont_foreign;
  std::vector<double> wbin, wbin_e, wxy;
  DevBuf<double> d_wbin, d_wbin_e, d_wbin_e_pad, d_wxy, d_freq, d_rorr_tab;
  ChannelObj ir, sol;
  WrkObj wrk_ir, wrk_sol;
  // public fields (clima_radtran.f90:51-68)
  double diurnal_fac = 0.5;
  std::vector<double> zenith_u, zenith_w, surface_albedo, surface_emissivity, photons_sol;
  bool has_hard_surface = true;
  double ir_tau_min = 1.0e-6;
  double photon_scale_factor = 1.0;
  bool fields_dirty = true;
  DevBuf<double> d_zen_u, d_zen_w, d_zen_iu, d_partial, d_albedo, d_emis, d_photons, d_am_f1, d_am_f2, d_am_dw;
  // column + prep
  int nslots = 0;
  // names for opacities2yaml (the loaders know them; optional: radtran_set_names / radtran_set_opacity_labels)
  std::vector<std::string> species_names, particle_names, particle_data;
  std::string k_method_name = "RandomOverlapResortRebin", continuum_model = "MT_CKD";
  std::vector<SlotDev> slots;
  // custom optical properties (types.f90:432-548): tables [nw][nP] on the device, axis log10(P cgs) ascending
  bool cust_on = false;
  int cust_nP = 0;
  std::vector<double> cust_axis;
  DevBuf<double> d_cust_axis, d_cust_dtau, d_cust_w0, d_cust_g0;
  // batched shared-opacity IR calls (radtran_radiate_ir_batch)
  DevBuf<double> d_bT, d_bTs, d_bup, d_bdn, d_bpartial, d_bout;
  // ... and its response form (ir_green.inc): work arrays, deviation lists, the general sub-batch's rows
  DevBuf<double> d_green, d_green_acc, d_green_in, d_gen_out;
  int green_last_n = -1;           // columns of the last batch, when it took the response form (the next one of that size starts its opacity-only part early)
  PinnedBuf<double> h_bout;        // the batch's three result arrays on their way to the caller's
  PinnedBuf<char> h_green;         // what the host hands the response form (base profile, deviation lists)
  DevBuf<int> d_green_idx;
  DevBuf<double> d_adjoint;        // the adjoint rows' work buffer (radtran_ir_jacobian_spectral_rows, ir_adjoint.inc)
  DevBuf<double> d_rows_w, d_rows_out;   // radtran_ir_spectra_batch: the weights of both directions; a chunk's spectra and sums
  // illumination cases on the stored opacities (radtran_radiate_solar_batch): the cases' inputs, the spectra of the cases
  // in flight, a place for the per-case form's copy of the band optical depth
  DevBuf<double> d_sb_in, d_sb_spec, d_sb_band;
  bool solar_batch_shared = true;        // radtran_solar_batch_shared_set: 0 forces one full solve per case
  long solar_batch_shared_batches = 0;   // batches that took k_twostream_sol_batch (radtran_solar_batch_shared_get)
  int ir_green_mode = 1;           // CLIMA_HIP_IR_GREEN: 0 never, 1 when enough columns are sparse deviations of one profile, 2 whenever any is
  long ir_green_batches = 0;       // batches that took the response form (radtran_ir_green_batches_get)
  DevBuf<double> d_col;  // one column block
  ColumnLayout col_layout{};   // ... as column_layout(nz, nsp, np) lays it out
  int nsrc = 0;          // source layers of the resident column (pair_reuse decided at upload)
  bool all_pairs_exact = false;  // ... and every layer is half of an exact pair (the doubled radiative grid)
  DevBuf<double> d_prep;  // one block: [log10P | cols | foreign_col | absw | q | ix (ints)]
  size_t prep_count = 0;
  std::vector<AbsEntry> abs_entries;  // continuum terms in the reference's summation order (+ zero-weight padding)
  DevBuf<double> d_zero_xs;
  DevBuf<int> d_err;
#ifdef CLIMA_STAMPS
  DevBuf<long long> d_stamps;
#endif
  double *h_col = nullptr;  // pinned staging
  double *h_col_dev = nullptr;  // the same buffer as the device addresses it (null: not mapped, use the copy engine)
  hipEvent_t ev_upload = nullptr;   // marks the end of the last column copy out of the pinned staging buffer
  bool upload_pending = false;
  int call_id = 0, checked_id = 0;  // opacity passes enqueued / already checked for device errors
  Holds holds;                      // what the handle holds between calls: the column, its own optical properties, the level rows
  std::string deferred_err;         // a failure met inside a getter without an `err` argument: reported by the next call that has one
  // fused hand-off (k_fused): bound of a two-stream block's wait, the last timed-out pass already
  // handled, the pass of the last solar computation, flags of the last call, re-issued calls so far
  int fused_max_spins = 400000, checked_timeout = 0, solar_id = 0, fused_fallbacks = 0;
  bool last_cs = true;
  std::vector<double> last_T, last_P, last_radii;  // host copy for byte accounting
  // opr: one block [tau | w0 | g | tau_band | scat] (opr_views); the five are views into it
  DevBuf<double> d_opr;
  size_t opr_count = 0;
  DevBuf<double> d_tau, d_w0, d_g, d_tau_band, d_scat;
  // results
  LevelRows rows{};           // level_rows(nz): the layout of d_small, h_small and a column's slice of d_flux_arena
  DevBuf<double> d_small;     // one level-row block: one D2H copy per call
  DevBuf<double> d_flux_n;    // view into d_small: its four flux rows
  std::vector<std::pair<void *, size_t>> host_registered;   // caller arrays page-locked by radtran_spectra_get_all / radtran_radiate_ir_batch
  double *batch_out[3] = {nullptr, nullptr, nullptr};       // the result arrays of the last radtran_radiate_ir_batch call
  size_t batch_out_n = 0;
  static constexpr int batch_shared_min = 2;                // batches of at most so many columns take the per-column kernel
  bool batch_pin_results = false;                           // radtran_batch_pin_results_set
  hipEvent_t bout_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // the batch's result pieces
  hipStream_t copy_streams[3] = {nullptr, nullptr, nullptr}; // radtran_spectra_get_all: the seven copies go out over four queues
  double *h_small = nullptr;  // pinned: d_small's block on the host
  double *h_small_dev = nullptr;   // the same block as the device addresses it (null: not mapped)
  int *h_errflag = nullptr;
  // sharding
  DevBuf<double> d_flux_part;  // this rank's partial level rows (d_flux_n is all-reduced in place)
  int shard_rank = 0, shard_world = 1;
  // the library's own multi-GPU step (radtran_comm_init_rank): with a communicator every radiate() ends with ONE
  // ncclAllReduce of the partial level fluxes and one status word (rows.reduce_count) on the handle's stream
  ncclComm_t comm = nullptr;
  int comm_n = 1, comm_rank = 0, device = 0;
  long comm_reduces = 0;       // all-reduces enqueued so far (tests)
  double comm_status = 0.0;    // the reduced status word of the last fetched step (see IntegrateParams::timeout_out)
  int op_lo = 0, op_n = 0, ir_lo = 0, ir_n = 0, sol_lo = 0, sol_n = 0;
  // stream + profiling
  hipStream_t stream = nullptr;
  // column batches (radtran_toa_fluxes_batch): every column's block, every column's level rows (rows.stride each)
  DevBuf<double> d_cols_arena, d_flux_arena;
  // one-launch batches: per-column prep / opr / spectra blocks for the columns in flight
  DevBuf<double> d_prep_arena, d_opr_arena, d_res_arena;
  int batch_cols_in_flight = 64;
  // A batch out of device arrays (radtran_toa_fluxes_batch_device) returns with its work enqueued: its settle_batch
  // is due at the next settle_device_batch().  A repeat reads the column blocks still in d_cols_arena and writes the
  // caller's same result arrays.
  BatchRun dev_batch;
  // a batch's spectral sinks: its level list (0-based; staged once per batch), the host form's rows on their way out
  std::vector<int> spec_level;
  DevBuf<int> d_spec_level;
  DevBuf<double> d_spec_stage;
  PinnedBuf<double> h_spec;
  DevBuf<int> d_batch_nsrc;        // every column's source-layer count, as k_pack_columns found it
  std::vector<int> batch_nsrc;     // ... on the host: pack_column's, or fetched (only before one call per column: those launches are sized by it)
  hipEvent_t ev_producer = nullptr;   // orders the handle's stream behind the stream that wrote a device batch's inputs
  bool batch_shared = true;        // radiate_ir_batch: temperature-independent work shared by the columns (CLIMA_HIP_BATCH_SHARED=0: one full solve per column)
  int rebin_mode = 1;              // 0 window form, 1 streaming, 2 streaming multi-edge (rebin_mode_for)
  bool rebin_stream = false;       // CLIMA_HIP_REBIN=stream when the handle was made: never the window form
  long coop_items = 34816;         // ng = 8: at most this many (bin, source layer) items go to k_opacity_coop<8> (CLIMA_HIP_COOP_ITEMS)
  bool fused = true;               // opacity + two-stream in one grid (k_fused); CLIMA_HIP_FUSED=0 or radtran_fused_set turns it off
  bool ts_block_mode = false;      // CLIMA_HIP_TS_MODE=block when the handle was made: the workgroup-per-bin two-stream kernel
  DevBuf<int> d_done;              // per opacity block: call id of its last completed run
  // A resident call that returns with nobody reading its results keeps its frequency integration back (pending_ip): the
  // next compute_opacity call launches it in one grid with its own prep pass (k_prep_integrate), anything else launches
  // it first as it is (resolve_pending_integration).  A pending integration belongs to its call slot: these are the
  // current slot's, `other` holds the second pair, swap_slot exchanges them.  pending_pipelined: kept back by a call of a
  // handle that pipelines two -- the next call into this slot, two calls on, takes it along on the slot's lane.
  bool defer_integration = true;   // radtran_defer_integration_set
  bool flux_ptr_taken = false;     // radtran_flux_device_ptr was called: its caller reads d_small in stream order, unannounced
  bool int_pending = false, pending_pipelined = false;
  IntegrateParams pending_ip;
  long merged_integrations = 0, standalone_integrations = 0;   // pending integrations resolved either way (radtran_merged_integrations_get)
  // Two resident calls in flight: consecutive pipelined calls alternate between the two call slots, each on a lane
  // (stream) of its own -- lane 0 is `stream`, the one every other entry point works on; lane 1 exists once a call has
  // gone there.  `stream` names the lane being enqueued on: lane 0 except inside a LaneScope.
  int calls_in_flight = 0;         // radtran_calls_in_flight_set: 0 automatic, 1 one at a time, 2 two whenever eligible
  CallSlot other;                  // the slot that is not current
  long col_upload = 0;             // the upload the current slot's column block holds
  hipStream_t lane_stream[2] = {nullptr, nullptr};
  int lane = 0;                    // lane of the latest pipelined call (0 after a join)
  bool on_other_lane = false;      // a call is being enqueued beside the previous one: nothing joins inside it
  hipEvent_t ev_lane1 = nullptr;   // behind the latest work of lane 1: what a join makes lane 0 wait for
  hipEvent_t ev_fence = nullptr;   // lane 0 at the last join: lane 1 waits for it before it reuses a slot lane 0 worked in
  hipEvent_t ev_colcopy = nullptr; // behind a slot-to-slot copy of the column: an upload into the block it read waits for it
  bool fence_due = false, colcopy_pending = false;
  const double *colcopy_src = nullptr;   // the block that copy read
  int cus = 0;                     // compute units of the device (the automatic rule's measure of one residency round)
  int profile = 0;  // 0 off, 1 HIP events around every kernel, 2 around the dominant kernel (id 1) only
  long timer_calls = 0;
  int profile_stride = 1;   // events on every profile_stride-th call only (bounds the cost of measuring)
  struct Ev { hipEvent_t a, b; int id; };
  std::vector<Ev> pending;
  std::vector<hipEvent_t> pool;
  double k_ms[7] = {0, 0, 0, 0, 0, 0, 0};
  int k_n[7] = {0, 0, 0, 0, 0, 0, 0};

  ~Radtran() {
    for (auto *x : k) delete x;
    for (auto *x : cia) delete x;
    for (auto *x : ray) delete x;
    for (auto *x : pxs) delete x;
    for (auto *x : part) delete x;
    for (auto &e : pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : pool) (void)hipEventDestroy(e);
    if (h_col) (void)hipHostFree(h_col);
    for (auto &e : host_registered) (void)hipHostUnregister(e.first);
    for (auto &cs : copy_streams) if (cs) (void)hipStreamDestroy(cs);
    for (auto &e : bout_ev) if (e) (void)hipEventDestroy(e);
    if (h_small) (void)hipHostFree(h_small);
    if (ev_upload) (void)hipEventDestroy(ev_upload);
    if (ev_producer) (void)hipEventDestroy(ev_producer);
    if (comm) (void)ncclCommDestroy(comm);
    // (an integration still pending, in either slot, is dropped: nobody is left to read its rows)
    for (hipEvent_t e : {ev_lane1, ev_fence, ev_colcopy}) if (e) (void)hipEventDestroy(e);
    if (lane_stream[1]) { (void)hipStreamSynchronize(lane_stream[1]); (void)hipStreamDestroy(lane_stream[1]); }   // (its kernels write the other slot's buffers, freed below)
    if (lane_stream[0]) stream = lane_stream[0];
    if (stream) (void)hipStreamDestroy(stream);
    magic = 0;
  }
};

Radtran *as_rad(void *ptr) {
  Radtran *r = reinterpret_cast<Radtran *>(ptr);
  if (!r || r->magic != MAGIC) return nullptr;
  return r;
}

// ---- two resident calls in flight: the slots and the lanes ----
// THE join: lane 0 -- the stream every entry point but a pipelined resident call works on -- is ordered behind what lane 1
// has been given, by an event and a stream wait, never by a host wait.  Called where the handle's debts are resolved
// (settle_device_batch, resolve_pending_integration, wait_error_words) and in front of a write to device memory that a
// call in flight may read (drain_lanes, do_upload).  After it the next call stays in the current slot.
// The other slot's call may have kept its integration back for the next call into that slot, two calls on; that call
// now stays here, so the integration goes out at the join, alone, on lane 0 behind lane 1 -- the older call's, in front
// of the current slot's own (which whoever reads or enqueues resolves as ever: resolve_pending_integration).  The fence
// is recorded anew behind it: the launch reads the spectra lane 1 writes when it next takes that slot.
void launch_other_slot_integration(Radtran *r);
void join_lanes(Radtran *r) {
  if (r->on_other_lane) return;
  if (r->holds.other_in_flight) {
    HIPCHK(hipEventRecord(r->ev_fence, r->lane_stream[0]));
    HIPCHK(hipStreamWaitEvent(r->lane_stream[0], r->ev_lane1, 0));
    r->fence_due = true;
  }
  r->holds.joined();
  r->lane = 0;
  if (r->other.int_pending) {
    launch_other_slot_integration(r);
    HIPCHK(hipEventRecord(r->ev_fence, r->lane_stream[0]));
    r->fence_due = true;
  }
}
// ... and both lanes have run dry (the one host wait of a setter that rewrites device memory the kernels read)
void drain_lanes(Radtran *r) {
  join_lanes(r);
  if (r->stream) HIPCHK(hipStreamSynchronize(r->stream));
}
// Work goes to `lane` until the scope ends: `stream` names that lane's stream, and nothing inside joins.  Lane 1 is
// first ordered behind what lane 0 had done at the last join (it may have worked in the slot lane 1 is about to reuse);
// at the end an event behind lane 1's work is what the next join waits for.
struct LaneScope {
  Radtran *r;
  int lane;
  LaneScope(Radtran *r_, int lane_) : r(r_), lane(lane_) {
    r->on_other_lane = true;
    r->stream = r->lane_stream[lane];
    if (lane == 1 && r->fence_due) { r->fence_due = false; HIPCHK(hipStreamWaitEvent(r->stream, r->ev_fence, 0)); }
  }
  ~LaneScope() {
    if (lane == 1) { (void)hipEventRecord(r->ev_lane1, r->lane_stream[1]); r->holds.other_in_flight = true; }
    r->stream = r->lane_stream[0];
    r->on_other_lane = false;
  }
};
// The other slot's buffers and lane 1, the first time something goes there: the sizes of the current slot's, cleared as
// create_end clears those
void ensure_other_slot(Radtran *r) {
  CallSlot &o = r->other;
  if (o.allocated) return;
  if (!r->lane_stream[1]) HIPCHK(hipStreamCreateWithFlags(&r->lane_stream[1], hipStreamNonBlocking));
  for (hipEvent_t *e : {&r->ev_lane1, &r->ev_fence, &r->ev_colcopy})
    if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  auto like = [](DevBuf<double> &dst, const DevBuf<double> &src) { dst.alloc(src.n); dst.zero(); };
  like(o.d_col, r->d_col); like(o.d_prep, r->d_prep); like(o.d_opr, r->d_opr);
  auto view = [&](DevBuf<double> &dst, const DevBuf<double> &src) { dst.view(o.d_opr.p + (src.p - r->d_opr.p), src.n); };
  view(o.d_tau, r->d_tau); view(o.d_w0, r->d_w0); view(o.d_g, r->d_g); view(o.d_tau_band, r->d_tau_band); view(o.d_scat, r->d_scat);
  const DevBuf<double> *spec[8] = {&r->wrk_ir.fup_a, &r->wrk_ir.fdn_a, &r->wrk_ir.amean, &r->wrk_ir.tau_band,
                                   &r->wrk_sol.fup_a, &r->wrk_sol.fdn_a, &r->wrk_sol.amean, &r->wrk_sol.tau_band};
  for (int k = 0; k < 8; k++) like(o.spec[k], *spec[k]);
  o.d_small.alloc(r->rows.count); o.d_small.zero();   // (its error-word slot is never used: the words are the handle's, d_err)
  o.d_flux_n.view(o.d_small.p, r->rows.flux_count);
  o.d_done.alloc(r->d_done.n); o.d_done.zero();
  HIPCHK(hipStreamSynchronize(nullptr));   // the clears went to the null stream, which the lanes do not wait for
  o.allocated = true;
}
// The handle's buffers become the other slot's and the other way round
void swap_slot(Radtran *r) {
  CallSlot &o = r->other;
  r->d_col.swap(o.d_col); r->d_prep.swap(o.d_prep); r->d_opr.swap(o.d_opr);
  r->d_tau.swap(o.d_tau); r->d_w0.swap(o.d_w0); r->d_g.swap(o.d_g); r->d_tau_band.swap(o.d_tau_band); r->d_scat.swap(o.d_scat);
  DevBuf<double> *spec[8] = {&r->wrk_ir.fup_a, &r->wrk_ir.fdn_a, &r->wrk_ir.amean, &r->wrk_ir.tau_band,
                             &r->wrk_sol.fup_a, &r->wrk_sol.fdn_a, &r->wrk_sol.amean, &r->wrk_sol.tau_band};
  for (int k = 0; k < 8; k++) spec[k]->swap(o.spec[k]);
  r->d_small.swap(o.d_small); r->d_flux_n.swap(o.d_flux_n); r->d_done.swap(o.d_done);
  std::swap(r->col_upload, o.col_upload);
  std::swap(r->int_pending, o.int_pending); std::swap(r->pending_pipelined, o.pending_pipelined); std::swap(r->pending_ip, o.pending_ip);
}

// futils gauss_legendre (setup only, clima_eqns.f90:26-41)
void gauss_legendre(int n, std::vector<double> &x, std::vector<double> &w) {
  x.assign(n, 0.0);
  w.assign(n, 0.0);
  for (int i = 0; i < n; i++) {
    double z = std::cos(PI * (i + 0.75) / (n + 0.5)), pp = 0.0;
    for (int it = 0; it < 100; it++) {
      double p1 = 1.0, p2 = 0.0;
      for (int j = 0; j < n; j++) {
        double p3 = p2;
        p2 = p1;
        p1 = ((2.0 * j + 1.0) * z * p2 - j * p3) / (j + 1.0);
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0);
      double z1 = z;
      z = z1 - p1 / pp;
      if (std::fabs(z - z1) < 1e-16) break;
    }
    x[n - 1 - i] = z;
    w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
  }
}

int host_bracket(const std::vector<double> &xt, double x) {
  int n = (int)xt.size();
  if (x < xt[0]) return 0;
  if (x >= xt[n - 1]) return n - 2;
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    int mid = (lo + hi) / 2;
    if (x < xt[mid]) hi = mid; else lo = mid;
  }
  return lo;
}

// create_RTChannel, types_create.f90:226-270
bool make_channel(Radtran *r, ChannelObj &c, int which, int n, const double *wavl, char *err) {
  int ind1 = 0, ind2 = 0;
  double best1 = INFINITY, best2 = INFINITY;
  for (int i = 0; i < r->nw + 1; i++) {
    double d1 = std::fabs(wavl[0] - r->wavl[i]), d2 = std::fabs(wavl[n - 1] - r->wavl[i]);
    if (d1 < best1) { best1 = d1; ind1 = i; }
    if (d2 < best2) { best2 = d2; ind2 = i; }
  }
  const char *msg = "The wavelength bins are not compatible with the k-distribution wavelength bins.";
  if (n != ind2 - ind1 + 1) { set_err(err, msg); return false; }
  for (int i = 0; i < n; i++)
    if (!is_close(wavl[i], r->wavl[ind1 + i], 1.0e-7)) { set_err(err, msg); return false; }
  c.parent = r;
  c.which = which;
  c.nw = n - 1;
  c.wavl.assign(wavl, wavl + n);
  c.freq.resize(n);
  for (int i = 0; i < n; i++) c.freq[i] = C_LIGHT / (wavl[i] * 1.0e-9);
  c.ind_start = ind1;
  c.ind_end = ind2 - 1;
  return true;
}

void upload_fields(Radtran *r) {
  if (!r->fields_dirty) return;
  // kernels of earlier, unsynchronised calls may still be reading the old values (on either lane)
  drain_lanes(r);
  r->d_zen_u.upload(r->zenith_u);
  r->d_zen_w.upload(r->zenith_w);
  {
    std::vector<double> iu(r->zenith_u.size());
    for (size_t i = 0; i < iu.size(); i++) iu[i] = 1.0 / r->zenith_u[i];
    r->d_zen_iu.upload(iu);
  }
  r->d_albedo.upload(r->surface_albedo);
  r->d_emis.upload(r->surface_emissivity);
  r->d_photons.upload(r->photons_sol);
  r->fields_dirty = false;
}

// the g-point weights' edges (weight_e) and pair products, types_create.f90:1303-1304
void weight_edges_and_products(const std::vector<double> &wbin, std::vector<double> &wbin_e, std::vector<double> &wxy) {
  const int ng = (int)wbin.size();
  wbin_e.assign(ng + 1, 0.0);
  for (int i = 1; i < ng + 1; i++) wbin_e[i] = wbin[i - 1] + wbin_e[i - 1];
  wxy.assign((size_t)ng * ng, 0.0);
  for (int i = 0; i < ng; i++)
    for (int j = 0; j < ng; j++) wxy[j + (size_t)i * ng] = wbin[i] * wbin[j];
}

// Which rebin form the opacity kernels may use for these g-point weights (ng = 8).  The window form
// evaluates, for output edge k, only the sorted elements [RB_WIN_LO[k], RB_WIN_HI[k]]; the element j*
// that crosses E_k (C_{j*-1} < E_k <= C_{j*}) must be among them WHATEVER order the sort produces.
// C_j is bounded by the sums of the j+1 smallest / largest pair weights, so
//   j* >= first j with (sum of the j+1 largest)  >= E_k,   j* <= first j with (sum of the j+1 smallest) >= E_k.
// Both bounds are taken with a relative slack far above the rounding of a 64-term sum.  `stream`: never the window form.
int rebin_mode_for(const std::vector<double> &wbin, const std::vector<double> &wbin_e, const std::vector<double> &wxy, bool stream) {
  const int multi = (*std::max_element(wxy.begin(), wxy.end()) > *std::min_element(wbin.begin(), wbin.end())) ? 2 : 1;
  if (wbin.size() != 8 || stream) return multi;
  std::vector<double> s(wxy);
  std::sort(s.begin(), s.end());
  if (s[0] <= 0.0) return multi;
  double lo[64], hi[64], a = 0.0, b = 0.0;
  for (int j = 0; j < 64; j++) { a += s[j]; b += s[63 - j]; lo[j] = a; hi[j] = b; }
  for (int k = 1; k < 8; k++) {
    const double E = wbin_e[k];
    int jlo = 0, jhi = 0;
    while (jlo < 63 && hi[jlo] < E * (1.0 - 1e-9)) jlo++;
    while (jhi < 63 && lo[jhi] < E * (1.0 + 1e-9)) jhi++;
    if (jlo < RB_WIN_LO[k] || jhi > RB_WIN_HI[k]) return multi;
  }
  // the tight table (x and y ascending): lightest / heaviest down-set (Young diagram within the 8x8
  // grid of pairs (i, j), weight wbin(i)*wbin(j)) of every size, by enumeration of the 12 870 diagrams
  double dlo[65], dhi[65];
  for (int n = 0; n <= 64; n++) { dlo[n] = 1e300; dhi[n] = -1.0; }
  double rowcum[8][9];
  for (int i = 0; i < 8; i++) { rowcum[i][0] = 0.0; for (int j = 0; j < 8; j++) rowcum[i][j + 1] = rowcum[i][j] + wbin[i] * wbin[j]; }
  int len[8];
  std::function<void(int, int, int, double)> rec = [&](int i, int maxlen, int size, double wt) {
    if (i == 8) { dlo[size] = std::min(dlo[size], wt); dhi[size] = std::max(dhi[size], wt); return; }
    for (int rl = 0; rl <= maxlen; rl++) { len[i] = rl; rec(i + 1, rl, size + rl, wt + rowcum[i][rl]); }
  };
  rec(0, 8, 0, 0.0);
  for (int k = 1; k < 8; k++) {
    const double E = wbin_e[k];
    int jlo = 0, jhi = 0;
    while (jlo < 63 && dhi[jlo + 1] < E * (1.0 - 1e-9)) jlo++;
    while (jhi < 63 && dlo[jhi + 1] < E * (1.0 + 1e-9)) jhi++;
    if (jlo < RB_TIGHT_LO[k] || jhi > RB_TIGHT_HI[k]) return multi;
  }
  return 0;
}

// relative cost of a bin's opacity work, IR solve, solar solve (base + per zenith angle)
constexpr double SHARD_W_OP = 3.0, SHARD_W_IR = 1.0, SHARD_W_SOL0 = 0.6, SHARD_W_SOLZ = 0.24;

void compute_shard(Radtran *r) {
  // contiguous opacity-bin ranges balanced by work: opacity 3, IR solve 1, solar
  // solve 0.6 + 0.24 nzen -- the measured device-time ratios of the three kinds of work on MI355X
  // (tools/gpu_balance.py); rank 0-based.
  const int nw = r->nw, W = r->shard_world, R = r->shard_rank;
  std::vector<double> cost(nw + 1, 0.0);
  const int nzen = (int)r->zenith_u.size();
  for (int l = 0; l < nw; l++) {
    double c = SHARD_W_OP;
    if (l >= r->ir.ind_start && l <= r->ir.ind_end) c += SHARD_W_IR;
    if (l >= r->sol.ind_start && l <= r->sol.ind_end) c += SHARD_W_SOL0 + SHARD_W_SOLZ * nzen;
    cost[l + 1] = cost[l] + c;
  }
  auto cut = [&](int k) {
    if (k <= 0) return 0;
    if (k >= W) return nw;
    double target = cost[nw] * k / W;
    return (int)(std::lower_bound(cost.begin(), cost.end(), target) - cost.begin());
  };
  int lo = cut(R), hi = cut(R + 1);
  if (W == 1) { lo = 0; hi = nw; }
  r->op_lo = lo;
  r->op_n = hi - lo;
  auto clip = [&](const ChannelObj &c, int &clo, int &cn) {
    int a = std::max(lo, c.ind_start), b = std::min(hi - 1, c.ind_end);
    if (b < a) { clo = 0; cn = 0; } else { clo = a - c.ind_start; cn = b - a + 1; }
  };
  clip(r->ir, r->ir_lo, r->ir_n);
  clip(r->sol, r->sol_lo, r->sol_n);
}

hipEvent_t get_event(Radtran *r) {
  if (!r->pool.empty()) {
    hipEvent_t e = r->pool.back();
    r->pool.pop_back();
    return e;
  }
  hipEvent_t e;
  HIPCHK(hipEventCreate(&e));
  return e;
}

struct KernelTimer {
  Radtran *r;
  int id;
  hipEvent_t a = nullptr, b = nullptr;
  bool on() const {
    if (r->profile_stride > 1 && (r->timer_calls % r->profile_stride) != 0) return false;
    return r->profile == 1 || (r->profile == 2 && id == 1);
  }
  KernelTimer(Radtran *r_, int id_) : r(r_), id(id_) {
    if (on()) {
      a = get_event(r);
      b = get_event(r);
      HIPCHK(hipEventRecord(a, r->stream));
    }
  }
  void stop() {
    if (on()) {
      HIPCHK(hipEventRecord(b, r->stream));
      r->pending.push_back({a, b, id});
    }
  }
};

void resolve_events(Radtran *r) {
  for (auto &e : r->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      r->k_ms[e.id] += ms;
      r->k_n[e.id] += 1;
    }
    r->pool.push_back(e.a);
    r->pool.push_back(e.b);
  }
  r->pending.clear();
}

// Prep block of one column (d_prep or a slice of the batch arena)
void prep_views(Radtran *r, double *base, ColumnDev &c) {
  const size_t nz = r->nz, nab = std::max<size_t>(1, r->abs_entries.size()), ns = (size_t)r->nslots + 1;
  c.log10P = base;
  c.cols = c.log10P + nz;
  c.foreign_col = c.cols + nz * r->nsp;
  c.absw = c.foreign_col + nz;
  c.q = c.absw + nab * nz;
  c.ix = reinterpret_cast<int *>(c.q + ns * nz);
}
size_t prep_block_count(Radtran *r) {
  const size_t nz = r->nz, nab = std::max<size_t>(1, r->abs_entries.size()), ns = (size_t)r->nslots + 1;
  return nz * (2 + r->nsp + nab + ns) + (ns * nz + 1) / 2;
}

// Optical-property block [tau | w0 | g | tau_band | scat] laid over `base` (d_opr, or a column's slice of the batch
// arena); count: doubles in the block.  A null base gives the count alone.
struct OprViews { double *tau, *w0, *g, *tau_band, *scat; size_t count; };
OprViews opr_views(const Radtran *r, double *base) {
  const size_t nwz = (size_t)r->nw * r->nz, nwgz = nwz * r->ng;
  OprViews v{};
  auto take = [&](size_t n) { double *p = base ? base + v.count : nullptr; v.count += n; return p; };
  v.tau = take(nwgz); v.w0 = take(nwgz); v.g = take(nwz); v.tau_band = take(nwz); v.scat = take(nwz);
  return v;
}

// Spectra block of one column of a batch, laid over `base` the same way:
// [ir fup_a | ir fdn_a | ir tau_band | sol fup_a | sol fdn_a | sol amean | sol tau_band]
struct SpectraViews { double *ir_fup_a, *ir_fdn_a, *ir_tau_band, *sol_fup_a, *sol_fdn_a, *sol_amean, *sol_tau_band; size_t count; };
SpectraViews spectra_views(const Radtran *r, double *base) {
  const size_t nl = (size_t)r->nz + 1, nz = r->nz, ni = r->ir.nw, ns = r->sol.nw;
  SpectraViews v{};
  auto take = [&](size_t n) { double *p = base ? base + v.count : nullptr; v.count += n; return p; };
  v.ir_fup_a = take(ni * nl); v.ir_fdn_a = take(ni * nl); v.ir_tau_band = take(ni * nz);
  v.sol_fup_a = take(ns * nl); v.sol_fdn_a = take(ns * nl); v.sol_amean = take(ns * nl); v.sol_tau_band = take(ns * nz);
  return v;
}

// Where one radiate call's data lives.  RESIDENT: the handle's own buffers.  ARENA_COLUMN: one column of a batch
// (radtran_toa_fluxes_batch), its column block and level rows in the arenas, everything else the handle's.
// ARENA_CHUNK: `ncol` columns worked on by ONE launch of each kernel, per-column blocks in the arenas, column c of
// the chunk at base + c * stride.
enum CallKind { CALL_RESIDENT, CALL_ARENA_COLUMN, CALL_ARENA_CHUNK };
struct CallBufs {
  CallKind kind;
  double *col, *prep;      // column block, prep block
  const double *bounds;    // a bounds batch: the bounds block of the (first) column; null: the handle's fields
  int nsrc;                // source layers of the column (a chunk: nz, the bound of its columns')
  bool all_pairs_exact;    // every layer is half of an exact pair (known of the resident column only)
  OprViews opr;
  SpectraViews spec;
  double *flux_n;          // the level rows (LevelRows)
  int *done;               // the fused grid's per-tile flags
  int ncol;                // columns of this launch; their blocks are bs apart (zero but for a chunk)
  BatchStrides bs;
  bool host_out;           // a synchronous wrapper's call: the integration may store into the host's pinned block
};

CallBufs resident_bufs(Radtran *r, bool host_out = false) {
  CallBufs b{};
  b.kind = CALL_RESIDENT; b.ncol = 1; b.host_out = host_out;
  b.col = r->d_col.p; b.prep = r->d_prep.p;
  b.nsrc = r->nsrc; b.all_pairs_exact = r->all_pairs_exact;
  b.opr = OprViews{r->d_tau.p, r->d_w0.p, r->d_g.p, r->d_tau_band.p, r->d_scat.p, r->opr_count};
  b.spec = SpectraViews{r->wrk_ir.fup_a.p, r->wrk_ir.fdn_a.p, r->wrk_ir.tau_band.p, r->wrk_sol.fup_a.p,
                        r->wrk_sol.fdn_a.p, r->wrk_sol.amean.p, r->wrk_sol.tau_band.p, 0};   // (seven buffers, no block)
  b.flux_n = r->d_flux_n.p; b.done = r->d_done.p;
  return b;
}
// the bounds blocks' layout on this handle
BoundsLayout handle_bounds_layout(const Radtran *r) { return bounds_layout(r->sol.nw, r->ir.nw, (int)r->zenith_u.size()); }
// column c of the arena (nsrc: what build_meta returned for it) on the handle's optical-property and spectra buffers;
// bounds: the batch's bounds blocks, bounds_count doubles each (null: none)
CallBufs arena_column_bufs(Radtran *r, int c, int nsrc, const double *bounds = nullptr, size_t bounds_count = 0) {
  CallBufs b = resident_bufs(r);
  b.bounds = bounds ? bounds + (size_t)c * bounds_count : nullptr;
  b.kind = CALL_ARENA_COLUMN; b.nsrc = nsrc; b.all_pairs_exact = false;
  b.col = r->d_cols_arena.p + (size_t)c * r->col_layout.count;
  b.flux_n = r->d_flux_arena.p + c * r->rows.stride;
  return b;
}
// columns [c0, c0 + ncol) of the arena, their prep / opr / spectra blocks from the start of those arenas
CallBufs arena_chunk_bufs(Radtran *r, int c0, int ncol, const double *bounds = nullptr, size_t bounds_count = 0) {
  CallBufs b = resident_bufs(r);
  b.bounds = bounds ? bounds + (size_t)c0 * bounds_count : nullptr;
  b.kind = CALL_ARENA_CHUNK; b.ncol = ncol; b.nsrc = r->nz; b.all_pairs_exact = false;
  b.col = r->d_cols_arena.p + (size_t)c0 * r->col_layout.count; b.prep = r->d_prep_arena.p;
  b.opr = opr_views(r, r->d_opr_arena.p); b.spec = spectra_views(r, r->d_res_arena.p);
  b.flux_n = r->d_flux_arena.p + c0 * r->rows.stride;
  b.bs = BatchStrides{r->col_layout.count, r->prep_count, b.opr.count, b.spec.count, r->rows.stride,
                      (int)(((size_t)r->op_n * r->nz + 255) / 256), (int)bounds_count};
  return b;
}

ColumnDev column_dev(Radtran *r, const CallBufs &b) {
  ColumnDev c;
  const ColumnLayout &l = r->col_layout;
  c.T_surface = b.col;
  c.T = b.col + l.T; c.P = b.col + l.P; c.dz = b.col + l.dz;
  c.dens = b.col + l.dens; c.pdens = b.col + l.pdens; c.radii = b.col + l.radii;
  c.meta = reinterpret_cast<const int *>(b.col + l.meta);
  prep_views(r, b.prep, c);
  c.err_flag = r->d_err.p;
  return c;
}

// The pair_reuse table of one column (pair_decision, radtran_dev.h, for every pair of an even number of layers), so
// that the grid size and every kernel work from ONE decision.
// meta: [0] = nsrc, [1 + m] = m-th source layer (0-based, ascending) | SRC_PAIR | SRC_EXACT,
// [1 + nz + j] = source layer of layer j.  Returns nsrc.
int build_meta(Radtran *r, const ColumnArrays &a, int *meta) {
  const int nz = r->nz;
  const bool use_radii = a.has_particles() && !r->part.empty();  // present(radii) .and. self%npart > 0
  int nsrc = 0;
  int *srcl = meta + 1, *src = meta + 1 + nz;
  for (int j = 0; j < nz; j++) {
    PairDecision d{false, false};
    if ((nz & 1) == 0 && (j & 1) == 1) d = pair_decision(j, nz, r->nsp, r->np, a.T, a.P, a.dz, a.dens, a.pdens, a.radii, use_radii);
    if (d.reuse) {
      srcl[nsrc - 1] |= SRC_PAIR | (d.exact ? SRC_EXACT : 0);  // layer j-1 is the entry just written
      src[j] = j - 1;
    } else {
      srcl[nsrc++] = j;
      src[j] = j;
    }
  }
  for (int m = nsrc; m < nz; m++) srcl[m] = nz - 1;
  meta[0] = nsrc;
  return nsrc;
}

// Packs one column into a host block (column_layout), pair_reuse table included.  Returns nsrc.
int pack_column(Radtran *r, double *h, const ColumnArrays &in) {
  const size_t nz = r->nz;
  const ColumnLayout &l = r->col_layout;
  const ColumnArrays a = in.column(0, r->nz, r->nsp, r->np);   // (the particle columns together or not at all)
  h[0] = *a.T_surface;
  std::memcpy(h + l.T, a.T, sizeof(double) * nz);
  std::memcpy(h + l.P, a.P, sizeof(double) * nz);
  std::memcpy(h + l.dz, a.dz, sizeof(double) * nz);
  std::memcpy(h + l.dens, a.dens, sizeof(double) * nz * r->nsp);
  if (a.has_particles()) {
    std::memcpy(h + l.pdens, a.pdens, sizeof(double) * nz * r->np);
    std::memcpy(h + l.radii, a.radii, sizeof(double) * nz * r->np);
  }
  return build_meta(r, a, reinterpret_cast<int *>(h + l.meta));
}

// The bounds blocks of n columns (bounds_layout) on the host: bounds_element of the caller's arrays and the handle's
// fields, as k_pack_bounds takes them on the device
void pack_bounds(const Radtran *r, int n, const BoundsArrays &in, double *blocks) {
  const BoundsLayout l = handle_bounds_layout(r);
  const BoundsArrays own{r->surface_albedo.data(), r->surface_emissivity.data(), r->zenith_u.data(), r->zenith_w.data(), nullptr};
  for (size_t c = 0; c < (size_t)n; c++)
    for (size_t i = 0; i < l.count; i++) blocks[c * l.count + i] = bounds_element(l, i, c, in, own, r->photon_scale_factor);
}

// f_total into the fifth row of a level-row block: THE place where a call's f_total is formed (a device batch's:
// k_batch_finish)
void f_total_row(double *h, const LevelRows &l) {
  for (size_t i = 0; i < l.nl; i++)
    h[l.f_total + i] = f_total_level(h[l.ir_up + i], h[l.ir_dn + i], h[l.sol_up + i], h[l.sol_dn + i]);
}
// ... and ISR, OLR from its last level
void toa_fluxes(const double *h, const LevelRows &l, double *ISR, double *OLR) {
  const size_t top = l.nl - 1;
  toa_isr_olr(h[l.ir_up + top], h[l.ir_dn + top], h[l.sol_up + top], h[l.sol_dn + top], *ISR, *OLR);
}

// The parameter blocks of a call's launches: each from the handle and the call's buffers
TwoStreamParams make_twostream_params(Radtran *r, const CallBufs &b, const ColumnDev &col, bool compute_solar) {
  TwoStreamParams ts;
  const int nz = r->nz;
  std::memset(&ts, 0, sizeof(ts));
  ts.nz = nz; ts.ng = r->ng;
  ts.n_sol = compute_solar ? r->sol_n : 0; ts.sol_lo = r->sol_lo;
  ts.n_ir = r->ir_n; ts.ir_lo = r->ir_lo;
  ts.sol_start = r->sol.ind_start; ts.ir_start = r->ir.ind_start;
  ts.tau = b.opr.tau; ts.w0 = b.opr.w0; ts.g = b.opr.g; ts.tau_band = b.opr.tau_band; ts.scat = b.opr.scat;
  ts.wbin = r->d_wbin.p; ts.freq = r->d_freq.p;
  ts.T = col.T; ts.T_surface = col.T_surface;
  ts.emissivity = r->d_emis.p; ts.has_hard_surface = r->has_hard_surface ? 1 : 0; ts.ir_tau_min = r->ir_tau_min;
  ts.nzen = (int)r->zenith_u.size(); ts.zen_u = r->d_zen_u.p; ts.zen_w = r->d_zen_w.p; ts.zen_iu = r->d_zen_iu.p;
  for (int z = 0; z < ts.nzen && z < MAX_ZEN; z++) {
    ts.zen_u_v[z] = r->zenith_u[z]; ts.zen_w_v[z] = r->zenith_w[z]; ts.zen_iu_v[z] = 1.0 / r->zenith_u[z];
  }
  ts.albedo = r->d_albedo.p; ts.photons_sol = r->d_photons.p;
  ts.photon_scale_factor = r->photon_scale_factor; ts.diurnal_fac = r->diurnal_fac;
  ts.am_f1 = r->d_am_f1.p; ts.am_f2 = r->d_am_f2.p; ts.am_dw = r->d_am_dw.p;
  if (b.bounds) { ts.bounds = 1; ts.albedo = b.bounds; ts.bnd_nw_sol = r->sol.nw; ts.bnd_nw_ir = r->ir.nw; }   // (TwoStreamParams::bounds)
  ts.ir_fup_a = b.spec.ir_fup_a; ts.ir_fdn_a = b.spec.ir_fdn_a; ts.ir_tau_band = b.spec.ir_tau_band;
  ts.sol_fup_a = b.spec.sol_fup_a; ts.sol_fdn_a = b.spec.sol_fdn_a; ts.sol_amean = b.spec.sol_amean;
  ts.sol_tau_band = b.spec.sol_tau_band;
  return ts;
}

// clears: the two-stream outputs that spare blocks of the prep launch zero (null: none)
PrepParams make_prep_params(Radtran *r, const CallBufs &b, const ColumnDev &col, int call_id, const TwoStreamParams *clears) {
  PrepParams pp;
  std::memset(&pp, 0, sizeof(pp));
  pp.ncol = b.ncol; pp.bs = b.bs;
  pp.nz = r->nz; pp.nsp = r->nsp; pp.np = r->np; pp.nslots = r->nslots;
  pp.has_cont = r->has_cont; pp.LH2O = r->LH2O;
  for (int s = 0; s < r->nslots; s++) pp.slots[s] = r->slots[s];
  if (r->cust_on) {  // evaluated without clamping: the end intervals extrapolate (linear_interpolation_module.F90:348-350)
    SlotDev cs;
    cs.axis = r->d_cust_axis.p; cs.n = r->cust_nP; cs.source = -1;
    cs.lo = -std::numeric_limits<double>::infinity(); cs.hi = std::numeric_limits<double>::infinity();
    cs.flag_clamp = 0;
    pp.slots[pp.nslots++] = cs;
  }
  pp.nabs = (int)r->abs_entries.size();
  for (int e = 0; e < pp.nabs; e++) { pp.abs_kind[e] = r->abs_entries[e].kind; pp.abs_a[e] = r->abs_entries[e].a; pp.abs_b[e] = r->abs_entries[e].b; }
  pp.col = col;
  pp.call_id = call_id;
  if (clears) pp.nzero = ts_clear_ranges(*clears, pp.zero_ptr, pp.zero_count);
  return pp;
}

OpacityParams make_opacity_params(Radtran *r, const CallBufs &b, const ColumnDev &col, bool write_w0) {
  OpacityParams op;
  std::memset(&op, 0, sizeof(op));
  op.nz = r->nz; op.nw = r->nw; op.ng = r->ng; op.nsp = r->nsp; op.np = r->np;
  op.bin_lo = r->op_lo; op.nbins = r->op_n; op.nsrc = b.nsrc;
  op.nk = (int)r->k.size(); op.nray = (int)r->ray.size(); op.npart = (int)r->part.size();
  for (size_t i = 0; i < r->k.size(); i++)
    op.k[i] = KDev{r->k[i]->d_log10k.p, r->k[i]->sp, r->k[i]->nP, r->k[i]->nT, (int)(2 * i), (int)(2 * i + 1)};
  for (size_t i = 0; i < r->ray.size(); i++) op.ray[i] = XsDev{r->ray[i]->d_data.p, 0, r->ray[i]->sp1, -1, 0, -1};
  op.nabs = (int)r->abs_entries.size();
  for (int e = 0; e < op.nabs; e++) op.abs[e] = r->abs_entries[e];
  for (size_t i = 0; i < r->part.size(); i++)
    op.part[i] = PartDev{r->part[i]->d_w0.p, r->part[i]->d_qext.p, r->part[i]->d_gt.p, r->part[i]->p_ind, r->part[i]->nrad, r->part_slot[i]};
  op.wbin = r->d_wbin.p; op.wbin_e = r->d_wbin_e.p; op.wxy = r->d_wxy.p; op.wbin_e_pad = r->d_wbin_e_pad.p; op.rorr_tab = r->d_rorr_tab.p;
  op.col = col;
  op.cust = CustomDev{r->d_cust_dtau.p, r->d_cust_w0.p, r->d_cust_g0.p, r->cust_nP, r->nslots, r->cust_on ? 1 : 0};
  op.rebin_mode = r->rebin_mode;
#ifdef CLIMA_STAMPS
  op.stamps = r->d_stamps.p;
#endif
  op.tau = b.opr.tau; op.w0 = b.opr.w0; op.g = b.opr.g; op.tau_band = b.opr.tau_band; op.scat = b.opr.scat;
  op.write_w0 = write_w0 ? 1 : 0;
  return op;
}

// reduce: the call ends with the handle's all-reduce.  host_out set in the result: the integration stores the level
// rows and the error words into the host's pinned block as well (a synchronous call on an unsharded handle, which
// then ends with a stream synchronise -- no copy launch in front of it)
IntegrateParams make_integrate_params(Radtran *r, const CallBufs &b, bool compute_solar, bool reduce) {
  IntegrateParams ip;
  std::memset(&ip, 0, sizeof(ip));
  ip.ncol = b.ncol; ip.bs = b.bs;
  ip.nz = r->nz; ip.nw_ir = r->ir.nw; ip.nw_sol = r->sol.nw;
  ip.ir_lo = r->ir_lo; ip.ir_n = r->ir_n; ip.sol_lo = r->sol_lo; ip.sol_n = r->sol_n;
  ip.do_solar = compute_solar ? 1 : 0;
  ip.ir_fup_a = b.spec.ir_fup_a; ip.ir_fdn_a = b.spec.ir_fdn_a;
  ip.sol_fup_a = b.spec.sol_fup_a; ip.sol_fdn_a = b.spec.sol_fdn_a;
  ip.ir_freq = r->ir.d_freq.p; ip.sol_freq = r->sol.d_freq.p;
  ip.flux_n = b.flux_n;
  ip.flux_part = r->shard_world > 1 ? r->d_flux_part.p : nullptr;
  ip.nchunk = integrate_chunks(std::max(r->ir_n, r->sol_n));
  ip.partial = r->d_partial.p;
  if (b.host_out && r->h_small_dev && b.kind == CALL_RESIDENT && !reduce && r->shard_world == 1 && integrate_fits_one_launch(ip.nchunk)) {
    ip.host_out = r->h_small_dev;
    ip.err_words = r->d_err.p;
  }
  if (reduce) {
    // the status word rides on the all-reduce in the slot behind the four level rows (LevelRows::status; f_total is
    // formed on the host from the REDUCED rows, fetch_small)
    ip.timeout_out = r->d_small.p + r->rows.status; ip.timeout_flag = r->d_err.p + 1;
    ip.id_opr = r->call_id; ip.id_sol = r->solar_id;
  }
  return ip;
}

// The one switch fixed for the process at its first use (the handle-less test hooks obey it too); the others are read
// once into the handle when it is made (read_handle_switches) -- a look into the environment per call is a walk through the whole of it.
bool sw_no_half() { static const bool v = [] { const char *e = getenv("CLIMA_HIP_NO_HALF"); return e && e[0] == '1'; }(); return v; }

// what plan_radiate needs to know of a call on this handle; a chunk: one launch per kernel for its columns
PlanIn plan_input(const Radtran *r, const CallBufs &b, bool compute_solar, bool compute_opacity, bool allow_fused) {
  PlanIn in{};
  in.nz = r->nz; in.ng = r->ng; in.nzen = (int)r->zenith_u.size();
  in.n_ir = r->ir_n; in.n_sol = compute_solar ? r->sol_n : 0; in.op_n = r->op_n;
  in.batch = b.kind == CALL_ARENA_CHUNK; in.ncol = b.ncol;
  in.nsrc = b.nsrc;
  in.rebin_mode = r->rebin_mode; in.cust_on = r->cust_on; in.compute_opacity = compute_opacity;
  // exact pairs in the column (and this call computes the opacities from it) -> exact pairs in opr
  in.all_pairs = compute_opacity && b.all_pairs_exact;
  in.fused = r->fused; in.allow_fused = allow_fused;
  in.ts_block_mode = r->ts_block_mode; in.coop_items = r->coop_items;
  in.no_half = sw_no_half();
  return in;
}

// The stored w0 array is current (a fused call's tiles leave it to the two-stream part of the same grid:
// whoever else wants it -- IR-only calls on the stored opacities, the batched IR kernel, radtran_opr_get --
// gets it formed from tau and the layers' scattering optical depth first)
void ensure_w0(Radtran *r) {
  if (r->holds.w0_stored) return;
  launch_w0_from_scat(r->d_tau.p, r->d_scat.p, r->d_w0.p, r->nw, r->ng, r->nz, r->stream);
  HIPCHK(hipGetLastError());
  r->holds.w0_formed();
}

// What an entry point needs of the handle (NEED_*), stated in one line at its top: true, and refused()'s text with the
// caller's name in `err`, when the handle does not hold it.  comm_counts false: not even a communicator makes a shard do.
bool refuse(const Radtran *r, const char *who, int needs, char *err, bool comm_counts = true) {
  const char *t = refused(r->holds, needs, r->shard_world, comm_counts && r->comm, r->op_lo, r->op_n);
  if (t) set_err(err, t[0] == ' ' ? std::string(who) + t : std::string(t));
  return t != nullptr;
}

// May a resident call on this handle keep its integration back?  Not on a bin-sharded handle or one with a communicator
// (the all-reduce follows the integration), not with per-kernel events (they need the four kernels apart), not while the
// stream is being captured (a graph holds whole calls), not once the flux device pointer is out, not with the switch off.
bool defer_allowed(bool switch_on, int shard_world, bool has_comm, int profile, bool capturing, bool flux_ptr_taken) {
  return switch_on && shard_world == 1 && !has_comm && profile != 1 && !capturing && !flux_ptr_taken;
}
bool stream_capturing(Radtran *r) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  HIPCHK(hipStreamIsCapturing(r->stream, &st));
  return st != hipStreamCaptureStatusNone;
}
bool defer_eligible(Radtran *r) {   // (the runtime is asked only where the answer decides)
  return defer_allowed(r->defer_integration, r->shard_world, r->comm != nullptr, r->profile, false, r->flux_ptr_taken) && !stream_capturing(r);
}
// Waves of a compute_opacity call's main grid: the fused grid's opacity tiles and two-stream items, or the opacity launch
// of the separate form; blocks of 256 threads (OP_THREADS, kernels.hip), four waves each.
long radiate_grid_waves(const PlanIn &in, const LaunchPlan &pl) {
  const long items = (long)in.op_n * in.nsrc, tiles = (items + 255) / 256;
  if (pl.fused.form != TS_NONE) return 4 * (tiles + (long)(in.n_sol + in.n_ir) * pl.fused.groups);
  if (pl.opacity == OP_COOP) return 4 * ((items * pl.coop_ng + 255) / 256);
  return 4 * tiles;
}
// Does a resident call that computes opacities and solar fluxes run BESIDE the previous call, in the call slot that is
// not current and on that slot's lane?  THE rule, every condition of it, as plain values: the call may keep its results
// back (defer_ok: defer_allowed, the capture state included); nobody has waited for or joined the previous pipelined call
// since it was enqueued; its dominant kernel carries no event pair (sampled: a timed launch runs alone); the fields on the
// device are current (stale ones are uploaded behind a join and a host wait); no integration is pending that a call
// which was not pipelined kept back (a pipelined call's own stays in its slot for the next call into that slot and
// keeps nobody from going beside: radtran_radiate_resident feeds in only the former); the integration fits the
// one-launch kernel (the other form's partial sums are shared); and the mode says so: 1 never, 2 always, 0 (automatic)
// when the grid does not fit the device in one residency round of two waves per SIMD -- a smaller call is launch-bound,
// and the tests pin its launch sequence.  Everything else joins first and stays in the current slot.
struct TwoInFlight {
  int mode;
  bool defer_ok, prev_unjoined, sampled, fields_dirty, int_pending, integrates_in_one_launch;
  long grid_waves;
  int cus;
};
bool two_in_flight_allowed(const TwoInFlight &q) {
  if (q.mode == 1 || !q.defer_ok || !q.prev_unjoined || q.sampled || q.fields_dirty || q.int_pending || !q.integrates_in_one_launch) return false;
  return q.mode == 2 || q.grid_waves > 2L * 4 * q.cus;
}
bool call_is_sampled(const Radtran *r) {   // KernelTimer::on() of the next call's dominant kernel
  return r->profile == 2 && (r->profile_stride <= 1 || (r->timer_calls + 1) % r->profile_stride == 0);
}
// The rule asked of this handle's next full resident call, the previous call taken as `prev_unjoined` and a pending
// integration as `int_pending`.  The plan is made only where the mode needs the grid's size, and the runtime is asked for
// the capture state only where the answer decides.
bool two_in_flight(Radtran *r, bool prev_unjoined, bool int_pending) {
  TwoInFlight q{};
  q.mode = r->calls_in_flight; q.prev_unjoined = prev_unjoined; q.int_pending = int_pending;
  q.sampled = call_is_sampled(r); q.fields_dirty = r->fields_dirty; q.cus = r->cus;
  q.defer_ok = defer_allowed(r->defer_integration, r->shard_world, r->comm != nullptr, r->profile, false, r->flux_ptr_taken);
  q.integrates_in_one_launch = integrate_fits_one_launch(integrate_chunks(std::max(r->ir_n, r->sol_n)));
  if (q.mode == 0 && q.defer_ok && prev_unjoined) {
    const PlanIn in = plan_input(r, resident_bufs(r, false), true, true, true);
    q.grid_waves = radiate_grid_waves(in, plan_radiate(in));
  }
  if (!two_in_flight_allowed(q)) return false;
  q.defer_ok = !stream_capturing(r);
  return two_in_flight_allowed(q);
}
// ... were the previous call unjoined: the handle pipelines two, so its full resident calls alternate between the slots
// and each keeps its integration back in its own
bool pipelining_two(Radtran *r) { return two_in_flight(r, true, false); }

// THE place where the current slot's pending integration is resolved.  With the prep parameters of a compute_opacity
// call that is about to launch its prep pass (and clears nothing there): both in one grid where k_prep_integrate covers
// them -- returns true, the prep pass is launched.  Otherwise (prep null: everything else that enqueues work or reads
// results, through settle_device_batch) the integration alone, with the parameters stored when its call was enqueued --
// returns false.  A call beside the previous one (LaneScope) finds here what the call two before it left in the slot it
// takes, and launches it on that slot's lane; everyone else joins first, which sends the other slot's out ahead.
bool resolve_pending_integration(Radtran *r, const PrepParams *prep = nullptr) {
  join_lanes(r);   // (whoever comes here enqueues work or reads results: the other lane's call first)
  if (!r->int_pending) return false;
  r->int_pending = false;
  if (prep && r->profile != 1 && prep_integrate_merges(*prep, r->pending_ip) && !stream_capturing(r)) {
    launch_prep_integrate(*prep, r->pending_ip, r->stream);
    HIPCHK(hipGetLastError());
    r->merged_integrations++;
    return true;
  }
  { KernelTimer t(r, 3); launch_integrate(r->pending_ip, r->stream); HIPCHK(hipGetLastError()); t.stop(); }
  r->standalone_integrations++;
  return false;
}
// ... and the other slot's, at a join (join_lanes): alone, on lane 0
void launch_other_slot_integration(Radtran *r) {
  r->other.int_pending = false;
  { KernelTimer t(r, 3); launch_integrate(r->other.pending_ip, r->lane_stream[0]); HIPCHK(hipGetLastError()); t.stop(); }
  r->standalone_integrations++;
}

// The current slot's column block is the handle's latest column: an upload went to the slot its next call was expected
// to take, and a slot that was passed over gets the column by one device copy out of the other's block, behind the upload
// (ev_upload).  Whatever next writes the block such a copy read -- an upload, or a copy the other way -- waits for the
// copy's event first (wait_for_column_copy); the debt stays until that has happened.
void wait_for_column_copy(Radtran *r, const double *block_to_write) {
  if (!r->colcopy_pending || r->colcopy_src != block_to_write) return;
  HIPCHK(hipStreamWaitEvent(r->stream, r->ev_colcopy, 0));
  r->colcopy_pending = false;
}
void ensure_column(Radtran *r) {
  if (r->col_upload == r->holds.uploads || !r->other.allocated || r->other.col_upload != r->holds.uploads) return;
  if (r->upload_pending) HIPCHK(hipStreamWaitEvent(r->stream, r->ev_upload, 0));
  wait_for_column_copy(r, r->d_col.p);
  // (an earlier copy that read the same block and is still owed a wait: this lane waits for it too, so that the one
  //  event, recorded anew below, stands for both)
  if (r->colcopy_pending) HIPCHK(hipStreamWaitEvent(r->stream, r->ev_colcopy, 0));
  launch_copy(r->d_col.p, r->other.d_col.p, r->col_layout.count, r->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(r->ev_colcopy, r->stream));
  r->colcopy_pending = true;
  r->colcopy_src = r->other.d_col.p;
  r->col_upload = r->holds.uploads;
}

// plan -> prep -> opacity (or the fused grid) -> two-stream -> integrate -> reduce, on the buffers `b` names
// defer: the caller returns without anyone reading a result, so the integration may wait for the next call's prep launch
// (DEFER_FOR_A_MERGE, a pipelined call of a handle that keeps two in flight: only where this call's own prep pass
// cleared nothing -- the next call into the slot has this call's shape, and behind a prep pass that clears the kept-back
// integration would only be the same launch later on the same lane, which measured 1.6 us per call slower at config 5)
enum Defer { DEFER_NEVER = 0, DEFER_ALWAYS, DEFER_FOR_A_MERGE };
void enqueue_radiate(Radtran *r, const CallBufs &b, bool compute_solar, bool compute_opacity, bool allow_fused = true, Defer defer = DEFER_NEVER) {
  char why[CLIMA_ERR_LEN + 1];   // (a one-launch batch left its optical properties in the arena, another shard's pass covers other bins)
  if (!compute_opacity && refuse(r, "radiate", NEED_OPACITIES, why)) throw HipFail{why};
  r->timer_calls++;
  upload_fields(r);
  const bool resident = b.kind == CALL_RESIDENT, chunk = b.kind == CALL_ARENA_CHUNK;
  if (resident) { join_lanes(r); ensure_column(r); }   // (a call beside the previous one: nothing joins, see LaneScope)
  const ColumnDev col = column_dev(r, b);
  TwoStreamParams ts = make_twostream_params(r, b, col, compute_solar);
  const LaunchPlan plan = plan_radiate(plan_input(r, b, compute_solar, compute_opacity, allow_fused));
  bool fused_done = false;
  if (compute_opacity) {
    const int call_id = ++r->call_id;
    const PrepParams pp = make_prep_params(r, b, col, call_id, plan.prep_clears ? &ts : nullptr);
    // (a prep pass that clears would zero the very spectra a pending integration reads: that one goes first, alone)
    if (!resolve_pending_integration(r, resident && !plan.prep_clears ? &pp : nullptr)) {
      KernelTimer t(r, 0); launch_prep(pp, r->stream); HIPCHK(hipGetLastError()); t.stop();
    }

    OpacityParams op = make_opacity_params(r, b, col, plan.write_w0);
    if (plan.fused.form != TS_NONE) {
      FusedParams fp;
      std::memset(&fp, 0, sizeof(fp));
      fp.ncol = b.ncol; fp.bs = b.bs;
      fp.call_id = call_id; fp.max_spins = r->fused_max_spins;
      fp.done = b.done; fp.timeout_flag = r->d_err.p + 1;
      KernelTimer t(r, 1);
      fused_done = launch_fused(op, ts, fp, plan.fused, r->stream);
      HIPCHK(hipGetLastError());
      t.stop();
      // (the runtime refused the grid its LDS: the separate launches, w0 stored; ensure_w0() materialises an
      //  unwritten w0 when something else asks for it)
      if (!fused_done) op = make_opacity_params(r, b, col, true);
    }
    if (chunk && !fused_done) throw HipFail{"internal: a one-launch batch needs the fused grid"};
    if (!fused_done) {
      KernelTimer t(r, 1);
      const bool ok = launch_opacity(op, plan, r->stream);
      HIPCHK(hipGetLastError());
      if (!ok)
        throw HipFail{"k-distributions with " + std::to_string(r->ng) + " g-points are not supported (1..32)"};
      t.stop();
    }
    r->holds.opacities_written(!chunk, op.write_w0 != 0, resident, r->op_lo, r->op_n);
  } else {
    resolve_pending_integration(r);   // (an IR-only call's solar rows are the last solar call's)
    if (!chunk) ensure_w0(r);   // this call's two-stream kernels read the stored optical properties
  }
  r->last_cs = compute_solar;
  if (compute_solar) r->solar_id = r->call_id;

  if (!fused_done) {
    KernelTimer t(r, 2);
    // default: wave-per-column kernel; CLIMA_HIP_TS_MODE=block selects the workgroup-per-bin form
    bool ok = launch_twostream_w(ts, plan.ts, r->stream);
    if (!ok) { HIPCHK(hipGetLastError()); ok = launch_twostream(ts, plan.block, r->stream); }
    HIPCHK(hipGetLastError());
    if (!ok)
      throw HipFail{"nz*ngauss = " + std::to_string(r->nz * r->ng) + " exceeds what the two-stream kernels can stage"};
    t.stop();
  }

  const bool reduce = r->comm && resident;
  const IntegrateParams ip = make_integrate_params(r, b, compute_solar, reduce);
  r->holds.rows_enqueued(ip.host_out != nullptr);
  const bool may_defer = defer == DEFER_ALWAYS || (defer == DEFER_FOR_A_MERGE && !plan.prep_clears);
  if (may_defer && resident && !reduce && !ip.host_out && integrate_fits_one_launch(ip.nchunk) && defer_eligible(r)) {
    r->pending_ip = ip;
    r->int_pending = true;
    r->pending_pipelined = false;   // (radtran_radiate_resident marks a pipelined call's)
  } else {
    KernelTimer t(r, 3); launch_integrate(ip, r->stream); HIPCHK(hipGetLastError()); t.stop();
  }
  if (reduce) {
    // the step's single collective (src/radtran/clima_radtran_radiate.f90:184-192 summed over the bins of all
    // ranks): in place, on the handle's stream, no host round trip
    NCCLCHK(ncclAllReduce(r->d_small.p, r->d_small.p, r->rows.reduce_count, ncclDouble, ncclSum, r->comm, r->stream));
    r->comm_reduces++;
  }
}

bool recover_fused_timeout(Radtran *r);
void settle_device_batch(Radtran *r);
void settle_pending_batch(Radtran *r);

void fetch_small(Radtran *r) {
  settle_device_batch(r);
  if (r->holds.rows_on_host) return;
  const LevelRows &l = r->rows;
  for (int pass = 0; pass < 2; pass++) {
    if (!r->holds.rows_in_pinned) {
      // one copy: the error words end the handle's first level-row block.  The second slot's rows are a block of their
      // own, and the words -- shared by the slots -- come out of the first one's
      const bool own = reinterpret_cast<int *>(r->d_small.p + l.err_words) == r->d_err.p;
      HIPCHK(hipMemcpyAsync(r->h_small, r->d_small.p, sizeof(double) * (own ? l.count : l.err_words), hipMemcpyDeviceToHost, r->stream));
      if (!own) HIPCHK(hipMemcpyAsync(r->h_errflag, r->d_err.p, 2 * sizeof(int), hipMemcpyDeviceToHost, r->stream));
    }
    HIPCHK(hipStreamSynchronize(r->stream));
    resolve_events(r);
    if (r->comm) r->comm_status = r->h_small[l.status];
    if (!r->holds.column || !recover_fused_timeout(r)) break;  // re-issued unfused: fetch again
  }
  f_total_row(r->h_small, l);   // no kernel forms a call's f_total
  r->holds.rows_fetched();
}

bool check_dims(Radtran *r, int dim_T, int dim_P, int d1, int d2, int dim_dz, int has_p, int p1, int p2,
                int r1, int r2, const double *pdens, const double *radii, char *err) {
  // check_inputs / check_dimensions(_p), clima_radtran.f90:417-491 (same texts)
  if (has_p && ((pdens && !radii) || (radii && !pdens))) { set_err(err, "Both pdensities and radii must be arguments."); return false; }
  if (r->np > 0 && (!has_p || !radii)) { set_err(err, "The model contains particles but \"pdensities\" and \"radii\" are not arguments."); return false; }
  if (dim_T != r->nz) { set_err(err, "\"T\" has the wrong input dimension."); return false; }
  if (dim_P != r->nz) { set_err(err, "\"P\" has the wrong input dimension."); return false; }
  if (d1 != r->nz || d2 != r->nsp) { set_err(err, "\"densities\" has the wrong input dimension."); return false; }
  if (dim_dz != r->nz) { set_err(err, "\"dz\" has the wrong input dimension."); return false; }
  if (has_p && radii) {
    if (p1 != r->nz || p2 != r->np) { set_err(err, "\"pdensities\" has the wrong input dimension."); return false; }
    if (r1 != r->nz || r2 != r->np) { set_err(err, "\"radii\" has the wrong input dimension."); return false; }  // :458-461
  }
  return true;
}

void do_upload(Radtran *r, const ColumnArrays &a) {
  const int nz = r->nz;
  double *h = r->h_col;
  settle_pending_batch(r);   // (a pending integration stays: it does not read the column)
  // the pinned staging buffer is reused: wait (lazily, here) for the previous upload's copy
  if (r->upload_pending) { HIPCHK(hipEventSynchronize(r->ev_upload)); r->upload_pending = false; }
  r->nsrc = pack_column(r, h, a);
  const int *meta = reinterpret_cast<const int *>(h + r->col_layout.meta);
  bool all = (nz % 2 == 0) && r->nsrc * 2 == nz;
  for (int m = 0; m < r->nsrc && all; m++) all = (meta[1 + m] & SRC_EXACT) != 0;
  r->all_pairs_exact = all;
  // The column goes into the block of the slot the handle's next call is expected to take, on that slot's lane: the
  // other one when that call would run beside the previous pipelined call (a call that then takes the current slot
  // after all copies the column over: ensure_column).  Otherwise into the current slot's, behind a join -- its latest
  // call may be reading that block on the other lane.
  const bool to_other = r->holds.unjoined && pipelining_two(r);
  if (to_other) ensure_other_slot(r); else join_lanes(r);
  {
    LaneScope lane(r, to_other ? r->lane ^ 1 : 0);
    double *d_col = to_other ? r->other.d_col.p : r->d_col.p;
    wait_for_column_copy(r, d_col);
    // ~18 KB: a kernel that reads the pinned buffer over PCIe gets the column into HBM 4 us sooner
    // than the copy engine does (which takes over where the runtime did not map the buffer)
    if (r->h_col_dev) launch_copy(d_col, r->h_col_dev, r->col_layout.count, r->stream);
    else HIPCHK(hipMemcpyAsync(d_col, h, sizeof(double) * r->col_layout.count, hipMemcpyHostToDevice, r->stream));
    HIPCHK(hipEventRecord(r->ev_upload, r->stream));
    (to_other ? r->other.col_upload : r->col_upload) = r->holds.uploads + 1;   // (counted by Holds::uploaded below)
  }
  r->upload_pending = true;
  r->last_T.assign(a.T, a.T + nz);
  r->last_P.assign(a.P, a.P + nz);
  if (r->np > 0 && a.radii) r->last_radii.assign(a.radii, a.radii + (size_t)nz * r->np); else r->last_radii.clear();
  r->holds.uploaded(a.has_particles());
}

// A two-stream block of the fused grid gave up waiting for its bin's opacity blocks (k_fused: the
// wait is bounded; it can expire when the device is time-sliced with another process, or if blocks
// were ever dispatched out of index order).  Nothing is wrong with the inputs: the stale parts are
// computed again through the separate launches.  h_errflag[1] must be current (fetch_small /
// radtran_synchronize).  Opacities and IR results are stale when the last opacity pass timed out,
// the solar results when the pass of the last solar computation did.
const char *const REPLACED_MSG = "The fused opacity/two-stream hand-off of an earlier opacity pass timed out and the column has "
                                 "been replaced since: repeat the steps from that opacity pass on.";
bool recover_fused_timeout(Radtran *r) {
  if (r->comm) {
    // With a communicator the partial rows are already summed when the host looks: the step is repeated by
    // EVERY rank -- each learns of any rank's expired wait from the reduced status word -- through the separate
    // launches, collective included.  The repeat's own status word is 0 (its passes have new ids).
    const double st = r->comm_status;
    if (!(st > 0.0)) return false;
    r->comm_status = 0.0;
    r->checked_timeout = r->call_id;
    if (std::fmod(st, 1024.0) > 0.0 && !r->holds.opr_from_resident_column()) throw HipFail{REPLACED_MSG};
    r->fused_fallbacks++;
    enqueue_radiate(r, resident_bufs(r), st >= 1024.0 || r->last_cs, true, false);
    return true;
  }
  const int t = r->h_errflag[1];
  if (t <= r->checked_timeout) return false;
  r->checked_timeout = r->call_id;
  const bool stale_opr = t == r->call_id, stale_sol = t == r->solar_id;
  if (!stale_opr && !stale_sol) return false;
  if (r->shard_world > 1)  // reduced by the CALLER (no communicator on the handle): this step cannot be redone here
    throw HipFail{"The fused opacity/two-stream hand-off timed out on a bin-sharded handle whose all-reduce is the caller's; "
                  "repeat the step (radtran_fused_set(0) selects the separate launches; with radtran_comm_init_rank the "
                  "library repeats it itself)."};
  // the stored opacities came from a column that has been replaced since (upload A, opacity pass, upload B, a
  // compute_opacity = .false. pass): computing them again from column B is not what the caller asked for
  if (stale_opr && !r->holds.opr_from_resident_column()) throw HipFail{REPLACED_MSG};
  r->fused_fallbacks++;
  enqueue_radiate(r, resident_bufs(r), stale_sol || r->last_cs, true, false);
  return true;
}

constexpr const char *OPACITY_FAILED_MSG = "Opacity computation failed in one or more wavelength bins.";  // clima_radtran_types.f90:773-776
bool surface_device_error(Radtran *r, char *err) {
  const bool failed = *r->h_errflag > r->checked_id;  // a call since the last check flagged
  r->checked_id = r->call_id;
  if (failed) set_err(err, OPACITY_FAILED_MSG);
  return failed;
}

// The two error words (opacity failure, expired fused hand-off wait: the ids of the last calls that flagged them) as
// they stand once everything enqueued so far has run
void wait_error_words(Radtran *r) {
  join_lanes(r);
  HIPCHK(hipMemcpyAsync(r->h_errflag, r->d_err.p, 2 * sizeof(int), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  resolve_events(r);
}

// Everything enqueued so far has run, and a fused hand-off that timed out has been repaired: after this the
// device buffers hold the call's results (what fetch_small does for the level rows; the per-bin spectra and the
// optical properties are read out after this)
void settle(Radtran *r) {
  settle_device_batch(r);
  for (int pass = 0; pass < 2; pass++) {
    if (r->comm && !r->holds.rows_on_host)   // the reduced status word (the rows themselves are fetched when they are read)
      HIPCHK(hipMemcpyAsync(&r->comm_status, r->d_small.p + r->rows.status, sizeof(double), hipMemcpyDeviceToHost, r->stream));
    wait_error_words(r);
    if (!r->holds.column || !recover_fused_timeout(r)) break;
  }
}

// ... and what works on the stored optical properties next finds them whole: fields current, w0 in memory
// (a communicator handle: the level rows of the last step are the reduced ones from here on)
void ready_stored_opacities(Radtran *r) {
  settle(r);
  upload_fields(r);
  ensure_w0(r);
}

void defer_err(Radtran *r, const std::string &msg) {
  if (r && r->deferred_err.empty()) r->deferred_err = msg;
}

// ---- column batches (radtran_toa_fluxes_batch, radtran_toa_fluxes_batch_device): one path, two sinks ----
// An earlier batch's checks (and its repeat, which reads the arena this one overwrites), then room for n columns'
// blocks and level rows (and their source-layer counts, where the device finds them); with_bounds: and for their bounds
// blocks behind the column blocks (batch_bounds_base)
void begin_batch(Radtran *r, int n, bool nsrc_on_device, bool with_bounds = false) {
  settle_device_batch(r);
  r->d_cols_arena.reserve((size_t)n * (r->col_layout.count + (with_bounds ? handle_bounds_layout(r).count : 0)));
  r->d_flux_arena.reserve(n * r->rows.stride);
  if (nsrc_on_device) r->d_batch_nsrc.reserve(n);
}
double *batch_bounds_base(Radtran *r, int n) { return r->d_cols_arena.p + (size_t)n * r->col_layout.count; }
// The launch form of a batch of n columns, decided here, once: one launch of each kernel per chunk of CH columns
// (the fused grid takes the columns' work items in turn, so one column's two-stream tail runs beside the next
// column's opacity tiles) where the fused form covers the configuration -- the per-column arenas of a chunk are
// sized here --, otherwise the columns' calls back to back.
BatchRun batch_form(Radtran *r, int n) {
  BatchRun f;
  f.n = n; f.first_call = r->call_id + 1; f.CH = std::min(n, r->batch_cols_in_flight);
  const CallBufs first = arena_chunk_bufs(r, 0, f.CH);   // the first chunk (only its counts are read)
  f.one_launch = plan_radiate(plan_input(r, first, true, true, true)).fused.form != TS_NONE &&
                 integrate_fits_one_launch(integrate_chunks(std::max(r->ir_n, r->sol_n)));
  if (const char *e = getenv("CLIMA_HIP_BATCH_ONE_LAUNCH")) f.one_launch = f.one_launch && atoi(e) != 0;
  if (f.one_launch) {
    const BatchStrides &bs = first.bs;
    r->d_prep_arena.reserve(bs.prep * f.CH);
    r->d_opr_arena.reserve(bs.opr * f.CH);
    if (r->d_res_arena.reserve(bs.res * f.CH)) r->d_res_arena.zero(r->stream);
    if (r->d_done.reserve((size_t)bs.done * f.CH + 1)) r->d_done.zero(r->stream);
  }
  return f;
}
// the columns' source-layer counts as k_pack_columns found them (4 bytes each): the launches of one call per column are sized by them
void fetch_batch_nsrc(Radtran *r, int n) {
  r->batch_nsrc.resize(n);
  HIPCHK(hipMemcpyAsync(r->batch_nsrc.data(), r->d_batch_nsrc.p, sizeof(int) * n, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
}
// The batch whose column blocks are in d_cols_arena and whose source-layer counts are in batch_nsrc, start to end: the
// chunks (or the columns' calls), the rows out to the sink, the handle's own level rows = the last column's.  Nothing waits.
void enqueue_batch(Radtran *r, const BatchRun &b, bool allow_fused) {
  const int n = b.n, nl = r->nz + 1;
  const LevelRows &l = r->rows;
  // the rows asked for out of the `ncol` columns from c0 on that the launches just enqueued worked on, before the next
  // ones overwrite their spectra (the arena of a chunk, the handle's own buffers of a column's call)
  auto gather = [&](const CallBufs &cb, int c0, int ncol) {
    if (!b.nsel) return;
    BatchSpectraParams p{};
    p.ncol = ncol; p.nsel = b.nsel; p.nl = nl; p.level = b.spec_level; p.src_stride = cb.bs.res;
    const double *const src[4] = {cb.spec.ir_fup_a, cb.spec.ir_fdn_a, cb.spec.sol_fup_a, cb.spec.sol_fdn_a};
    for (int k = 0; k < 4; k++) {
      p.nw[k] = k < 2 ? r->ir.nw : r->sol.nw;
      p.src[k] = src[k];
      p.dst[k] = b.spec[k] ? b.spec[k] + (size_t)c0 * b.nsel * p.nw[k] : nullptr;
    }
    launch_batch_spectra(p, r->stream);
    HIPCHK(hipGetLastError());
  };
  if (b.one_launch && allow_fused) {
    for (int c0 = 0; c0 < n; c0 += b.CH) {
      const CallBufs cb = arena_chunk_bufs(r, c0, std::min(b.CH, n - c0), b.bounds, b.bounds_count);
      enqueue_radiate(r, cb, true, true);
      gather(cb, c0, cb.ncol);
    }
  } else {
    for (int c = 0; c < n; c++) {
      const CallBufs cb = arena_column_bufs(r, c, r->batch_nsrc[c], b.bounds, b.bounds_count);
      enqueue_radiate(r, cb, true, true, allow_fused);
      gather(cb, c, 1);
    }
  }
  if (b.rows) {
    HIPCHK(hipMemcpyAsync(b.rows, r->d_flux_arena.p, sizeof(double) * n * l.stride, hipMemcpyDeviceToHost, r->stream));
    if (b.spec_count) HIPCHK(hipMemcpyAsync(b.spec_host, r->d_spec_stage.p, sizeof(double) * b.spec_count, hipMemcpyDeviceToHost, r->stream));
  } else {
    launch_batch_finish(BatchFinishParams{n, r->nz, r->d_flux_arena.p, b.ISR, b.OLR, b.fluxes}, r->stream);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(r->d_flux_n.p, r->d_flux_arena.p + (n - 1) * l.stride, sizeof(double) * l.flux_count, hipMemcpyDeviceToDevice, r->stream));
}
// What the handle holds after a batch is the LAST column's, like after n single calls: its level rows (enqueue_batch),
// and its spectra / band optical depths -- the one-launch form left those in the batch arena (copied here); its optical
// properties stay in the arena (Holds::batch_left: an IR-only call needs a compute_opacity call first).  One call per
// column works in the handle's own buffers; so does a repeat (settle_batch), which overwrites what is copied here.
void batch_leaves_handle(Radtran *r, const BatchRun &b) {
  r->holds.batch_left(b.one_launch, r->np);   // (d_col does not hold the last column: a resident call needs an upload first)
  if (!b.one_launch) return;
  const SpectraViews src = spectra_views(r, r->d_res_arena.p + (size_t)((b.n - 1) % b.CH) * spectra_views(r, nullptr).count);
  auto d2d = [&](DevBuf<double> &dst, const double *from) { HIPCHK(hipMemcpyAsync(dst.p, from, sizeof(double) * dst.n, hipMemcpyDeviceToDevice, r->stream)); };
  d2d(r->wrk_ir.fup_a, src.ir_fup_a); d2d(r->wrk_ir.fdn_a, src.ir_fdn_a); d2d(r->wrk_ir.tau_band, src.ir_tau_band);
  d2d(r->wrk_sol.fup_a, src.sol_fup_a); d2d(r->wrk_sol.fdn_a, src.sol_fdn_a); d2d(r->wrk_sol.amean, src.sol_amean);
  d2d(r->wrk_sol.tau_band, src.sol_tau_band);
}
// Everything the batch enqueued has run, and a fused hand-off wait that expired in one of its calls has been repaired:
// the whole batch again through the separate launches (the column blocks are still in the arena, the results go to the
// same sink).  Returns whether one of its calls flagged an opacity failure.
bool settle_batch(Radtran *r, const BatchRun &b) {
  wait_error_words(r);
  if (r->h_errflag[1] >= b.first_call) {
    r->fused_fallbacks++;
    if (b.one_launch && !b.rows) fetch_batch_nsrc(r, b.n);   // (the host's pack_column returned them)
    enqueue_batch(r, b, false);
    wait_error_words(r);
    r->holds.batch_repeated();
  }
  r->checked_timeout = r->checked_id = r->call_id;
  r->holds.rows_changed();
  return *r->h_errflag >= b.first_call;
}
// What the handle still owes before anything else is enqueued or read: a resident call's integration that was kept
// back (alone, now) and a device batch's checks (an opacity failure kept for the next call that reports errors)
void settle_device_batch(Radtran *r) {
  resolve_pending_integration(r);
  settle_pending_batch(r);
}
void settle_pending_batch(Radtran *r) {
  if (!r->dev_batch.pending) return;
  r->dev_batch.pending = false;
  if (settle_batch(r, r->dev_batch)) defer_err(r, OPACITY_FAILED_MSG);
}
// the parameter block of k_pack_bounds: the bounds blocks of a batch built on the device (the handle's device copies of
// its fields must be current: upload_fields)
PackBoundsParams make_pack_bounds_params(Radtran *r, int n, const BoundsArrays &in, double *blocks) {
  PackBoundsParams p;
  std::memset(&p, 0, sizeof(p));
  p.ncol = n; p.l = handle_bounds_layout(r);
  p.in = in;
  p.own = BoundsArrays{r->d_albedo.p, r->d_emis.p, r->d_zen_u.p, r->d_zen_w.p, nullptr};
  p.own_scale = r->photon_scale_factor;
  p.blocks = blocks;
  return p;
}
// the parameter block of k_pack_columns: the column blocks of a batch built on the device
PackParams make_pack_params(Radtran *r, int n, const ColumnArrays &in, double *blocks, int *nsrc) {
  PackParams p;
  std::memset(&p, 0, sizeof(p));
  p.ncol = n; p.nz = r->nz; p.nsp = r->nsp; p.np = r->np;
  p.has_particles = r->np > 0 && in.has_particles();
  p.use_radii = p.has_particles && !r->part.empty();
  p.in = in;
  p.blocks = blocks; p.nsrc = nsrc;
  return p;
}
// A communicator handle worked on its share of the bins: ONE all-reduce of the up / down arrays (2 arr doubles from the
// start of d_bout) over the ranks, then the total from the reduced ones, which `total` launches.
template <class F>
void comm_reduce_up_down(Radtran *r, size_t arr, F total) {
  if (!r->comm) return;
  NCCLCHK(ncclAllReduce(r->d_bout.p, r->d_bout.p, 2 * arr, ncclDouble, ncclSum, r->comm, r->stream));
  r->comm_reduces++;
  total();
  HIPCHK(hipGetLastError());
}

// The Jacobian kernels' launches (`launch`), `count` doubles from the start of d_bout -- or, on a shard without IR bins,
// no k_green_* kernel (their grids would be empty): zeros into the all-reduce
template <class F>
void jacobian_of_ir_bins(Radtran *r, size_t count, F launch) {
  if (r->ir_n > 0) { launch(); HIPCHK(hipGetLastError()); }
  else HIPCHK(hipMemsetAsync(r->d_bout.p, 0, sizeof(double) * count, r->stream));
}

// device memory of the handle's device?  (an address the runtime does not know -- pageable host memory -- is an
// error return on some runtimes and "unregistered" on others)
bool on_handle_device(const Radtran *r, const void *p) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == r->device;
}

void get2d(WrkObj *w, DevBuf<double> &buf, int dim1, int dim2, double *arr) {
  Radtran *r = w->parent;
  if (!r->holds.rows_on_host) settle(r);   // (valid rows: the call was synchronised and checked when they were fetched, nothing enqueued since)
  size_t n = std::min((size_t)dim1 * dim2, buf.n);
  if (n) HIPCHK(hipMemcpy(arr, buf.p, n * sizeof(double), hipMemcpyDeviceToHost));
}

}  // namespace

#define GUARD(r, ptr, err)                                   \
  Radtran *r = as_rad(ptr);                                  \
  if (!r) { set_err(err, "invalid Radtran handle"); return; }
// ... of a handle that radtran_create_end has finished
#define GUARD_BUILT(r, ptr, err) \
  GUARD(r, ptr, err)             \
  if (r->state != 2) { set_err(err, "Radtran is not constructed"); return; }
#define TRY try {
#define CATCH(err) } catch (const HipFail &f) { set_err(err, f.msg); } catch (const std::exception &e) { set_err(err, e.what()); }

// The environment's say in how a handle runs, read once while the handle is made (radtran_create_begin), before the
// first use of any of it.  INTEGRATION.md lists every name the library reads.
static void read_handle_switches(Radtran *r) {
  if (const char *f = getenv("CLIMA_HIP_FUSED")) r->fused = atoi(f) != 0;
  if (const char *f = getenv("CLIMA_HIP_TS_MODE")) r->ts_block_mode = std::strcmp(f, "block") == 0;
  if (const char *f = getenv("CLIMA_HIP_BATCH_SHARED")) r->batch_shared = atoi(f) != 0;
  if (const char *f = getenv("CLIMA_HIP_IR_GREEN")) r->ir_green_mode = std::max(0, std::min(2, atoi(f)));
  if (const char *f = getenv("CLIMA_HIP_FUSED_SPINS")) r->fused_max_spins = std::max(0, atoi(f));  // test aid: 0 makes waits expire
  if (const char *f = getenv("CLIMA_HIP_BATCH_COLS")) r->batch_cols_in_flight = std::max(1, atoi(f));
  if (const char *f = getenv("CLIMA_HIP_COOP_ITEMS")) r->coop_items = atol(f);
  if (const char *f = getenv("CLIMA_HIP_REBIN")) r->rebin_stream = std::strcmp(f, "stream") == 0;
}

extern "C" {

void allocate_radtran(void **ptr) { *ptr = new Radtran(); }
void deallocate_radtran(void *ptr) {
  Radtran *r = as_rad(ptr);
  if (r) delete r;
}

void radtran_create_begin(void *ptr, const int *nz, const int *nsp, const int *np, const int *nw,
                          const double *wavl, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (*nz < 1) { set_err(err, "\"nz\" can not be less than 1."); return; }  // clima_radtran.f90:149-152
  if (*nw < 1 || *nsp < 1 || *np < 0) { set_err(err, "invalid dimensions"); return; }
  if (*np > MAX_PART) { set_err(err, "too many particle species for this build"); return; }
  r->nz = *nz; r->nsp = *nsp; r->np = *np; r->nw = *nw;
  r->wavl.assign(wavl, wavl + *nw + 1);
  r->freq.resize(*nw + 1);
  for (int i = 0; i < *nw + 1; i++) r->freq[i] = C_LIGHT / (wavl[i] * 1.0e-9);  // types_create.f90:361
  read_handle_switches(r);
  r->state = 1;
}

void radtran_add_ktable(void *ptr, const int *sp_ind, const int *ngauss, const double *weights,
                        const int *npress, const double *log10P, const int *ntemp, const double *temp,
                        const double *log10k, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_add_ktable: call between create_begin and create_end"); return; }
  if (*sp_ind < 1 || *sp_ind > r->nsp) { set_err(err, "k-distribution species index out of range"); return; }
  if ((int)r->k.size() >= MAX_K) { set_err(err, "too many k-distributions for this build"); return; }
  if (!r->k.empty() && *ngauss != r->ng) { set_err(err, "all k-distributions must share the same g-points"); return; }
  if (*npress < 2 || *ntemp < 2) { set_err(err, "k-distribution grids need at least 2 nodes"); return; }
  auto *k = new KTabHost();
  k->sp = *sp_ind - 1; k->ng = *ngauss; k->nP = *npress; k->nT = *ntemp;
  k->weights.assign(weights, weights + *ngauss);
  k->log10P.assign(log10P, log10P + *npress);
  k->temp.assign(temp, temp + *ntemp);
  k->log10k.assign(log10k, log10k + (size_t)r->nw * *ntemp * *npress * *ngauss);
  if (r->k.empty()) {  // create_Ksettings, types_create.f90:191-224; weight_e :1303-1304
    r->ng = *ngauss;
    r->wbin = k->weights;
    weight_edges_and_products(r->wbin, r->wbin_e, r->wxy);
    r->rebin_mode = rebin_mode_for(r->wbin, r->wbin_e, r->wxy, r->rebin_stream);
  }
  r->k.push_back(k);
}

void radtran_add_xsection(void *ptr, const int *xs_type, const int *dim, const int *sp_ind1,
                          const int *sp_ind2, const int *ntemp, const double *temp, const double *data,
                          char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_add_xsection: call between create_begin and create_end"); return; }
  std::vector<XsHost *> *list;
  if (*xs_type == CLIMA_XS_CIA) list = &r->cia;
  else if (*xs_type == CLIMA_XS_RAYLEIGH) list = &r->ray;
  else if (*xs_type == CLIMA_XS_PHOTOLYSIS || *xs_type == CLIMA_XS_ABSORPTION) list = &r->pxs;
  else { set_err(err, "unknown cross-section type"); return; }
  if ((int)list->size() >= MAX_XS) { set_err(err, "too many cross sections for this build"); return; }
  if (*dim != 0 && *dim != 1) { set_err(err, "cross-section dim must be 0 or 1"); return; }
  if (*xs_type == CLIMA_XS_RAYLEIGH && *dim != 0) { set_err(err, "Rayleigh cross sections are 0-D"); return; }
  if (*sp_ind1 < 1 || *sp_ind1 > r->nsp) { set_err(err, "cross-section species index out of range"); return; }
  if (*xs_type == CLIMA_XS_CIA && (*sp_ind2 < 1 || *sp_ind2 > r->nsp)) { set_err(err, "CIA species index out of range"); return; }
  if (*dim == 1 && *ntemp < 2) { set_err(err, "1-D cross sections need at least 2 temperatures"); return; }
  auto *x = new XsHost();
  x->type = *xs_type; x->dim = *dim; x->sp1 = *sp_ind1 - 1; x->sp2 = (*xs_type == CLIMA_XS_CIA) ? *sp_ind2 - 1 : -1;
  x->nT = *dim ? *ntemp : 0;
  if (*dim) x->temp.assign(temp, temp + *ntemp);
  x->data.assign(data, data + (*dim ? (size_t)r->nw * *ntemp : (size_t)r->nw));
  list->push_back(x);
}

void radtran_set_water_continuum(void *ptr, const int *LH2O, const int *ntemp, const double *temp,
                                 const double *log10_xs_H2O, const double *log10_xs_foreign, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_set_water_continuum: call between create_begin and create_end"); return; }
  if (*LH2O < 1 || *LH2O > r->nsp || *ntemp < 2) { set_err(err, "invalid water continuum arguments"); return; }
  r->has_cont = true; r->LH2O = *LH2O - 1; r->cont_nT = *ntemp;
  r->cont_temp.assign(temp, temp + *ntemp);
  r->cont_H2O.assign(log10_xs_H2O, log10_xs_H2O + (size_t)r->nw * *ntemp);
  r->cont_foreign.assign(log10_xs_foreign, log10_xs_foreign + (size_t)r->nw * *ntemp);
}

void radtran_add_particle(void *ptr, const int *p_ind, const int *nrad, const double *radii,
                          const double *w0, const double *qext, const double *gt, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_add_particle: call between create_begin and create_end"); return; }
  if (*p_ind < 1 || *p_ind > r->np || *nrad < 2) { set_err(err, "invalid particle arguments"); return; }
  if ((int)r->part.size() >= MAX_PART) { set_err(err, "too many particles for this build"); return; }
  auto *p = new PartHost();
  p->p_ind = *p_ind - 1; p->nrad = *nrad;
  size_t n = (size_t)r->nw * *nrad;
  p->radii.assign(radii, radii + *nrad);
  p->w0.assign(w0, w0 + n); p->qext.assign(qext, qext + n); p->gt.assign(gt, gt + n);
  r->part.push_back(p);
}

void radtran_set_channels(void *ptr, const int *n_ir_edges, const double *ir_wavl, const int *n_sol_edges,
                          const double *sol_wavl, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_set_channels: call between create_begin and create_end"); return; }
  if (*n_ir_edges < 2 || *n_sol_edges < 2) { set_err(err, "channels need at least one bin"); return; }
  if (!make_channel(r, r->ir, 0, *n_ir_edges, ir_wavl, err)) return;
  if (!make_channel(r, r->sol, 1, *n_sol_edges, sol_wavl, err)) return;
}

void radtran_set_photons_sol(void *ptr, const int *n, const double *photons_sol, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->sol.nw == 0 || *n != r->sol.nw) { set_err(err, "\"photons_sol\" has the wrong size"); return; }
  r->photons_sol.assign(photons_sol, photons_sol + *n);
  r->fields_dirty = true;
}

// futils v0.1.14 interp(xg, x, y, yg, ierr=) as called at types.f90:487-497: piecewise linear,
// constant beyond both ends (linear_extrap defaults to false); nonzero when x is not ascending
static int futils_interp(const std::vector<double> &xg, int n, const double *x, const double *y, double *yg) {
  if (n < 1) return -1;
  for (int i = 1; i < n; i++) if (!(x[i] > x[i - 1])) return -2;
  for (size_t i = 0; i < xg.size(); i++) {
    const double xv = xg[i];
    if (xv <= x[0]) yg[i] = y[0];
    else if (xv >= x[n - 1]) yg[i] = y[n - 1];
    else {
      int lo = 0, hi = n - 1;
      while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (xv < x[mid]) hi = mid; else lo = mid; }
      const double slope = (y[lo + 1] - y[lo]) / (x[lo + 1] - x[lo]);
      yg[i] = y[lo] + slope * (xv - x[lo]);
    }
  }
  return 0;
}

// clima/fortran/Radtran.f90:77-107 -> Radtran_set_custom_optical_properties (clima_radtran.f90:494-506)
// -> OpticalProperties_set_custom_optical_properties (clima_radtran_types.f90:432-538)
void radtran_set_custom_optical_properties(void *ptr, const int *dim_wv, const double *wv, const int *dim_P,
                                           const double *P, const int *dim1_dtau_dz, const int *dim2_dtau_dz,
                                           const double *dtau_dz, const int *dim1_w0, const int *dim2_w0,
                                           const double *w0, const int *dim1_g0, const int *dim2_g0,
                                           const double *g0, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nwv = *dim_wv, nP = *dim_P;
  for (int i = 0; i < nwv; i++) if (wv[i] <= 0.0) { set_err(err, "All elements of `wv` must be larger than zero"); return; }
  for (int i = 0; i < nP; i++) if (P[i] <= 0.0) { set_err(err, "All elements of `P` must be larger than zero"); return; }
  if (nP != *dim1_dtau_dz) { set_err(err, "`P` and `dtau_dz` have incompatible shapes"); return; }
  if (nwv != *dim2_dtau_dz) { set_err(err, "`wv` and `dtau_dz` have incompatible shapes"); return; }
  if (nP != *dim1_w0) { set_err(err, "`P` and `w0` have incompatible shapes"); return; }
  if (nwv != *dim2_w0) { set_err(err, "`wv` and `w0` have incompatible shapes"); return; }
  if (nP != *dim1_g0) { set_err(err, "`P` and `g0` have incompatible shapes"); return; }
  if (nwv != *dim2_g0) { set_err(err, "`wv` and `g0` have incompatible shapes"); return; }
  TRY
  const int nw = r->nw;
  std::vector<double> wv1(nw), row(nwv), tmp(nw);
  for (int i = 0; i < nw; i++) wv1[i] = 0.5 * (r->wavl[i + 1] + r->wavl[i]);  // :479
  std::vector<double> tab[3];
  const double *src[3] = {dtau_dz, w0, g0};
  for (auto &t : tab) t.assign((size_t)nw * nP, 0.0);
  for (int i = 0; i < nP; i++) {
    const int j = nP - 1 - i;  // :483
    for (int a = 0; a < 3; a++) {
      for (int k = 0; k < nwv; k++) row[k] = src[a][i + (size_t)k * nP];
      if (futils_interp(wv1, nwv, wv, row.data(), tmp.data()) != 0) {
        set_err(err, "Interpolation error in `set_custom_optical_properties`");
        return;
      }
      for (int l = 0; l < nw; l++) tab[a][(size_t)l * nP + j] = tmp[l];
    }
  }
  std::vector<double> lp(nP);
  for (int i = 0; i < nP; i++) lp[nP - 1 - i] = std::log10(P[i]);  // :505-506
  bool ok = nP >= 2;  // linear_interp_1d%initialize: two or more strictly increasing nodes
  for (int i = 1; i < nP && ok; i++) ok = lp[i] > lp[i - 1];
  if (!ok) { set_err(err, "Interpolation initialization error in `set_custom_optical_properties`"); return; }
  drain_lanes(r);  // a previous call may still read the old tables
  r->cust_axis = lp; r->cust_nP = nP;
  r->d_cust_axis.upload(lp); r->d_cust_dtau.upload(tab[0]); r->d_cust_w0.upload(tab[1]); r->d_cust_g0.upload(tab[2]);
  r->cust_on = true;
  CATCH(err)
}

static std::vector<std::string> split_lines(const char *s) {
  std::vector<std::string> out;
  if (!s) return out;
  std::string cur;
  for (const char *c = s; *c; c++) {
    if (*c == '\n') { out.push_back(cur); cur.clear(); } else cur.push_back(*c);
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

// Names the loaders know and opacities2yaml prints: species / particles in index order, one per
// line (OpticalProperties%species_names, %particle_names, clima_radtran_types.f90:100-101)
void radtran_set_names(void *ptr, const char *species_names, const char *particle_names, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  auto sp = split_lines(species_names), pa = split_lines(particle_names);
  if (r->state >= 1 && ((int)sp.size() != r->nsp || (int)pa.size() != r->np)) {
    set_err(err, "radtran_set_names: the number of names does not match the number of species / particles");
    return;
  }
  r->species_names = sp; r->particle_names = pa;
}

// k-method name (Ksettings%k_method_name), water-continuum model (WaterContinuum%model) and the
// data-set name of every particle cross section in the order they were added (ParticleXsection%dat_name)
void radtran_set_opacity_labels(void *ptr, const char *k_method, const char *water_continuum_model,
                                const char *particle_data, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (k_method && k_method[0]) r->k_method_name = k_method;
  if (water_continuum_model && water_continuum_model[0]) r->continuum_model = water_continuum_model;
  r->particle_data = split_lines(particle_data);
}

// OpticalProperties_opacities2yaml, clima_radtran_types.f90:328-430 (line by line)
static std::string opacities2yaml(Radtran *r) {
  auto sp = [&](int i) { return (i >= 0 && i < (int)r->species_names.size()) ? r->species_names[i] : ("species" + std::to_string(i + 1)); };
  auto join = [](const std::vector<std::string> &v) {
    std::string o;
    for (size_t i = 0; i < v.size(); i++) { o += v[i]; if (i + 1 != v.size()) o += ", "; }
    return o;
  };
  std::string out = "  k-method: " + r->k_method_name;
  out += "\n  opacities:";
  if (!r->k.empty()) {
    std::vector<std::string> v;
    for (auto *k : r->k) v.push_back(sp(k->sp));
    out += "\n    k-distributions: [" + join(v) + "]";
  }
  if (!r->cia.empty()) {
    std::vector<std::string> v;
    for (auto *x : r->cia) v.push_back(sp(x->sp1) + "-" + sp(x->sp2));
    out += "\n    CIA: [" + join(v) + "]";
  }
  if (!r->ray.empty()) {
    std::vector<std::string> v;
    for (auto *x : r->ray) v.push_back(sp(x->sp1));
    out += "\n    rayleigh: [" + join(v) + "]";
  }
  if (!r->pxs.empty()) {
    std::vector<std::string> v;
    for (auto *x : r->pxs) v.push_back(sp(x->sp1));
    out += "\n    photolysis-xs: [" + join(v) + "]";
  }
  if (r->has_cont) out += "\n    water-continuum: " + r->continuum_model;
  if (!r->part.empty()) {
    std::vector<std::string> v;
    for (size_t i = 0; i < r->part.size(); i++) {
      const int pi = r->part[i]->p_ind;
      const std::string name = (pi >= 0 && pi < (int)r->particle_names.size()) ? r->particle_names[pi] : ("particle" + std::to_string(pi + 1));
      const std::string dat = i < r->particle_data.size() ? r->particle_data[i] : std::string("unknown");
      v.push_back("{name: " + name + ", data: " + dat + "}");
    }
    out += "\n    particle-xs: [" + join(v) + "]";
  }
  return out;
}

// clima/fortran/Radtran.f90:41-75: _1 allocates the C string and returns its length, _2 copies it
// into the caller's buffer (out_len + 1 chars) and frees it
void radtran_opacities2yaml_wrapper_1(void *ptr, int *out_len, void **out_cp) {
  Radtran *r = as_rad(ptr);
  const std::string s = r ? opacities2yaml(r) : std::string();
  char *buf = (char *)std::malloc(s.size() + 1);
  std::memcpy(buf, s.c_str(), s.size() + 1);
  *out_len = (int)s.size();
  *out_cp = buf;
}
void radtran_opacities2yaml_wrapper_2(void *ptr, void **out_cp, const int *out_len, char *out_c) {
  (void)ptr;
  if (!out_cp || !*out_cp) return;
  std::memcpy(out_c, *out_cp, (size_t)*out_len + 1);
  std::free(*out_cp);
  *out_cp = nullptr;
}

void radtran_fused_set(void *ptr, const int *enable) {
  Radtran *r = as_rad(ptr);
  if (r) r->fused = (*enable != 0);
}
void radtran_fused_get(void *ptr, int *enabled) {
  Radtran *r = as_rad(ptr);
  *enabled = (r && r->fused) ? 1 : 0;
}
void radtran_coop_items_set(void *ptr, const int *items) {
  Radtran *r = as_rad(ptr);
  if (r) r->coop_items = *items;
}
void radtran_coop_items_get(void *ptr, int *items) {
  Radtran *r = as_rad(ptr);
  *items = r ? (int)std::min<long>(r->coop_items, 2147483647L) : 0;
}
void radtran_fused_spins_set(void *ptr, const int *spins) {
  Radtran *r = as_rad(ptr);
  if (r) r->fused_max_spins = std::max(0, *spins);
}
void radtran_fused_spins_get(void *ptr, int *spins) {
  Radtran *r = as_rad(ptr);
  *spins = r ? r->fused_max_spins : 0;
}
void radtran_ir_green_set(void *ptr, const int *mode) {
  Radtran *r = as_rad(ptr);
  if (r) r->ir_green_mode = std::max(0, std::min(2, *mode));
}
void radtran_ir_green_get(void *ptr, int *mode, int *batches) {
  Radtran *r = as_rad(ptr);
  *mode = r ? r->ir_green_mode : 0;
  *batches = r ? (int)std::min<long>(r->ir_green_batches, 2147483647L) : 0;
}
void radtran_solar_batch_shared_set(void *ptr, const int *on) {
  Radtran *r = as_rad(ptr);
  if (r) r->solar_batch_shared = *on != 0;
}
void radtran_solar_batch_shared_get(void *ptr, int *on, int *batches) {
  Radtran *r = as_rad(ptr);
  *on = r && r->solar_batch_shared ? 1 : 0;
  *batches = r ? (int)std::min<long>(r->solar_batch_shared_batches, 2147483647L) : 0;
}
void radtran_fused_fallbacks_get(void *ptr, int *count) {
  Radtran *r = as_rad(ptr);
  *count = r ? r->fused_fallbacks : 0;
}
void radtran_defer_integration_set(void *ptr, const int *enable) {
  Radtran *r = as_rad(ptr);
  if (r) r->defer_integration = (*enable != 0);
}
void radtran_defer_integration_get(void *ptr, int *enabled) {
  Radtran *r = as_rad(ptr);
  *enabled = (r && r->defer_integration) ? 1 : 0;
}
void clima_test_defer_allowed(const int *switch_on, const int *shard_world, const int *has_comm, const int *profile,
                              const int *capturing, const int *flux_ptr_taken, int *allowed) {
  *allowed = defer_allowed(*switch_on != 0, *shard_world, *has_comm != 0, *profile, *capturing != 0, *flux_ptr_taken != 0) ? 1 : 0;
}
void clima_test_plan_radiate(const int *in, int *out) {
  PlanIn p{};
  p.nz = in[0]; p.ng = in[1]; p.nzen = in[2]; p.n_ir = in[3]; p.n_sol = in[4]; p.op_n = in[5]; p.nsrc = in[6]; p.ncol = in[7];
  p.batch = in[8] != 0; p.ir_batch = in[9] != 0; p.rebin_mode = in[10]; p.cust_on = in[11] != 0;
  p.compute_opacity = in[12] != 0; p.all_pairs = in[13] != 0; p.fused = in[14] != 0; p.allow_fused = in[15] != 0;
  p.ts_block_mode = in[16] != 0; p.no_half = in[17] != 0; p.coop_items = in[18]; p.force_slots = in[19];
  const LaunchPlan pl = plan_radiate(p);
  int k = 0;
  out[k++] = pl.opacity; out[k++] = pl.coop_ng;
  for (const TsPlan *t : {&pl.fused, &pl.ts, &pl.block}) {
    out[k++] = t->form; out[k++] = t->slots; out[k++] = t->groups; out[k++] = t->per_launch; out[k++] = t->zero_launch ? 1 : 0;
  }
  out[k++] = pl.prep_clears ? 1 : 0; out[k++] = pl.caller_clears ? 1 : 0; out[k++] = pl.write_w0 ? 1 : 0;
  out[k++] = integrate_fits_one_launch(integrate_chunks(in[20])) ? 1 : 0;
  static_assert(CLIMA_PLAN_IN_N == 21 && CLIMA_PLAN_OUT_N == 2 + 3 * 5 + 4, "the orders documented in clima_radtran_hip.h");
}
void clima_test_handle_holds(const int *n, const int *events, int *out) {
  Holds h;
  const int shard_world = events[0], has_comm = events[1], op_lo = events[2], op_n = events[3];
  for (int i = 0; i < *n; i++) {
    const int *e = events + 4 + (size_t)i * CLIMA_HOLDS_EVENT_N;
    switch (e[0]) {
      case 0: h.uploaded(e[1] != 0); break;
      case 1: h.opacities_written(e[1] != 0, e[2] != 0, e[3] != 0, e[4], e[5]); break;
      case 2: h.w0_formed(); break;
      case 3: h.rows_enqueued(e[1] != 0); break;
      case 4: h.rows_changed(); break;
      case 5: h.rows_fetched(); break;
      case 6: h.batch_left(e[1] != 0, e[2]); break;
      case 7: h.batch_repeated(); break;
      case 8: h.results_dropped(); break;
      default: out[0] = -1; return;
    }
  }
  int k = 0;
  out[k++] = h.column; out[k++] = h.column_particles; out[k++] = (int)h.uploads;
  out[k++] = h.opr; out[k++] = h.w0_stored; out[k++] = (int)h.opr_upload; out[k++] = h.opr_lo; out[k++] = h.opr_n;
  out[k++] = h.rows_on_host; out[k++] = h.rows_in_pinned;
  for (int need : {NEED_COLUMN, NEED_OPACITIES, NEED_SPECTRUM}) out[k++] = refused(h, need, shard_world, has_comm != 0, op_lo, op_n) ? 1 : 0;
  out[k++] = h.opr_from_resident_column();
  static_assert(CLIMA_HOLDS_EVENT_N == 6 && CLIMA_HOLDS_OUT_N == 14, "the orders documented in clima_radtran_hip.h");
}
void clima_test_rebin_mode_for(const int *ng, const double *weights, const int *stream, int *mode) {
  std::vector<double> wbin(weights, weights + std::max(*ng, 0)), wbin_e, wxy;
  if (wbin.empty()) { *mode = -1; return; }
  weight_edges_and_products(wbin, wbin_e, wxy);
  *mode = rebin_mode_for(wbin, wbin_e, wxy, *stream != 0);
}
void radtran_merged_integrations_get(void *ptr, int *merged, int *standalone) {
  Radtran *r = as_rad(ptr);
  *merged = r ? (int)std::min<long>(r->merged_integrations, 2147483647L) : 0;
  *standalone = r ? (int)std::min<long>(r->standalone_integrations, 2147483647L) : 0;
}
void radtran_calls_in_flight_set(void *ptr, const int *mode) {
  Radtran *r = as_rad(ptr);
  if (r) r->calls_in_flight = std::max(0, std::min(2, *mode));
}
void radtran_calls_in_flight_get(void *ptr, int *mode) {
  Radtran *r = as_rad(ptr);
  *mode = r ? r->calls_in_flight : 0;
}
void radtran_overlapped_calls_get(void *ptr, int *count) {
  Radtran *r = as_rad(ptr);
  *count = r ? (int)std::min<long>(r->holds.overlapped, 2147483647L) : 0;
}
void clima_test_two_in_flight(const int *rule, const int *in, int *out) {
  PlanIn p{};
  p.nz = in[0]; p.ng = in[1]; p.nzen = in[2]; p.n_ir = in[3]; p.n_sol = in[4]; p.op_n = in[5]; p.nsrc = in[6]; p.ncol = in[7];
  p.batch = in[8] != 0; p.ir_batch = in[9] != 0; p.rebin_mode = in[10]; p.cust_on = in[11] != 0;
  p.compute_opacity = in[12] != 0; p.all_pairs = in[13] != 0; p.fused = in[14] != 0; p.allow_fused = in[15] != 0;
  p.ts_block_mode = in[16] != 0; p.no_half = in[17] != 0; p.coop_items = in[18]; p.force_slots = in[19];
  const long waves = radiate_grid_waves(p, plan_radiate(p));
  TwoInFlight q{};
  q.mode = rule[0];
  q.defer_ok = defer_allowed(rule[1] != 0, rule[2], rule[3] != 0, rule[4], rule[5] != 0, rule[6] != 0);
  q.prev_unjoined = rule[7] != 0; q.sampled = rule[8] != 0; q.cus = rule[9];
  q.fields_dirty = rule[10] != 0; q.int_pending = rule[11] != 0; q.integrates_in_one_launch = integrate_fits_one_launch(integrate_chunks(in[20]));
  q.grid_waves = waves;
  out[0] = two_in_flight_allowed(q) ? 1 : 0;
  out[1] = (int)std::min<long>(waves, 2147483647L);
  static_assert(CLIMA_TWO_IN_FLIGHT_RULE_N == 12, "the order documented in clima_radtran_hip.h");
}

// clima/fortran/Radtran.f90:109-118
void radtran_unset_custom_optical_properties(void *ptr) {
  Radtran *r = as_rad(ptr);
  if (r) r->cust_on = false;
}

void radtran_create_end(void *ptr, const int *num_zenith_angles, const double *surface_albedo, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (r->state != 1) { set_err(err, "radtran_create_end: create_begin has not been called"); return; }
  if (r->k.empty()) { set_err(err, "There are no k-distributions, yet there must be some to compute total opacity."); return; }
  if (r->ir.nw == 0 || r->sol.nw == 0) { set_err(err, "wavelength channels are not set"); return; }
  if (*num_zenith_angles < 1) { set_err(err, "number of zenith angles must be >= 1"); return; }
  TRY
  const int nz = r->nz, nw = r->nw;
  // zenith_angles_and_weights (clima_eqns.f90:26-41) then cos(deg*pi/180) (clima_radtran.f90:165)
  std::vector<double> x, w;
  gauss_legendre(*num_zenith_angles, x, w);
  r->zenith_u.resize(*num_zenith_angles);
  r->zenith_w.resize(*num_zenith_angles);
  for (int i = 0; i < *num_zenith_angles; i++) {
    double mu = x[i] / 2.0 + 1.0 / 2.0;
    double ang = std::acos(mu) * 180.0 / PI;
    r->zenith_w[i] = w[i] / 2.0;
    r->zenith_u[i] = std::cos(ang * PI / 180.0);
  }
  r->surface_albedo.assign(r->sol.nw, *surface_albedo);   // :182-183
  r->surface_emissivity.assign(r->ir.nw, 1.0);            // :185-186
  if (r->photons_sol.empty()) r->photons_sol.assign(r->sol.nw, 0.0);

  int dev_count = 0;
  HIPCHK(hipGetDeviceCount(&dev_count));
  if (dev_count < 1) throw HipFail{"no HIP device available: the Radtran hot path has no CPU fallback"};
  HIPCHK(hipGetDevice(&r->device));
  HIPCHK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  r->lane_stream[0] = r->stream;
  HIPCHK(hipDeviceGetAttribute(&r->cus, hipDeviceAttributeMultiprocessorCount, r->device));
  HIPCHK(hipEventCreateWithFlags(&r->ev_upload, hipEventDisableTiming));

  // ---- tables to HBM + interpolation slots
  r->slots.clear();
  auto add_slot = [&](const double *axis_dev, const std::vector<double> &axis, int source, bool flag) {
    SlotDev s;
    s.axis = axis_dev; s.n = (int)axis.size(); s.source = source;
    s.lo = *std::min_element(axis.begin(), axis.end());   // types_create.f90:1371-1375
    s.hi = *std::max_element(axis.begin(), axis.end());
    s.flag_clamp = flag ? 1 : 0;
    r->slots.push_back(s);
  };
  for (auto *k : r->k) {
    k->d_log10k.upload(k->log10k); k->d_log10P.upload(k->log10P); k->d_temp.upload(k->temp);
    add_slot(k->d_log10P.p, k->log10P, 0, false);
    add_slot(k->d_temp.p, k->temp, 1, false);
  }
  r->abs_entries.clear();
  for (auto *v : {&r->cia, &r->pxs})
    for (auto *xs : *v) {
      xs->d_data.upload(xs->data);
      AbsEntry e;
      e.data = xs->d_data.p; e.nT = xs->dim ? xs->nT : 0; e.slot = 0;
      e.kind = (v == &r->cia) ? ABS_CIA : ABS_COLUMN; e.a = xs->sp1; e.b = xs->sp2 < 0 ? 0 : xs->sp2;
      if (xs->dim) { xs->d_temp.upload(xs->temp); e.slot = (int)r->slots.size(); add_slot(xs->d_temp.p, xs->temp, 1, false); }
      r->abs_entries.push_back(e);
    }
  for (auto *xs : r->ray) xs->d_data.upload(xs->data);
  if (r->has_cont) {  // H2O self then foreign (types.f90:719-721)
    r->d_cont_temp.upload(r->cont_temp); r->d_cont_H2O.upload(r->cont_H2O); r->d_cont_foreign.upload(r->cont_foreign);
    const int slot = (int)r->slots.size();
    add_slot(r->d_cont_temp.p, r->cont_temp, 1, false);
    r->abs_entries.push_back(AbsEntry{r->d_cont_H2O.p, r->cont_nT, slot, ABS_H2O_SELF, r->LH2O, 0});
    r->abs_entries.push_back(AbsEntry{r->d_cont_foreign.p, r->cont_nT, slot, ABS_H2O_FOREIGN, r->LH2O, 0});
  }
  if ((int)r->abs_entries.size() > MAX_ABS - (ABS_BATCH - 2)) throw HipFail{"too many continuum terms for this build"};
  // the opacity tile takes the terms in batches of ABS_BATCH without per-term tests: the list is padded with
  // terms of weight 0 on a table of zeros (they add +0.0 at the end of the sum)
  if (r->abs_entries.size() % ABS_BATCH) {
    r->d_zero_xs.upload(std::vector<double>((size_t)r->nw + 1, 0.0));
    while (r->abs_entries.size() % ABS_BATCH) r->abs_entries.push_back(AbsEntry{r->d_zero_xs.p, 0, 0, ABS_ZERO, 0, 0});
  }
  r->part_slot.clear();
  for (auto *p : r->part) {
    p->d_radii.upload(p->radii); p->d_w0.upload(p->w0); p->d_qext.upload(p->qext); p->d_gt.upload(p->gt);
    r->part_slot.push_back((int)r->slots.size());
    add_slot(p->d_radii.p, p->radii, 2 + p->p_ind, true);
  }
  r->nslots = (int)r->slots.size();
  if (r->nslots + 1 > MAX_SLOTS) throw HipFail{"too many interpolated tables for this build"};  // one kept for custom opacity
  r->d_wbin.upload(r->wbin); r->d_wbin_e.upload(r->wbin_e); r->d_wxy.upload(r->wxy);
  {
    std::vector<double> pad = r->wbin_e;
    for (int i = 0; i < 4; i++) pad.push_back(INFINITY);
    r->d_wbin_e_pad.upload(pad);
    // the tables the assembly form of the mixing step keeps in scalar registers (8 g-points): E_1..E_8, w, 1/width --
    // the reciprocal formed as the opacity tile forms it (1.0 / (E_(k+1) - E_k))
    std::vector<double> tab(24, 0.0);
    if (r->ng == 8)
      for (int k = 0; k < 8; k++) {
        tab[k] = r->wbin_e[k + 1];
        tab[8 + k] = r->wbin[k];
        tab[16 + k] = 1.0 / (r->wbin_e[k + 1] - r->wbin_e[k]);
      }
    r->d_rorr_tab.upload(tab);
  }
  r->d_freq.upload(r->freq);
  r->ir.d_freq.upload(r->ir.freq); r->sol.d_freq.upload(r->sol.freq);
  // amean unit factors per solar bin (radiate.f90:174-178)
  std::vector<double> f1(r->sol.nw), f2(r->sol.nw), dw(r->sol.nw);
  for (int l = 0; l < r->sol.nw; l++) {
    double avg_freq = 0.5 * (r->sol.freq[l] + r->sol.freq[l + 1]);
    double avg_wavl = 1.0e9 * C_LIGHT / avg_freq;
    f1[l] = (avg_freq / avg_wavl);
    f2[l] = (avg_wavl / (PLANK * C_LIGHT * 1.0e16));
    dw[l] = (r->sol.wavl[l + 1] - r->sol.wavl[l]);
  }
  r->d_am_f1.upload(f1); r->d_am_f2.upload(f2); r->d_am_dw.upload(dw);

  // ---- column, prep, opr, results
  r->col_layout = column_layout(nz, r->nsp, r->np);
  r->d_col.alloc(r->col_layout.count);
  r->d_col.zero();
  HIPCHK(hipHostMalloc((void **)&r->h_col, sizeof(double) * r->col_layout.count, hipHostMallocMapped));
  std::memset(r->h_col, 0, sizeof(double) * r->col_layout.count);
  if (hipHostGetDevicePointer((void **)&r->h_col_dev, r->h_col, 0) != hipSuccess) { r->h_col_dev = nullptr; (void)hipGetLastError(); }
  r->prep_count = prep_block_count(r);
  r->d_prep.alloc(r->prep_count); r->d_prep.zero();
  r->d_done.alloc(((size_t)nw * nz + 255) / 256 + 1); r->d_done.zero();
#ifdef CLIMA_STAMPS
  r->d_stamps.alloc(64 + 2 * 8192); r->d_stamps.zero();
#endif
  r->opr_count = opr_views(r, nullptr).count;
  r->d_opr.alloc(r->opr_count); r->d_opr.zero();
  const OprViews o = opr_views(r, r->d_opr.p);
  r->d_tau.view(o.tau, o.w0 - o.tau); r->d_w0.view(o.w0, o.g - o.w0); r->d_g.view(o.g, o.tau_band - o.g);
  r->d_tau_band.view(o.tau_band, o.scat - o.tau_band); r->d_scat.view(o.scat, o.tau + o.count - o.scat);
  auto mk = [&](WrkObj &wk, int which, int nwc) {  // clima_radtran.f90:199-214
    wk.parent = r; wk.which = which;
    wk.fup_a.alloc((size_t)(nz + 1) * nwc); wk.fdn_a.alloc((size_t)(nz + 1) * nwc);
    wk.amean.alloc((size_t)(nz + 1) * nwc); wk.tau_band.alloc((size_t)nz * nwc);
    wk.fup_a.zero(); wk.fdn_a.zero(); wk.amean.zero(); wk.tau_band.zero();
  };
  mk(r->wrk_ir, 0, r->ir.nw);
  mk(r->wrk_sol, 1, r->sol.nw);
  const LevelRows &l = r->rows = level_rows(nz);
  r->d_small.alloc(l.count); r->d_small.zero();
  r->d_flux_n.view(r->d_small.p, l.flux_count);
  // two ints share the last double slot: [0] particle-radius clamp, [1] fused hand-off timeout
  r->d_err.view(reinterpret_cast<int *>(r->d_small.p + l.err_words), 2);
  r->d_partial.alloc((size_t)4 * integrate_chunks(std::max(r->ir.nw, r->sol.nw)) * (nz + 1)); r->d_partial.zero();
  HIPCHK(hipHostMalloc((void **)&r->h_small, sizeof(double) * l.count, hipHostMallocMapped));
  std::memset(r->h_small, 0, sizeof(double) * l.count);
  if (hipHostGetDevicePointer((void **)&r->h_small_dev, r->h_small, 0) != hipSuccess) { r->h_small_dev = nullptr; (void)hipGetLastError(); }
  r->h_errflag = reinterpret_cast<int *>(r->h_small + l.err_words);
  HIPCHK(hipDeviceSynchronize());
  r->fields_dirty = true;
  compute_shard(r);
  r->holds.rows_fetched();   // (zeros on both sides)
  r->state = 2;
  CATCH(err)
}

void radtran_upload_column(void *ptr, const double *T_surface, const double *T, const double *P,
                           const double *densities, const double *dz, const double *pdensities,
                           const double *radii, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (r->np > 0 && (!pdensities || !radii)) { set_err(err, "The model contains particles but \"pdensities\" and \"radii\" are not arguments."); return; }
  TRY
  do_upload(r, ColumnArrays{T_surface, T, P, densities, dz, pdensities, radii});
  CATCH(err)
}

void radtran_radiate_resident(void *ptr, const int *compute_solar, const int *compute_opacity, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (refuse(r, "radiate_resident", NEED_COLUMN, err)) return;
  TRY
  const bool cs = *compute_solar != 0, co = *compute_opacity != 0;
  // Two calls in flight (two_in_flight_allowed): where the handle pipelines two, a full call, when nobody has joined the
  // previous such call, runs beside it: in the other slot, on the other lane.  Every other call joins first
  // (enqueue_radiate) and stays where the handle is.  Either way the call keeps its integration back IN ITS SLOT -- where
  // its prep pass cleared nothing: DEFER_FOR_A_MERGE --, and the call that next takes the slot -- two calls on, on the
  // same lane -- launches it with its own prep pass as one grid (resolve_pending_integration inside the LaneScope): a
  // lane's chain is [integrate(i-2) | prep(i)] -> fused(i).  Only an integration kept back by a call that was not
  // pipelined keeps the next call from going beside (it joins and takes it along where it is).
  upload_fields(r);   // (stale fields: behind a join and a host wait, as the call itself would; then it decides)
  const bool beside = cs && co && two_in_flight(r, r->holds.unjoined, r->int_pending && !r->pending_pipelined);
  const bool two = beside || (cs && co && pipelining_two(r));
  if (beside) {
    ensure_other_slot(r);
    swap_slot(r);
    r->lane ^= 1;
    try {
      LaneScope lane(r, r->lane);
      enqueue_radiate(r, resident_bufs(r), cs, co, true, DEFER_FOR_A_MERGE);
      r->pending_pipelined = r->int_pending;
    } catch (...) {
      // the handle is again what it was: its buffers the previous call's slot (whatever reached the other lane is
      // joined like a call: LaneScope left its event behind it)
      swap_slot(r);
      r->lane ^= 1;
      r->holds.other_in_flight = true;
      throw;
    }
    r->holds.call_pipelined(true);
  } else {
    enqueue_radiate(r, resident_bufs(r), cs, co, true, two ? DEFER_FOR_A_MERGE : DEFER_ALWAYS);
    r->pending_pipelined = two && r->int_pending;
    if (two) r->holds.call_pipelined(false);
  }
  CATCH(err)
}

// Batched form of the RCE Jacobian's radiative calls (src/adiabat/clima_adiabat_solve.f90:798-812:
// one `radiate(..., compute_solar=.false., compute_opacity=.false.)` per perturbed temperature
// profile).  Column c gets what that call would leave in wrk_ir%fup_n, wrk_ir%fdn_n and f_total
// (clima_radtran.f90:262-289: IR with the resident opr, solar terms of the last solar call).
//
// The general form: n columns at d_T [n][nz], d_Ts [n] (device) -> three arrays [n][nz+1] at d_out, out_arr elements apart.
static void ir_batch_general(Radtran *r, const double *d_T, const double *d_Ts, int n, double *d_out, size_t out_arr) {
  const int nz = r->nz, nl = nz + 1, nw_ir = r->ir.nw;
  // columns per launch: bounds the per-column spectra held in HBM (2.5 GB at 512 layers: 288 GB make that a
  // non-issue) and sets how many columns share one evaluation of the temperature-independent part -- a block of
  // the shared-matrix kernel takes a quarter of them: at 64 per launch that part was a fifth of the kernel
  const int CH = std::min(n, 512);
  const int nchunk = integrate_chunks(r->ir_n);
  const size_t spec = (size_t)nw_ir * nl;
  r->d_bup.reserve(spec * CH); r->d_bdn.reserve(spec * CH); r->d_bpartial.reserve((size_t)CH * 2 * nchunk * nl);
  const CallBufs b = resident_bufs(r);
  TwoStreamParams ts = make_twostream_params(r, b, column_dev(r, b), false);
  ts.ir_fup_a = r->d_bup.p; ts.ir_fdn_a = r->d_bdn.p;
  ts.b_T = nz; ts.b_Ts = 1; ts.b_out = spec;
  PlanIn in = plan_input(r, b, false, false, false);
  in.ir_batch = true;
  const LaunchPlan plan = plan_radiate(in);
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int nc = std::min(CH, n - c0);
    TwoStreamParams tb = ts;
    tb.T = d_T + (size_t)c0 * nz; tb.T_surface = d_Ts + c0; tb.b_ncol = nc;
    // shared-matrix batch kernel (up to 512 layers); otherwise one full solve per column
    // (one or two columns of more than 256 layers -- the response form's base profile and a dense column -- take the
    // single call's kernel: the 5-8 slot forms of the shared-matrix kernel run one wave per SIMD and amortise their
    // temperature-independent part over the columns of a block; measured at 402 layers, one column: 26 us less.  At
    // 202 layers the shared-matrix kernel is the faster one even alone: 20 us.)
    const bool tiny = nc <= r->batch_shared_min && nz > 256;
    const bool shared_ok = r->batch_shared && !tiny && launch_twostream_ir_batch(tb, nc, r->stream);
    HIPCHK(hipGetLastError());
    if (!shared_ok) {
      if (plan.caller_clears) {  // g-point groups add into zeroed spectra
        HIPCHK(hipMemsetAsync(r->d_bup.p, 0, sizeof(double) * spec * nc, r->stream));
        HIPCHK(hipMemsetAsync(r->d_bdn.p, 0, sizeof(double) * spec * nc, r->stream));
      }
      const bool ok = launch_twostream_w(tb, plan.ts, r->stream);
      HIPCHK(hipGetLastError());
      if (!ok)
        throw HipFail{"radiate_ir_batch: nz = " + std::to_string(nz) + " exceeds what the wave two-stream kernel holds (512)"};
    }
    BatchIntegrateParams bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.nz = nz; bp.ir_lo = r->ir_lo; bp.ir_n = r->ir_n; bp.nchunk = nchunk; bp.col0 = c0;
    bp.fup_a = r->d_bup.p; bp.fdn_a = r->d_bdn.p; bp.spec_stride = spec;
    bp.freq = r->ir.d_freq.p; bp.partial = r->d_bpartial.p; bp.flux_n = r->d_flux_n.p; bp.out = d_out; bp.out_arr = out_arr;
    launch_integrate_batch(bp, nc, r->stream);
    HIPCHK(hipGetLastError());
  }
}

// The response form (ir_green.inc).  The Jacobian's columns are one base profile with one (on the doubled radiative
// grid: a few) temperatures changed each; with the opacities fixed the IR solve is linear in the Planck values, so
// such a column is F(base) + unit responses x Planck differences.  The plan below finds the base (per level the
// temperature two of three sample columns share) and every column's deviations from it; a column with more than
// green_max_dev(nz) of them (the surface-temperature column of a convective profile moves every layer) goes through the
// general kernel together with the base profile itself.
// (8 in round 3.  With the accumulation on the matrix cores a deviation costs ~0.5 us at 402 layers where a column of the
// general kernel costs 17: the bound grows with the height of the grid, nz / 16 between 8 and 32.)
static int green_max_dev(int nz) { return std::min(32, std::max(8, nz / 16)); }
struct GreenPlan {
  std::vector<double> base;              // [nz] ground-first, then the surface temperature
  std::vector<int> dense;                // columns for the general kernel
  std::vector<int> col_src, col_ptr, col_dev, dev_k;
  std::vector<double> dev_T;
  int n_sparse = 0;
};
static void green_plan(const double *T, const double *Ts, int n, int nz, GreenPlan &pl) {
  // the base: per level what two of three sample columns agree on (a Jacobian's batch changes a level in one column
  // only, so any two columns agree nearly everywhere); a poor guess costs speed, never correctness -- columns far from
  // it go through the general kernel
  pl.base.assign(nz + 1, 0.0);
  {
    const int c0 = 0, c1 = n / 2, c2 = n - 1;
    for (int j = 0; j <= nz; j++) {
      const double a = j < nz ? T[(size_t)c0 * nz + j] : Ts[c0], b = j < nz ? T[(size_t)c1 * nz + j] : Ts[c1],
                   c = j < nz ? T[(size_t)c2 * nz + j] : Ts[c2];
      pl.base[j] = (b == c) ? b : a;
    }
  }
  pl.col_src.assign(n, -1);
  const int max_dev = green_max_dev(nz);
  std::vector<int> dk, dc; std::vector<double> dT;
  const double *base = pl.base.data();
  for (int c = 0; c < n; c++) {
    const double *Tc = T + (size_t)c * nz;
    int cnt = Ts[c] != base[nz] ? 1 : 0;
    for (int j = 0; j < nz; j++) cnt += Tc[j] != base[j] ? 1 : 0;      // (no early exit: this loop vectorises)
    if (cnt > max_dev) { pl.col_src[c] = 1 + (int)pl.dense.size(); pl.dense.push_back(c); continue; }
    pl.n_sparse++;
    if (cnt == 0) continue;
    for (int j = 0; j <= nz; j++) {
      const double v = j < nz ? Tc[j] : Ts[c];
      if (v != base[j]) { dk.push_back(j < nz ? nz - 1 - j : nz); dc.push_back(c); dT.push_back(v); }   // (radiate.f90:65-69: level k is layer nz-1-k)
    }
  }
  std::vector<int> order(dk.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return dk[a] < dk[b]; });
  pl.dev_k.resize(order.size()); pl.dev_T.resize(order.size());
  std::vector<int> cnt(n + 1, 0);
  for (size_t s2 = 0; s2 < order.size(); s2++) { pl.dev_k[s2] = dk[order[s2]]; pl.dev_T[s2] = dT[order[s2]]; cnt[dc[order[s2]] + 1]++; }
  pl.col_ptr.assign(n + 1, 0);
  for (int c = 0; c < n; c++) pl.col_ptr[c + 1] = pl.col_ptr[c] + cnt[c + 1];
  pl.col_dev.resize(order.size());
  std::vector<int> fill(pl.col_ptr.begin(), pl.col_ptr.end() - 1);
  for (size_t s2 = 0; s2 < order.size(); s2++) pl.col_dev[fill[dc[order[s2]]]++] = (int)s2;
}

// What every kernel of the IR derivative family reads of the handle: the dimensions, the stored opacities, the frequency
// grids, the emissivity, has_hard_surface and ir_tau_min; everything else of the block is zero, for the caller to fill
static GreenParams green_params(const Radtran *r) {
  GreenParams g;
  std::memset(&g, 0, sizeof(g));
  g.nz = r->nz; g.ng = r->ng; g.n_ir = r->ir_n; g.ir_lo = r->ir_lo; g.ir_start = r->ir.ind_start; g.NQ = r->ir_n * r->ng;
  g.tau = r->d_tau.p; g.w0 = r->d_w0.p; g.g = r->d_g.p; g.wbin = r->d_wbin.p;
  g.freq = r->d_freq.p; g.ir_freq = r->ir.d_freq.p; g.emissivity = r->d_emis.p;
  g.has_hard_surface = r->has_hard_surface ? 1 : 0; g.ir_tau_min = r->ir_tau_min;
  return g;
}

// The part of the response form that sees the opacities alone (k_green_factor, k_green_unit, k_green_local: ~345 of the
// ~700 us of GPU work of a 402-layer Jacobian batch): its arrays and launches.  radtran_radiate_ir_batch issues it BEFORE
// the host looks at the columns when the handle's last batch of this size took the response form -- the plan (~100 us of
// host time at 403 columns) then runs beside it instead of in front of it.
// (Measured and not kept: a second queue for the kernels that do not depend on each other -- k_green_local beside
// k_green_unit, the base profile's general kernel beside k_green_factor, the mixed blocks' sums beside the far-form
// ones.  rocprofv3's kernel trace shows them side by side and each that much slower: the far-form kernel holds 2 x 232
// registers per SIMD, the general kernel one wave of 512, and the batch took 828-840 us either way.)
static void green_factor_part(Radtran *r, GreenParams &g) {
  g = green_params(r);
  const int nz = r->nz, NQ = g.NQ;
  r->d_green.reserve(green_work_views(nz, NQ, nullptr).count);
  const GreenWork w = green_work_views(nz, NQ, r->d_green.p);
  g.RW = w.RW; g.IS = w.IS; g.FS = w.FS; g.DS = w.DS; g.D0 = w.D0;
  launch_green_factor(g, r->stream);
  HIPCHK(hipGetLastError());
}

// What the response form's two callers (ir_batch_green, radtran_ir_jacobian) share.
// The level blocks around a deviation's own levels (green_block_class == 2), deviations sorted by k: the pairs of
// k_green_accum_mixed
static void green_mixed_list(const std::vector<int> &dev_k, int nz, std::vector<int> &mdev, std::vector<int> &mblk) {
  const int nl = nz + 1;
  for (int d = 0; d < (int)dev_k.size(); d++)
    for (int blk = std::max(0, (dev_k[d] - 1) / GREEN_LB - 1); blk < (nl + GREEN_LB - 1) / GREEN_LB; blk++) {
      const int cls = green_block_class(dev_k[d], blk, nz);
      if (cls == 2) { mdev.push_back(d); mblk.push_back(blk); }
      if (cls == 1) break;
    }
}
// bin splits of the two accumulation kernels for ndev deviations (the mixed blocks' from a lower bound of their
// number when nmix < 0: one per deviation)
static void green_splits(const Radtran *r, int ndev, int nmix, int &qsplit, int &msplit) {
  const int nl = r->nz + 1, n_ir = r->ir_n;
  // bin splits: the accumulation's waves should fill the machine ONCE (green_far_resident_waves): a few waves more
  // than that and the kernel takes two rounds
  qsplit = green_far_splits(n_ir, green_far_waves(ndev, nl));
  // the mixed blocks: few pairs, finer splits
  msplit = std::max(qsplit, std::min(n_ir, 4096 / std::max(((nmix < 0 ? ndev : nmix) + 3) / 4, 1)));
}
// bytes of the response form's work arrays for ndev deviations (~150 KB per (bin, g-point) at 500 layers, and the
// partial sums of the two accumulation kernels: their bin splits x deviations x 2 x levels)
static double green_work_bytes(const Radtran *r, int ndev) {
  const int nz = r->nz, nl = nz + 1;
  int qs, ms;
  green_splits(r, ndev, -1, qs, ms);
  return ((double)r->ir_n * r->ng * (13.0 * nl + 14.0 * nz + 4.3 * nl) + (double)(qs + ms) * ((double)ndev + 64.0) * 2.0 * nl) * 8.0;
}
// the handle's pinned staging block, at least `bytes` long (half as much again when it has to grow)
static char *green_stage(Radtran *r, size_t bytes) { return r->h_green.reserve(bytes, bytes / 2); }
// the accumulation's arrays (Planck factors, the partial sums of both kernels) and split counts; the deviation and
// mixed-pair lists are the caller's
static void green_accum_arrays(Radtran *r, GreenParams &g, int ndev, int nmix) {
  const int nl = r->nz + 1, n_ir = r->ir_n, ndev_pad = green_ndev_pad(ndev);
  int qsplit, msplit;
  green_splits(r, ndev, nmix, qsplit, msplit);
  const size_t need = (size_t)n_ir * ndev_pad + 64 + (size_t)(qsplit + msplit) * ndev_pad * 2 * nl;
  r->d_green_acc.reserve(need);
  double *w = r->d_green_acc.p;
  auto take = [&](size_t cnt) { double *p0 = w; w += cnt; return p0; };
  g.DB = take((size_t)n_ir * ndev_pad + 64); g.partial = take((size_t)qsplit * ndev_pad * 2 * nl);
  g.msplit = msplit; g.partial_m = take((size_t)msplit * ndev_pad * 2 * nl);
  g.ndev = ndev; g.ndev_pad = ndev_pad; g.qsplit = qsplit; g.nmix = nmix;
}

// `pre`: the opacity-only part has been issued already (green_factor_part's parameter block)
static void ir_batch_green(Radtran *r, const GreenPlan &pl, const double *T, const double *Ts, int n, double *d_out, const GreenParams *pre) {
  const int nz = r->nz, nl = nz + 1;
  // 1. the base profile and the dense columns through the general kernel
  const int ngen = 1 + (int)pl.dense.size();
  const int ndev = (int)pl.dev_k.size(), ndev_pad = green_ndev_pad(ndev);
  std::vector<int> mdev, mblk;
  green_mixed_list(pl.dev_k, nz, mdev, mblk);
  const int nmix = (int)mdev.size();
  // everything the host hands over goes through ONE pinned block (no pageable copies, no synchronise before the
  // kernels): doubles T [ngen][nz] | Ts [ngen] | dev_T [ndev_pad] | base_T by level k [nl], then ints
  // dev_k [ndev_pad] | col_src [n] | col_ptr [n+1] | col_dev [ndev] | mix_dev [nmix] | mix_blk [nmix]
  const size_t nd = (size_t)ngen * nz + ngen + ndev_pad + nl, ni = (size_t)ndev_pad + n + (n + 1) + ndev + 2 * (size_t)nmix;
  double *hd = reinterpret_cast<double *>(green_stage(r, sizeof(double) * nd + sizeof(int) * ni));
  int *hi = reinterpret_cast<int *>(hd + nd);
  {
    double *hT = hd, *hTs = hd + (size_t)ngen * nz, *hdev = hTs + ngen, *hbase = hdev + ndev_pad;
    std::memcpy(hT, pl.base.data(), sizeof(double) * nz);
    hTs[0] = pl.base[nz];
    for (int i = 1; i < ngen; i++) {
      std::memcpy(hT + (size_t)i * nz, T + (size_t)pl.dense[i - 1] * nz, sizeof(double) * nz);
      hTs[i] = Ts[pl.dense[i - 1]];
    }
    for (int d = 0; d < ndev_pad; d++) hdev[d] = d < ndev ? pl.dev_T[d] : 0.0;
    for (int k = 0; k < nz; k++) hbase[k] = pl.base[nz - 1 - k];
    hbase[nz] = pl.base[nz];
    int *w2 = hi;
    for (int d = 0; d < ndev_pad; d++) *w2++ = d < ndev ? pl.dev_k[d] : 0;
    w2 = std::copy(pl.col_src.begin(), pl.col_src.end(), w2);
    w2 = std::copy(pl.col_ptr.begin(), pl.col_ptr.end(), w2);
    w2 = std::copy(pl.col_dev.begin(), pl.col_dev.end(), w2);
    w2 = std::copy(mdev.begin(), mdev.end(), w2);
    w2 = std::copy(mblk.begin(), mblk.end(), w2);
  }
  r->d_green_in.reserve(nd); r->d_gen_out.reserve((size_t)ngen * 3 * nl);
  r->d_green_idx.reserve(ni);
  HIPCHK(hipMemcpyAsync(r->d_green_in.p, hd, sizeof(double) * nd, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipMemcpyAsync(r->d_green_idx.p, hi, sizeof(int) * ni, hipMemcpyHostToDevice, r->stream));
  const double *d_T = r->d_green_in.p, *d_Ts = d_T + (size_t)ngen * nz;
  ir_batch_general(r, d_T, d_Ts, ngen, r->d_gen_out.p, (size_t)ngen * nl);
  // 3. the opacity-only part (unless it is under way already) and the accumulation's arrays
  GreenParams g;
  if (pre) g = *pre;
  else green_factor_part(r, g);
  green_accum_arrays(r, g, ndev, nmix);
  g.dev_k = r->d_green_idx.p; g.col_src = g.dev_k + ndev_pad; g.col_ptr = g.col_src + n; g.col_dev = g.col_ptr + n + 1;
  g.mix_dev = g.col_dev + ndev; g.mix_blk = g.mix_dev + nmix;
  g.dev_T = d_Ts + ngen; g.base_T = g.dev_T + ndev_pad;
  g.gen_out = r->d_gen_out.p; g.gen_arr = (size_t)ngen * nl; g.flux_n = r->d_flux_n.p; g.out = d_out; g.out_arr = (size_t)n * nl;
  launch_green_columns(g, n, r->stream);
  HIPCHK(hipGetLastError());
  r->ir_green_batches++;
}

// `narr` result arrays of `arr` doubles each, back to back in device memory from d_src on, into the caller's
// outs[0..narr-1] through the handle's pinned block in `npiece` pieces, the host copying piece i out while piece i + 1 is
// still on the link (one copy and then one memcpy of the whole took 95 + 140 us of a 0.93 ms batch call at 403 columns x
// 403 levels).  Returns when all are there.
constexpr int TO_HOST_PIECES = 6;     // (Radtran::bout_ev holds as many events)
static void to_host_in_pieces(Radtran *r, const double *d_src, double *const *outs, size_t arr, int narr, int npiece) {
  double *const h_bout = r->h_bout.reserve(narr * arr);
  const size_t total = narr * arr, piece = (total + npiece - 1) / npiece;
  for (auto &e : r->bout_ev)
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (int k = 0; k < npiece; k++) {
    const size_t lo = std::min(total, (size_t)k * piece), hi = std::min(total, lo + piece);
    if (hi > lo) HIPCHK(hipMemcpyAsync(h_bout + lo, d_src + lo, sizeof(double) * (hi - lo), hipMemcpyDeviceToHost, r->stream));
    HIPCHK(hipEventRecord(r->bout_ev[k], r->stream));
  }
  for (int k = 0; k < npiece; k++) {
    const size_t lo = std::min(total, (size_t)k * piece), hi = std::min(total, lo + piece);
    HIPCHK(hipEventSynchronize(r->bout_ev[k]));
    for (size_t x = lo; x < hi;) {      // (a piece may straddle two of the arrays)
      const size_t i = x / arr, n_here = std::min(hi, (i + 1) * arr) - x;
      std::memcpy(outs[i] + (x - i * arr), h_bout + x, sizeof(double) * n_here);
      x += n_here;
    }
  }
}
// ... from d_bout's first-th array on (the batch and the full Jacobian: three arrays from the start;
// radtran_ir_jacobian_reduced's total alone: one)
static void bout_to_host(Radtran *r, double *const *outs, size_t arr, int narr = 3, int first = 0) {
  to_host_in_pieces(r, r->d_bout.p + (size_t)first * arr, outs, arr, narr, TO_HOST_PIECES);
}
// ... one array of `count` doubles, whole below 32768 of them
static void rows_to_host(Radtran *r, const double *d_src, double *dst, size_t count) {
  if (count) to_host_in_pieces(r, d_src, &dst, count, 1, count < 32768 ? 1 : TO_HOST_PIECES);
}

static void register_host(Radtran *r, void *p, size_t bytes);
static bool host_is_registered(const Radtran *r, const void *p, size_t bytes);
void radtran_radiate_ir_batch(void *ptr, const int *ncol, const double *T_surface, const int *dim1_T,
                              const int *dim2_T, const double *T, double *fup_n, double *fdn_n,
                              double *f_total, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*dim1_T != r->nz || *dim2_T != *ncol || *ncol < 1) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (refuse(r, "radiate_ir_batch", NEED_OPACITIES | NEED_SPECTRUM, err)) return;
  TRY
  // CLIMA_HIP_BATCH_TIMES=1: the call's host-side phases on stderr (a diagnostic: tools/gpu_ir_batch.py)
  static const bool times = [] { const char *e = getenv("CLIMA_HIP_BATCH_TIMES"); return e && e[0] == '1'; }();
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count(); };
  ready_stored_opacities(r);
  const int nz = r->nz, nl = nz + 1, n = *ncol;
  r->d_bout.reserve((size_t)n * 3 * nl);
  bool green = false;
  if (r->ir_green_mode != 0 && r->batch_shared && nz >= 4 && nz <= 512 && r->ir_n > 0) {   // (CLIMA_HIP_BATCH_SHARED=0: one full solve per column, bit for bit the single call)
    // k_green_unit / k_green_local take one (bin, g-point) pair per blockIdx.y: a grid dimension of at most 65535
    const bool fits = (long)r->ir_n * r->ng <= 65535;
    GreenParams gpre;
    bool pre = false;
    if (fits && r->green_last_n == n) { green_factor_part(r, gpre); pre = true; }
    GreenPlan pl;
    green_plan(T, T_surface, n, nz, pl);
    // worth it from a few dozen sparse columns of a tall grid on (measured: 203 columns x 202 layers 0.60 against 1.29 ms,
    // 103 x 102: 0.54 against 0.46 -- the general kernel's 1-2 slot forms are cheap and the opacity-only pass is not free)
    if (r->ir_green_mode == 2) green = pl.n_sparse > 0;
    // (ir_tau_min far below the reference's 1e-6: layers of tau ~ 1e-8 keep the source slope dB / tau, and a single changed
    // level is the worst case for it -- the response form stays correct but loses digits faster than the general kernel
    // there, 1e-8 against 5e-10 of the row's maximum in the fuzz sweep: left to mode 2)
    else if (pl.n_sparse >= 48 && r->ir_tau_min >= 1.0e-7) {
      // cost model (ms on an MI355X, from profiles/r03_ir_batch.txt and the rocprofv3 runs behind DESIGN section 4; both
      // sides scale with the number of (bin, g-point) pairs): the general kernel per column against the opacity-only
      // pass + the accumulation over deviations x levels + the extra launches
      const double scale = (double)r->ir_n * r->ng / 4800.0;
      const double t_general = pl.n_sparse * (nz <= 256 ? 0.032e-3 : 0.044e-3) * nz * scale;
      const double t_green = 0.05 + scale * (0.35 * nz / 402.0 + 0.28 * (double)pl.dev_k.size() * nl / 162409.0);   // (round 4: the accumulation on the matrix cores)
      green = t_green < 0.8 * t_general;
    }
    // not with a base that is not a number anywhere (every column would "deviate" there and inherit it), nor when the
    // work arrays (~150 KB per (bin, g-point) at 500 layers) would take more than 16 GB
    for (double v : pl.base) if (!std::isfinite(v)) green = false;
    if (green_work_bytes(r, (int)pl.dev_k.size()) > 16.0e9) green = false;
    if (!fits) green = false;
    if (green) ir_batch_green(r, pl, T, T_surface, n, r->d_bout.p, pre ? &gpre : nullptr);
    r->green_last_n = green ? n : -1;
  }
  if (!green) {
    r->d_bT.reserve((size_t)n * nz); r->d_bTs.reserve(n);
    HIPCHK(hipMemcpyAsync(r->d_bT.p, T, sizeof(double) * (size_t)n * nz, hipMemcpyHostToDevice, r->stream));
    HIPCHK(hipMemcpyAsync(r->d_bTs.p, T_surface, sizeof(double) * n, hipMemcpyHostToDevice, r->stream));
    ir_batch_general(r, r->d_bT.p, r->d_bTs.p, n, r->d_bout.p, (size_t)n * nl);
  }
  const size_t arr = (size_t)n * nl;
  // (src/radtran/clima_radtran_radiate.f90:184-192 summed over the bins of all ranks; f_total from the reduced rows)
  comm_reduce_up_down(r, arr, [&] { launch_batch_ftotal(r->d_bout.p, arr, n, nz, r->d_flux_n.p, r->stream); });
  const double t_enq = times ? since() : 0.0;
  if (times) HIPCHK(hipStreamSynchronize(r->stream));
  const double t_kern = times ? since() : 0.0;
  // The three result arrays (3.9 MB at 403 columns x 403 levels).  Default: through the handle's pinned block in pieces,
  // the host copying piece i into the caller's arrays while piece i + 1 is still on the link (one copy and then one
  // memcpy of the whole took 95 + 140 us of a 0.93 ms call).  radtran_batch_pin_results_set(1): the caller's arrays are
  // page-locked when it passes the same three as in its previous batch (the Jacobian's work arrays: the RCE solver fills
  // one set per iteration, src/adiabat/clima_adiabat_solve.f90:768-822) and the device fills them directly -- opt-in,
  // because the arrays must then stay allocated until radtran_spectra_release or the handle's end.
  double *outs[3] = {fup_n, fdn_n, f_total};
  bool direct = false;
  if (r->batch_pin_results) {
    const bool same = r->batch_out_n == arr && r->batch_out[0] == fup_n && r->batch_out[1] == fdn_n && r->batch_out[2] == f_total;
    r->batch_out[0] = fup_n; r->batch_out[1] = fdn_n; r->batch_out[2] = f_total; r->batch_out_n = arr;
    direct = same;
    if (same)
      for (double *o : outs) { register_host(r, o, sizeof(double) * arr); direct = direct && host_is_registered(r, o, sizeof(double) * arr); }
  }
  double t_d2h = 0.0;
  if (direct) {
    // (one queue: the three arrays over three copy queues behind an event took 86 instead of 95 us at 403 x 403 and
    // 50-150 us MORE at 201 x 201 -- the extra queues' start-up)
    for (int i = 0; i < 3; i++)
      HIPCHK(hipMemcpyAsync(outs[i], r->d_bout.p + (size_t)i * arr, sizeof(double) * arr, hipMemcpyDeviceToHost, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    t_d2h = times ? since() : 0.0;
  } else {
    bout_to_host(r, outs, arr);
    t_d2h = times ? since() : 0.0;
  }
  if (times)
    fprintf(stderr, "radiate_ir_batch: %d columns%s: plan + enqueue %.0f us, kernels done at %.0f, results with the caller at %.0f%s\n",
            n, green ? " (response form)" : "", t_enq, t_kern, t_d2h, direct ? " (its arrays page-locked)" : " (through the pinned block, six pieces)");
  CATCH(err)
}

// Batched form of solar calls that differ in how the star lights ONE atmosphere: case c is `radiate(...,
// compute_solar=.true., compute_opacity=.false.)` (clima_radtran.f90:291-316) on the stored optical properties after
// zenith_u, zenith_weights, surface_albedo and photon_scale_factor had been set to the case's.  include/clima_radtran_hip.h
// has the contract.  Two forms: k_twostream_sol_batch (solar_batch.inc: what the opacities alone decide once per (bin,
// g-point) and block), or one full solve per case by the stand-alone two-stream kernels.
static bool solar_batch_refused(Radtran *r, int n, int nzen, const double *zenith_u, const double *zenith_weights, const double *fup_n,
                                const double *fdn_n, const double *f_total, int nsel, const int *spec_level, const double *const *spec,
                                char *err) {
  const std::string pre = "radiate_solar_batch: ";
  if (refuse(r, "radiate_solar_batch", NEED_OPACITIES, err)) return true;
  if (r->shard_world != 1 || r->comm) {
    const std::string shard = r->shard_world != 1 ? "a bin shard of " + std::to_string(r->shard_world) : "";
    set_err(err, pre + "needs the whole spectrum (" + shard + (r->comm ? (shard.empty() ? "a communicator" : ", a communicator") : "") + ")");
    return true;
  }
  if (n < 1) { set_err(err, pre + "ncol must be at least 1 (ncol = " + std::to_string(n) + ")"); return true; }
  if (nzen < 1 || nzen > MAX_ZEN) { set_err(err, pre + "nzen must lie in 1.." + std::to_string(MAX_ZEN) + " (nzen = " + std::to_string(nzen) + ")"); return true; }
  if (!zenith_u) { set_err(err, pre + "\"zenith_u\" is a required argument"); return true; }
  if (!zenith_weights) { set_err(err, pre + "\"zenith_weights\" is a required argument"); return true; }
  if (!fup_n) { set_err(err, pre + "\"fup_n\" is a required argument"); return true; }
  if (!fdn_n) { set_err(err, pre + "\"fdn_n\" is a required argument"); return true; }
  // (what Holds records: no call has left level rows, or a graph replay dropped them)
  if (f_total && !r->holds.rows) { set_err(err, pre + "\"f_total\" was asked for, but the handle holds no level rows"); return true; }
  if (nsel < 0) { set_err(err, pre + "nsel must not be negative (nsel = " + std::to_string(nsel) + ")"); return true; }
  if (nsel > 0) {
    const int nl = r->nz + 1;
    if (!spec_level) { set_err(err, pre + "\"spec_level\" is a required argument"); return true; }
    for (int a = 0; a < nsel; a++) {
      const int v = spec_level[a];
      if (v < 1 || v > nl) {
        set_err(err, pre + "spec_level(" + std::to_string(a + 1) + ") = " + std::to_string(v) + " is outside 1.." + std::to_string(nl));
        return true;
      }
    }
    if (!spec[0] && !spec[1] && !spec[2]) { set_err(err, pre + "nsel = " + std::to_string(nsel) + ", but none of sol_fup, sol_fdn, sol_amean was given"); return true; }
  }
  return false;
}

void radtran_radiate_solar_batch(void *ptr, const int *ncol, const int *nzen_, const double *zenith_u, const double *zenith_weights,
                                 const double *surface_albedo, const double *photon_scale_factor, double *fup_n, double *fdn_n,
                                 double *f_total, const int *nsel_, const int *spec_level, double *sol_fup, double *sol_fdn,
                                 double *sol_amean, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int n = *ncol, nzen = *nzen_, nsel = *nsel_;
  double *spec_out[3] = {sol_fup, sol_fdn, sol_amean};
  if (solar_batch_refused(r, n, nzen, zenith_u, zenith_weights, fup_n, fdn_n, f_total, nsel, spec_level, spec_out, err)) return;
  TRY
  ready_stored_opacities(r);
  const int nz = r->nz, nl = nz + 1, nw_sol = r->sol.nw;
  const size_t spec = (size_t)nw_sol * nl, arr = (size_t)n * nl;
  // the cases' inputs in one block: [zen (u0 | weight | 1/u0)[nzen]] per case, then the albedos and scale factors
  const size_t o_alb = (size_t)n * 3 * nzen, o_scale = o_alb + (surface_albedo ? (size_t)n * nw_sol : 0), n_in = o_scale + n;
  std::vector<double> h_in(n_in);
  for (int c = 0; c < n; c++)
    for (int z = 0; z < nzen; z++) {
      const double u0 = zenith_u[(size_t)c * nzen + z];
      double *q = h_in.data() + (size_t)c * 3 * nzen;
      q[z] = u0; q[nzen + z] = zenith_weights[(size_t)c * nzen + z]; q[2 * nzen + z] = 1.0 / u0;
    }
  if (surface_albedo) std::memcpy(h_in.data() + o_alb, surface_albedo, sizeof(double) * (size_t)n * nw_sol);
  for (int c = 0; c < n; c++) h_in[o_scale + c] = photon_scale_factor ? photon_scale_factor[c] : r->photon_scale_factor;
  r->d_sb_in.reserve(n_in);
  HIPCHK(hipMemcpyAsync(r->d_sb_in.p, h_in.data(), sizeof(double) * n_in, hipMemcpyHostToDevice, r->stream));
  const double *d_alb = surface_albedo ? r->d_sb_in.p + o_alb : r->d_albedo.p;
  const size_t alb_stride = surface_albedo ? (size_t)nw_sol : 0;
  // cases per launch: bounds the three per-case spectra held in device memory (ir_batch_general's CH)
  const int CH = std::min(n, 512);
  const int nchunk = integrate_chunks(r->sol_n);
  r->d_sb_spec.reserve(3 * spec * CH); r->d_bpartial.reserve((size_t)CH * 2 * nchunk * nl); r->d_bout.reserve(3 * arr);
  double *d_fup = r->d_sb_spec.p, *d_fdn = d_fup + spec * CH, *d_am = d_fdn + spec * CH;
  std::vector<int> lv0(nsel);
  size_t spec_off[3], spec_total = 0;
  if (nsel > 0) {
    for (int a = 0; a < nsel; a++) lv0[a] = spec_level[a] - 1;
    r->d_spec_level.reserve(nsel);
    HIPCHK(hipMemcpyAsync(r->d_spec_level.p, lv0.data(), sizeof(int) * nsel, hipMemcpyHostToDevice, r->stream));
    for (int k = 0; k < 3; k++) { spec_off[k] = spec_total; if (spec_out[k]) spec_total += (size_t)nw_sol * nsel * n; }
    r->d_spec_stage.reserve(spec_total);
  }
  const CallBufs b = resident_bufs(r);
  bool shared_ran = false;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int nc = std::min(CH, n - c0);
    bool shared_ok = false;
    if (r->solar_batch_shared && r->sol_n > 0) {
      SolBatchParams sp;
      std::memset(&sp, 0, sizeof(sp));
      sp.nz = nz; sp.ng = r->ng; sp.n_sol = r->sol_n; sp.sol_lo = r->sol_lo; sp.sol_start = r->sol.ind_start;
      sp.ncase = nc; sp.nzen = nzen;
      sp.tau = b.opr.tau; sp.w0 = b.opr.w0; sp.g = b.opr.g; sp.wbin = r->d_wbin.p;
      sp.zen = r->d_sb_in.p + (size_t)c0 * 3 * nzen; sp.albedo = d_alb + (size_t)c0 * alb_stride; sp.alb_stride = alb_stride;
      sp.scale = r->d_sb_in.p + o_scale + c0;
      sp.photons_sol = r->d_photons.p; sp.am_f1 = r->d_am_f1.p; sp.am_f2 = r->d_am_f2.p; sp.am_dw = r->d_am_dw.p;
      sp.diurnal_fac = r->diurnal_fac;
      sp.fup = d_fup; sp.fdn = d_fdn; sp.amean = d_am; sp.out_stride = spec;
      shared_ok = launch_twostream_sol_batch(sp, r->stream);
      HIPCHK(hipGetLastError());
    }
    if (shared_ok) shared_ran = true;
    else {
      // one full solve per case: the stand-alone kernels of the single call with the case's angles, albedo and scale
      // in the handle's place (the copy of the band optical depth they write goes to a buffer nobody reads)
      r->d_sb_band.reserve((size_t)nw_sol * nz);
      TwoStreamParams ts = make_twostream_params(r, b, column_dev(r, b), true);
      ts.n_ir = 0; ts.nzen = nzen; ts.sol_tau_band = r->d_sb_band.p;
      PlanIn in = plan_input(r, b, true, false, false);
      in.n_ir = 0; in.nzen = nzen;
      const LaunchPlan plan = plan_radiate(in);
      for (int ci = 0; ci < nc; ci++) {
        const int c = c0 + ci;
        TwoStreamParams tc = ts;
        const double *q = r->d_sb_in.p + (size_t)c * 3 * nzen, *hq = h_in.data() + (size_t)c * 3 * nzen;
        tc.zen_u = q; tc.zen_w = q + nzen; tc.zen_iu = q + 2 * nzen;
        for (int z = 0; z < nzen; z++) { tc.zen_u_v[z] = hq[z]; tc.zen_w_v[z] = hq[nzen + z]; tc.zen_iu_v[z] = hq[2 * nzen + z]; }
        tc.albedo = d_alb + (size_t)c * alb_stride;
        tc.photon_scale_factor = h_in[o_scale + c];
        tc.sol_fup_a = d_fup + spec * ci; tc.sol_fdn_a = d_fdn + spec * ci; tc.sol_amean = d_am + spec * ci;
        if (plan.ts.zero_launch || plan.ts.groups > 1) {   // g-point groups add into cleared spectra
          HIPCHK(hipMemsetAsync(tc.sol_fup_a, 0, sizeof(double) * spec, r->stream));
          HIPCHK(hipMemsetAsync(tc.sol_fdn_a, 0, sizeof(double) * spec, r->stream));
          HIPCHK(hipMemsetAsync(tc.sol_amean, 0, sizeof(double) * spec, r->stream));
        }
        TsPlan wp = plan.ts;
        wp.zero_launch = false;
        bool ok = launch_twostream_w(tc, wp, r->stream);
        if (!ok) { HIPCHK(hipGetLastError()); ok = launch_twostream(tc, plan.block, r->stream); }
        HIPCHK(hipGetLastError());
        if (!ok) throw HipFail{"radiate_solar_batch: nz*ngauss = " + std::to_string(nz * r->ng) + " exceeds what the two-stream kernels can stage"};
      }
    }
    // frequency integration of the cases' up and down spectra (radiate.f90:184-192), two deterministic stages per case
    BatchIntegrateParams bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.nz = nz; bp.ir_lo = r->sol_lo; bp.ir_n = r->sol_n; bp.nchunk = nchunk; bp.col0 = c0;
    bp.fup_a = d_fup; bp.fdn_a = d_fdn; bp.spec_stride = spec;
    bp.freq = r->sol.d_freq.p; bp.partial = r->d_bpartial.p; bp.flux_n = r->d_flux_n.p; bp.out = r->d_bout.p; bp.out_arr = arr;
    launch_integrate_batch(bp, nc, r->stream);
    HIPCHK(hipGetLastError());
    if (nsel > 0) {
      BatchSpectraParams q;
      std::memset(&q, 0, sizeof(q));
      q.ncol = nc; q.nsel = nsel; q.nl = nl; q.level = r->d_spec_level.p; q.src_stride = spec;
      const double *src[3] = {d_fup, d_fdn, d_am};
      for (int k = 0; k < 3; k++) {
        q.src[k] = src[k]; q.nw[k] = nw_sol;
        q.dst[k] = spec_out[k] ? r->d_spec_stage.p + spec_off[k] + (size_t)c0 * nw_sol * nsel : nullptr;
      }
      launch_batch_spectra(q, r->stream);
      HIPCHK(hipGetLastError());
    }
  }
  if (shared_ran) r->solar_batch_shared_batches++;
  if (nsel > 0) {
    double *h = r->h_spec.reserve(spec_total);
    HIPCHK(hipMemcpyAsync(h, r->d_spec_stage.p, sizeof(double) * spec_total, hipMemcpyDeviceToHost, r->stream));
  }
  double *outs[2] = {fup_n, fdn_n};
  bout_to_host(r, outs, arr, 2);
  HIPCHK(hipStreamSynchronize(r->stream));
  if (nsel > 0)
    for (int k = 0; k < 3; k++)
      if (spec_out[k]) std::memcpy(spec_out[k], r->h_spec.p + spec_off[k], sizeof(double) * (size_t)nw_sol * nsel * n);
  if (f_total) {
    // (fdn_n - fup_n) of the case plus the IR rows the handle holds from its last IR call (clima_radtran.f90:287)
    fetch_small(r);
    const double *h = r->h_small;
    const LevelRows &lr = r->rows;
    for (int c = 0; c < n; c++)
      for (int i = 0; i < nl; i++)
        f_total[(size_t)c * nl + i] = f_total_level(h[lr.ir_up + i], h[lr.ir_dn + i], fup_n[(size_t)c * nl + i], fdn_n[(size_t)c * nl + i]);
  }
  CATCH(err)
}

// What the entry points of the IR derivative family (the Jacobians, the spectra batch, its gradients) check alike; `pre`
// is the message's prefix ("name: "), and each returns whether the call is refused, its text in `err`.
// The levels `level` (1..nz+1 ground-first, the argument `name`) as levels from the top in `lv`
static bool ir_levels_refused(const std::string &pre, const char *name, int nz, int n, const int *level, std::vector<int> &lv, char *err) {
  lv.assign((size_t)n, 0);
  for (int a = 0; a < n; a++) {
    const int v = level[a];
    if (v < 1 || v > nz + 1) {
      set_err(err, pre + name + "(" + std::to_string(a + 1) + ") = " + std::to_string(v) + " is outside 1.." + std::to_string(nz + 1));
      return true;
    }
    lv[a] = nz - (v - 1);
  }
  return false;
}
// the functionals of the levels `lv` in the directions asked for: fun[a ndir + place] = 2 (level from the top) + (0 up | 1 down)
static std::vector<int> ir_functionals(const std::vector<int> &lv, bool up, bool dn) {
  std::vector<int> fun;
  for (const int k : lv) {
    if (up) fun.push_back(2 * k);
    if (dn) fun.push_back(2 * k + 1);
  }
  return fun;
}
static bool ir_T_usable(double v) { return std::isfinite(v) && v > 0.0; }
static bool ir_T_refusal(const std::string &pre, const std::string &name, double v, char *err) {
  set_err(err, pre + "temperatures must be finite and positive (" + name + " = " + std::to_string(v) + ")");
  return true;
}
// one column: T(1..nz), then T_surface
static bool ir_column_T_refused(const std::string &pre, int nz, const double *T_surface, const double *T, char *err) {
  for (int i = 0; i < nz; i++)
    if (!ir_T_usable(T[i])) return ir_T_refusal(pre, "T(" + std::to_string(i + 1) + ")", T[i], err);
  return !ir_T_usable(*T_surface) && ir_T_refusal(pre, "T_surface", *T_surface, err);
}
// n columns: per column T_surface(c), then T(1..nz, c)
static bool ir_batch_T_refused(const std::string &pre, int nz, int n, const double *T_surface, const double *T, char *err) {
  for (int c = 0; c < n; c++) {
    if (!ir_T_usable(T_surface[c])) return ir_T_refusal(pre, "T_surface(" + std::to_string(c + 1) + ")", T_surface[c], err);
    for (int i = 0; i < nz; i++) {
      const double v = T[(size_t)c * nz + i];
      if (!ir_T_usable(v)) return ir_T_refusal(pre, "T(" + std::to_string(i + 1) + ", " + std::to_string(c + 1) + ")", v, err);
    }
  }
  return false;
}
// a bin shard or a communicator, by name: the adjoint passes need the whole spectrum
static bool ir_rows_shard_refused(Radtran *r, const std::string &pre, char *err) {
  if (r->shard_world == 1 && !r->comm) return false;
  const std::string shard = r->shard_world != 1 ? "a bin shard of " + std::to_string(r->shard_world) : "";
  set_err(err, pre + "needs the whole spectrum (" + shard + (r->comm ? (shard.empty() ? "a communicator" : ", a communicator") : "") + ")");
  return true;
}

// What its two entry points (radtran_ir_jacobian, radtran_ir_jacobian_reduced) refuse alike, after their own extents.
static bool ir_jacobian_refused(const Radtran *r, const double *T_surface, const double *T, char *err) {
  const int nz = r->nz, nl = nz + 1;
  for (int j = 0; j <= nz; j++) {
    const double v = j < nz ? T[j] : *T_surface;
    if (!(std::isfinite(v) && v > 0.0)) { set_err(err, "ir_jacobian: temperatures must be finite and positive"); return true; }
  }
  if (refuse(r, "ir_jacobian", NEED_SPECTRUM, err)) return true;
  // the response form's range (that of radtran_radiate_ir_batch's): no other solver stands behind it
  if (nz < 4 || nz > 512) { set_err(err, "ir_jacobian: the response form takes 4 <= nz <= 512 (nz = " + std::to_string(nz) + ")"); return true; }
  if ((long)r->ir_n * r->ng > 65535) {     // (k_green_unit / k_green_local: one (bin, g-point) pair per blockIdx.y)
    set_err(err, "ir_jacobian: the response form takes at most 65535 (bin, g-point) pairs (" + std::to_string((long)r->ir_n * r->ng) + ")");
    return true;
  }
  if (green_work_bytes(r, nl) > 16.0e9) { set_err(err, "ir_jacobian: the response form's work arrays would take more than 16 GB"); return true; }
  return refuse(r, "ir_jacobian", NEED_OPACITIES, err);   // (last: what the form cannot take is refused before any opacity is needed)
}
// The opacity-only part and the accumulation's arrays for the Jacobian's deviations: every level k, sorted
// (dev_k[d] = d).  `extra`: further ints of the caller's, staged behind the lists; returns their place on the device.
static const int *ir_jacobian_green_part(Radtran *r, const double *T_surface, const double *T, const std::vector<int> &extra, GreenParams &g) {
  const int nz = r->nz, nl = nz + 1;
  // the mixed pairs as the batch builds them
  const int ndev = nl, ndev_pad = green_ndev_pad(ndev);
  std::vector<int> dev_k(ndev), mdev, mblk;
  for (int k = 0; k < ndev; k++) dev_k[k] = k;
  green_mixed_list(dev_k, nz, mdev, mblk);
  const int nmix = (int)mdev.size();
  // through the handle's pinned block: doubles base_T by level k [nl], then ints dev_k [ndev_pad] | mix_dev | mix_blk | extra
  const size_t ni = (size_t)ndev_pad + 2 * (size_t)nmix + extra.size();
  double *hd = reinterpret_cast<double *>(green_stage(r, sizeof(double) * nl + sizeof(int) * ni));
  int *hi = reinterpret_cast<int *>(hd + nl);
  for (int k = 0; k < nz; k++) hd[k] = T[nz - 1 - k];     // (radiate.f90:65-69: level k is layer nz-1-k)
  hd[nz] = *T_surface;
  for (int d = 0; d < ndev_pad; d++) hi[d] = d < ndev ? d : 0;
  std::copy(extra.begin(), extra.end(), std::copy(mblk.begin(), mblk.end(), std::copy(mdev.begin(), mdev.end(), hi + ndev_pad)));
  r->d_green_in.reserve(nl);
  r->d_green_idx.reserve(ni);
  HIPCHK(hipMemcpyAsync(r->d_green_in.p, hd, sizeof(double) * nl, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipMemcpyAsync(r->d_green_idx.p, hi, sizeof(int) * ni, hipMemcpyHostToDevice, r->stream));
  green_factor_part(r, g);
  green_accum_arrays(r, g, ndev, nmix);
  g.dev_k = r->d_green_idx.p; g.mix_dev = g.dev_k + ndev_pad; g.mix_blk = g.mix_dev + nmix;
  g.base_T = r->d_green_in.p;
  return g.mix_blk + nmix;
}
// The exact IR temperature Jacobian of the level fluxes: the limit of the batch's response form as the step goes to 0.
// Every level k = 0..nz is one deviation with the Planck derivative at its base temperature as amplitude, so the
// matrices come from the opacity-only part and one accumulation alone -- no base-profile solve, no plan, no step.
// jac_*(i, j) column-major (nz+1) x (nz+1): i the level ground-first, x(1) = T_surface, x(1 + m) = T(m).
void radtran_ir_jacobian(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                         const int *dim1, const int *dim2, double *jac_up, double *jac_dn, double *jac_total, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nz = r->nz, nl = nz + 1;
  if (*dim_T != nz) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (*dim1 != nl || *dim2 != nl) { set_err(err, "jac has the wrong dimension"); return; }
  if (ir_jacobian_refused(r, T_surface, T, err)) return;
  TRY
  ready_stored_opacities(r);
  const size_t arr = (size_t)nl * nl;
  r->d_bout.reserve(3 * arr);
  jacobian_of_ir_bins(r, 3 * arr, [&] {
    GreenParams g;
    ir_jacobian_green_part(r, T_surface, T, {}, g);
    g.out = r->d_bout.p; g.out_arr = arr;
    launch_green_jacobian(g, r->stream);
  });
  comm_reduce_up_down(r, arr, [&] { launch_jacobian_total(r->d_bout.p, arr, arr, r->stream); });
  double *const outs[3] = {jac_up, jac_dn, jac_total};
  bout_to_host(r, outs, arr);
  CATCH(err)
}

// The same derivative in the caller's unknowns (the RCE Jacobian's: a pair of the doubled radiative grid, a convective
// zone and the ghost layers move with ONE unknown, and only some levels are read -- clima_adiabat_solve.f90:731-733,
// 798-809): jac(a, g) = sum over the x(j) of group g, ascending j, of J(row_level(a), j).  The full matrices are never
// formed: k_green_jacobian_reduced adds the members' entries as it forms them, and (nrow, ngroup) doubles per requested
// matrix come back instead of 3 (nz+1)^2.  jac_up and jac_dn may both be NULL: the total alone.
void radtran_ir_jacobian_reduced(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                 const int *dim_x, const int *group_of_x, const int *ngroup,
                                 const int *nrow, const int *row_level,
                                 const int *dim1, const int *dim2,
                                 double *jac_up, double *jac_dn, double *jac_total, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nz = r->nz, nl = nz + 1, ng = *ngroup, nr = *nrow;
  const std::string pre = "ir_jacobian_reduced: ";
  if (*dim_T != nz) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (*dim_x != nl) {
    set_err(err, pre + "\"group_of_x\" has the wrong dimension (dim_x = " + std::to_string(*dim_x) + ", nz + 1 = " + std::to_string(nl) + ")");
    return;
  }
  if (nr < 1) { set_err(err, pre + "nrow must be at least 1 (nrow = " + std::to_string(nr) + ")"); return; }
  if (ng < 1) { set_err(err, pre + "ngroup must be at least 1 (ngroup = " + std::to_string(ng) + ")"); return; }
  if (*dim1 != nr || *dim2 != ng) { set_err(err, "jac has the wrong dimension"); return; }
  if (!jac_total) { set_err(err, pre + "jac_total is required (only jac_up and jac_dn may be absent)"); return; }
  if ((jac_up == nullptr) != (jac_dn == nullptr)) {
    set_err(err, pre + "jac_up and jac_dn go together: only " + (jac_up ? "jac_up" : "jac_dn") + " was given");
    return;
  }
  // the map as a CSR of the groups' members (deviation = level k = nz - (j - 1), members in ascending j), then the rows
  // as levels TOA-first
  std::vector<int> csr((size_t)ng + 1, 0);
  for (int j = 0; j < nl; j++) {
    const int v = group_of_x[j];
    if (v < 0 || v > ng) {
      set_err(err, pre + "group_of_x(" + std::to_string(j + 1) + ") = " + std::to_string(v) + " is outside 0.." + std::to_string(ng));
      return;
    }
    if (v > 0) csr[v]++;
  }
  for (int v = 1; v <= ng; v++) {
    // (an empty column is an off-by-one in the caller's map, not a request)
    if (csr[v] == 0) { set_err(err, pre + "group " + std::to_string(v) + " of " + std::to_string(ng) + " has no member in group_of_x"); return; }
    csr[v] += csr[v - 1];
  }
  const int nmem = csr[ng];
  std::vector<int> fill(csr.begin(), csr.end() - 1);
  csr.resize((size_t)ng + 1 + nmem + nr);
  int *mem = csr.data() + ng + 1, *rows = mem + nmem;
  for (int j = 0; j < nl; j++)
    if (group_of_x[j] > 0) mem[fill[group_of_x[j] - 1]++] = nz - j;
  std::vector<int> lv;
  if (ir_levels_refused(pre, "row_level", nz, nr, row_level, lv, err)) return;
  std::copy(lv.begin(), lv.end(), rows);
  if (ir_jacobian_refused(r, T_surface, T, err)) return;
  TRY
  ready_stored_opacities(r);
  const size_t arr = (size_t)nr * ng;
  // a communicator handle forms up and down whatever was asked for: they are what is summed over the ranks
  const bool want_parts = jac_up != nullptr, parts = want_parts || r->comm;
  const size_t need = (parts ? 3 : 1) * arr;
  r->d_bout.reserve(need);
  jacobian_of_ir_bins(r, need, [&] {
    GreenParams g;
    const int *d_map = ir_jacobian_green_part(r, T_surface, T, csr, g);
    g.col_ptr = d_map; g.col_dev = d_map + ng + 1;
    g.out = r->d_bout.p; g.out_arr = arr;
    launch_green_jacobian_reduced(g, d_map + ng + 1 + nmem, nr, ng, parts, r->stream);
  });
  comm_reduce_up_down(r, arr, [&] { launch_jacobian_total(r->d_bout.p, arr, arr, r->stream); });   // (2 nrow ngroup doubles)
  double *const outs[3] = {jac_up, jac_dn, jac_total};
  if (want_parts) bout_to_host(r, outs, arr);
  else bout_to_host(r, &jac_total, arr, 1, parts ? 2 : 0);
  CATCH(err)
}

// Rows of the same derivative BEFORE the sum over the bins: jac_*_a(l, a, j) = d wrk_ir%f*_a(row_level(a), l) / d x(j), per
// Hz.  Not the response form: one adjoint two-stream solve per (bin, g-point, requested row, direction) gives the whole
// row (ir_adjoint.inc), so none of the response form's limits apply; what bounds the call is its work buffer.
// include/clima_radtran_hip.h has the contract.
constexpr double IR_ADJOINT_MAX_BYTES = 4294967296.0;
// the adjoint work buffer of `count` rows or levels (the `noun`; `count_name` the argument that counts them) in ndir
// directions: refused, with its size, where it passes IR_ADJOINT_MAX_BYTES
static bool ir_adjoint_work_refused(Radtran *r, const std::string &pre, const char *noun, const char *count_name, int count, int ndir, char *err) {
  const int NQ = r->ir_n * r->ng, nfun = count * ndir;
  const size_t n_work = ir_adjoint_work_count(r->nz, NQ, nfun), n_part = ir_adjoint_part_count(r->nz, NQ, nfun);
  if (sizeof(double) * ((double)n_work + (double)n_part) <= IR_ADJOINT_MAX_BYTES) return false;
  set_err(err, pre + "the work buffer of " + count_name + " = " + std::to_string(count) + " " + noun + " in " + std::to_string(ndir) +
                   " direction(s) would take " + std::to_string(sizeof(double) * (n_work + n_part)) + " bytes, more than " +
                   std::to_string((long long)IR_ADJOINT_MAX_BYTES) + ": ask for fewer " + noun + " per call");
  return true;
}
// A small index list up into d_green_idx.  A call that may only enqueue (`enqueue_only`) sends it from pageable memory: a
// copy from memory that is not pinned is performed synchronously (hip_runtime_api.h, hipMemcpyAsync), so `v` has been
// read when the call returns and a call right behind this one cannot change what this one reads -- the handle's shared
// pinned block could be rewritten before a copy from it executes.  The price: the host waits until the stream has
// reached the copy.  A synchronous host form returns only when its copies have run, so it may use the pinned block
// (from its start: nothing else of the call may be staged there), which costs no wait.  The device buffer itself is
// reused in stream order.
static const int *ir_upload_indices(Radtran *r, const std::vector<int> &v, bool enqueue_only) {
  const int *src = v.data();
  if (!enqueue_only) {
    int *h = reinterpret_cast<int *>(green_stage(r, sizeof(int) * v.size()));
    std::copy(v.begin(), v.end(), h);
    src = h;
  }
  r->d_green_idx.reserve(v.size());
  HIPCHK(hipMemcpyAsync(r->d_green_idx.p, src, sizeof(int) * v.size(), hipMemcpyHostToDevice, r->stream));
  return r->d_green_idx.p;
}
// The adjoint pass on the stored opacities: the rows of the nrow x ndir functionals d_fun (`up`: the up direction is
// among them) into d_out_up / d_out_dn ((nw_ir, nrow, nz+1) each; null: the direction is not among them), with the Planck
// derivatives at d_base_T (by level from the top) as amplitudes -- null: unit amplitudes, the rows are the spectra
// batch's weights themselves.  Enqueued on the handle's stream, behind ready_stored_opacities; `timed`: counted as
// kernel id 4 (the weights pass of the spectra batches).
static void ir_adjoint_enqueue(Radtran *r, const int *d_fun, int nrow, int ndir, bool up, const double *d_base_T,
                               double *d_out_up, double *d_out_dn, bool timed) {
  const int nfun = nrow * ndir;
  IrAdjointParams p;
  std::memset(&p, 0, sizeof(p));
  p.g = green_params(r);
  p.g.base_T = d_base_T;
  const size_t n_work = ir_adjoint_work_count(r->nz, p.g.NQ, nfun), n_part = ir_adjoint_part_count(r->nz, p.g.NQ, nfun);
  r->d_adjoint.reserve(n_work + n_part);
  p.nfun = nfun; p.nrow = nrow; p.ndir = ndir; p.dir0 = up ? 0 : 1; p.fun = d_fun;
  p.work = r->d_adjoint.p; p.part = p.work + n_work;
  p.out_up = d_out_up; p.out_dn = d_out_dn;
  if (timed) {
    KernelTimer t(r, 4);
    launch_ir_adjoint(p, r->stream);
    t.stop();
  } else {
    launch_ir_adjoint(p, r->stream);
  }
  HIPCHK(hipGetLastError());
}
void radtran_ir_jacobian_spectral_rows(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                       const int *nrow, const int *row_level,
                                       const int *dim1, const int *dim2, const int *dim3,
                                       double *jac_up_a, double *jac_dn_a, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nz = r->nz, nl = nz + 1, nw_ir = r->ir.nw, nr = *nrow;
  const std::string pre = "ir_jacobian_spectral_rows: ";
  if (*dim_T != nz) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (nr < 1) { set_err(err, pre + "nrow must be at least 1 (nrow = " + std::to_string(nr) + ")"); return; }
  if (!row_level) { set_err(err, pre + "\"row_level\" is a required argument"); return; }
  if (*dim1 != nw_ir || *dim2 != nr || *dim3 != nl) {
    set_err(err, pre + "jac has the wrong dimension (" + std::to_string(*dim1) + ", " + std::to_string(*dim2) + ", " + std::to_string(*dim3) +
                     "), not (nw_ir, nrow, nz + 1) = (" + std::to_string(nw_ir) + ", " + std::to_string(nr) + ", " + std::to_string(nl) + ")");
    return;
  }
  if (!jac_up_a && !jac_dn_a) { set_err(err, pre + "neither jac_up_a nor jac_dn_a was given"); return; }
  const bool up = jac_up_a != nullptr, dn = jac_dn_a != nullptr;
  const int ndir = (up ? 1 : 0) + (dn ? 1 : 0);
  std::vector<int> lv;
  if (ir_levels_refused(pre, "row_level", nz, nr, row_level, lv, err)) return;
  if (ir_column_T_refused(pre, nz, T_surface, T, err)) return;
  if (ir_rows_shard_refused(r, pre, err)) return;
  if (refuse(r, "ir_jacobian_spectral_rows", NEED_OPACITIES, err)) return;
  if (ir_adjoint_work_refused(r, pre, "rows", "nrow", nr, ndir, err)) return;
  TRY
  ready_stored_opacities(r);
  const size_t arr = (size_t)nw_ir * nr * nl;
  r->d_bout.reserve(ndir * arr);
  jacobian_of_ir_bins(r, ndir * arr, [&] {
    // through the handle's pinned block: base_T by level k [nl] (radiate.f90:65-69: level k is layer nz-1-k), then the functionals
    const std::vector<int> fun = ir_functionals(lv, up, dn);
    double *hd = reinterpret_cast<double *>(green_stage(r, sizeof(double) * nl + sizeof(int) * fun.size()));
    int *hi = reinterpret_cast<int *>(hd + nl);
    for (int k = 0; k < nz; k++) hd[k] = T[nz - 1 - k];
    hd[nz] = *T_surface;
    std::copy(fun.begin(), fun.end(), hi);
    r->d_green_in.reserve(nl); r->d_green_idx.reserve(fun.size());
    HIPCHK(hipMemcpyAsync(r->d_green_in.p, hd, sizeof(double) * nl, hipMemcpyHostToDevice, r->stream));
    HIPCHK(hipMemcpyAsync(r->d_green_idx.p, hi, sizeof(int) * fun.size(), hipMemcpyHostToDevice, r->stream));
    ir_adjoint_enqueue(r, r->d_green_idx.p, nr, ndir, up, r->d_green_in.p, up ? r->d_bout.p : nullptr,
                       dn ? r->d_bout.p + (up ? arr : 0) : nullptr, false);
  });
  double *const outs[2] = {up ? jac_up_a : jac_dn_a, jac_dn_a};
  bout_to_host(r, outs, arr, ndir);
  CATCH(err)
}

// Per-bin IR spectra (and their sums over the bins) of many temperature profiles on the stored opacities, at requested
// levels: ONE adjoint pass with unit amplitudes gives the weights W of every requested (level, direction) (ir_adjoint.inc),
// after which a column is W times its Planck values (ir_rows_apply.inc) -- no solve per column.
// include/clima_radtran_hip.h has the contract.
constexpr int IR_ROWS_CHUNK = 512;                     // columns per launch (radtran_radiate_solar_batch's)
constexpr double IR_ROWS_CHUNK_BYTES = 268435456.0;    // ... fewer where their spectra would take more than this
// columns per launch where the spectra of `nstaged` directions (`spec` doubles per column each) pass through d_rows_out
static int ir_rows_chunk(int n, int nstaged, size_t spec) {
  int CH = std::min(n, IR_ROWS_CHUNK);
  while (CH > 1 && sizeof(double) * (double)nstaged * spec * CH > IR_ROWS_CHUNK_BYTES) CH = (CH + 1) / 2;
  return CH;
}
// Where the apply pass writes one direction's spectra or sums: into the device array of all columns (`step` doubles per
// column: a chunk writes its part in place), or into a staging area that every chunk fills from its start (step 0);
// p null: not formed
struct IrRowsDst { double *p; size_t step; };
// The apply pass of the spectra batch: the columns (d_T, d_Ts) [0, n) times the weights w[0..ndir) in chunks of CH columns
// (kernel id 5 counts them all), direction d's spectra to spec_dst[d] and their sums over the bins to sum_dst[d].  After
// each chunk `chunk_done` (where given) is told where the chunk's spectra o[d] and sums f[d] lie.
using IrRowsChunkDone = std::function<void(int c0, int nc, double *const *o, double *const *f)>;
static void ir_rows_apply(Radtran *r, int n, int CH, int nsel, int ndir, const double *d_T, const double *d_Ts, const double *const w[2],
                          const IrRowsDst spec_dst[2], const IrRowsDst sum_dst[2], const IrRowsChunkDone &chunk_done) {
  const size_t sums = (size_t)nsel;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int nc = std::min(CH, n - c0);
    double *o[2], *f[2];
    for (int d = 0; d < 2; d++) {
      o[d] = spec_dst[d].p ? spec_dst[d].p + spec_dst[d].step * c0 : nullptr;
      f[d] = sum_dst[d].p ? sum_dst[d].p + sum_dst[d].step * c0 : nullptr;
    }
    if (r->ir_n > 0) {
      IrRowsApplyParams q;
      std::memset(&q, 0, sizeof(q));
      q.n_ir = r->ir_n; q.nsel = nsel; q.nz = r->nz; q.ncol = nc; q.ndir = ndir;
      q.l0 = r->ir.ind_start + r->ir_lo; q.ir_lo = r->ir_lo;
      q.freq = r->d_freq.p; q.ir_freq = r->ir.d_freq.p;
      q.T = d_T + (size_t)c0 * r->nz; q.Ts = d_Ts + c0;
      q.w0 = w[0]; q.w1 = w[1];
      q.out0 = o[0]; q.out1 = o[1]; q.fn0 = f[0]; q.fn1 = f[1];
      KernelTimer t(r, 5);
      launch_ir_rows_apply(q, r->stream);
      HIPCHK(hipGetLastError());
      t.stop();
    } else {
      for (int d = 0; d < 2; d++)
        if (f[d]) HIPCHK(hipMemsetAsync(f[d], 0, sizeof(double) * sums * nc, r->stream));   // (no IR bins: empty spectra, sums of nothing)
    }
    if (chunk_done) chunk_done(c0, nc, o, f);
  }
}
void radtran_ir_spectra_batch(void *ptr, const int *ncol, const double *T_surface, const int *dim1_T, const int *dim2_T,
                              const double *T, const int *nsel_, const int *spec_level, double *ir_fup, double *ir_fdn,
                              double *fup_n, double *fdn_n, double *w_up, double *w_dn, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nz = r->nz, nl = nz + 1, nw_ir = r->ir.nw, n = *ncol, nsel = *nsel_;
  const std::string pre = "ir_spectra_batch: ";
  if (n < 0) { set_err(err, pre + "ncol must not be negative (ncol = " + std::to_string(n) + ")"); return; }
  if (*dim1_T != nz || *dim2_T != n) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(nsel) + ")"); return; }
  if (!spec_level) { set_err(err, pre + "\"spec_level\" is a required argument"); return; }
  const bool up = ir_fup || fup_n || w_up, dn = ir_fdn || fdn_n || w_dn;
  if (!up && !dn) { set_err(err, pre + "none of ir_fup, ir_fdn, fup_n, fdn_n, w_up, w_dn was given"); return; }
  const int ndir = (up ? 1 : 0) + (dn ? 1 : 0);
  std::vector<int> lv;
  if (ir_levels_refused(pre, "spec_level", nz, nsel, spec_level, lv, err)) return;
  if (n == 0 && (ir_fup || ir_fdn || fup_n || fdn_n)) {
    set_err(err, pre + "ncol = 0 gives the weights alone, but " + (ir_fup ? "ir_fup" : ir_fdn ? "ir_fdn" : fup_n ? "fup_n" : "fdn_n") + " was asked for");
    return;
  }
  if (n > 0) {
    if (!T) { set_err(err, pre + "\"T\" is a required argument (ncol = " + std::to_string(n) + ")"); return; }
    if (!T_surface) { set_err(err, pre + "\"T_surface\" is a required argument (ncol = " + std::to_string(n) + ")"); return; }
    if (ir_batch_T_refused(pre, nz, n, T_surface, T, err)) return;
  }
  if (ir_rows_shard_refused(r, pre, err)) return;
  if (refuse(r, "ir_spectra_batch", NEED_OPACITIES, err)) return;
  if (ir_adjoint_work_refused(r, pre, "levels", "nsel", nsel, ndir, err)) return;
  TRY
  ready_stored_opacities(r);
  // the weights: (nw_ir, nsel, nz+1) per direction asked for, up before down
  const size_t arr_w = (size_t)nw_ir * nsel * nl;
  r->d_rows_w.reserve(std::max<size_t>(1, ndir * arr_w));
  double *const d_w_up = up ? r->d_rows_w.p : nullptr, *const d_w_dn = dn ? r->d_rows_w.p + (up ? arr_w : 0) : nullptr;
  if (r->ir_n > 0) ir_adjoint_enqueue(r, ir_upload_indices(r, ir_functionals(lv, up, dn), false), nsel, ndir, up, nullptr, d_w_up, d_w_dn, true);
  if (w_up) rows_to_host(r, d_w_up, w_up, arr_w);
  if (w_dn) rows_to_host(r, d_w_dn, w_dn, arr_w);
  if (n > 0) {
    r->d_bT.reserve((size_t)n * nz); r->d_bTs.reserve(n);
    HIPCHK(hipMemcpyAsync(r->d_bT.p, T, sizeof(double) * (size_t)n * nz, hipMemcpyHostToDevice, r->stream));
    HIPCHK(hipMemcpyAsync(r->d_bTs.p, T_surface, sizeof(double) * n, hipMemcpyHostToDevice, r->stream));
    const size_t spec = (size_t)nw_ir * nsel, sums = (size_t)nsel;      // per column and direction
    const int CH = ir_rows_chunk(n, ndir, spec);
    r->d_rows_out.reserve(std::max<size_t>(1, (size_t)ndir * (spec + sums) * CH));
    double *const outs[2] = {up ? ir_fup : ir_fdn, dn && up ? ir_fdn : nullptr};
    double *const fns[2] = {up ? fup_n : fdn_n, dn && up ? fdn_n : nullptr};
    // every chunk is staged in d_rows_out, the directions' spectra before their sums, and copied back from there
    const double *const w[2] = {r->d_rows_w.p, ndir == 2 ? r->d_rows_w.p + arr_w : nullptr};
    double *const stage = r->d_rows_out.p, *const stage_n = stage + (size_t)ndir * spec * CH;
    IrRowsDst spec_dst[2], sum_dst[2];
    for (int d = 0; d < 2; d++) {
      spec_dst[d] = {d < ndir ? stage + (size_t)d * spec * CH : nullptr, 0};
      sum_dst[d] = {fns[d] ? stage_n + (size_t)d * sums * CH : nullptr, 0};
    }
    ir_rows_apply(r, n, CH, nsel, ndir, r->d_bT.p, r->d_bTs.p, w, spec_dst, sum_dst, [&](int c0, int nc, double *const *o, double *const *f) {
      for (int d = 0; d < ndir; d++) {
        if (outs[d]) rows_to_host(r, o[d], outs[d] + spec * c0, spec * nc);
        if (fns[d]) rows_to_host(r, f[d], fns[d] + sums * c0, sums * nc);
      }
    });
  }
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

// the first of `args` that is given and is not device memory of the handle's device, named in `err` (toa_fluxes_batch_dev's check)
struct NamedPtr { const char *name; const void *p; };
static bool ir_rows_not_device(Radtran *r, const std::string &pre, std::initializer_list<NamedPtr> args, char *err) {
  for (const auto &a : args)
    if (a.p && !on_handle_device(r, a.p)) {
      set_err(err, pre + "\"" + a.name + "\" is not device memory of this handle's device");
      return true;
    }
  return false;
}
static void wait_for_producer(Radtran *r, const void *producer_stream) {
  if (!producer_stream) return;
  if (!r->ev_producer) HIPCHK(hipEventCreateWithFlags(&r->ev_producer, hipEventDisableTiming));
  HIPCHK(hipEventRecord(r->ev_producer, reinterpret_cast<hipStream_t>(const_cast<void *>(producer_stream))));
  HIPCHK(hipStreamWaitEvent(r->stream, r->ev_producer, 0));
}
constexpr int IR_ROWS_DEVICE_CHUNK = 262144;           // columns per launch of the device forms: what the grids take

// radtran_ir_spectra_batch with every array but spec_level in device memory, the weights kept by the caller
// (weights_given = 0: computed here, and stored in d_w_up / d_w_dn where given; 1: read from there, no adjoint pass, no
// opacities needed).  The same two launchers as the host form, writing straight into the caller's arrays; enqueued behind
// producer_stream, nothing waited for.  include/clima_radtran_hip.h has the contract.
void radtran_ir_spectra_batch_device(void *ptr, const int *ncol, const double *d_T_surface, const int *dim1_T, const int *dim2_T,
                                     const double *d_T, const int *nsel_, const int *spec_level, double *d_ir_fup, double *d_ir_fdn,
                                     double *d_fup_n, double *d_fdn_n, double *d_w_up, double *d_w_dn, const int *weights_given,
                                     const void *producer_stream, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int nz = r->nz, nl = nz + 1, nw_ir = r->ir.nw, n = *ncol, nsel = *nsel_;
  const bool given = weights_given && *weights_given != 0;
  const std::string pre = "ir_spectra_batch_device: ";
  if (n < 0) { set_err(err, pre + "ncol must not be negative (ncol = " + std::to_string(n) + ")"); return; }
  if (*dim1_T != nz || *dim2_T != n) { set_err(err, "\"T\" has the wrong input dimension."); return; }
  if (nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(nsel) + ")"); return; }
  if (!spec_level) { set_err(err, pre + "\"spec_level\" is a required argument"); return; }
  const bool flux_up = d_ir_fup || d_fup_n, flux_dn = d_ir_fdn || d_fdn_n;
  const bool up = flux_up || (!given && d_w_up), dn = flux_dn || (!given && d_w_dn);
  if (!up && !dn) {
    set_err(err, pre + (given ? "none of ir_fup, ir_fdn, fup_n, fdn_n was given (weights_given = 1)" : "none of ir_fup, ir_fdn, fup_n, fdn_n, w_up, w_dn was given"));
    return;
  }
  if (given && ((flux_up && !d_w_up) || (flux_dn && !d_w_dn))) {
    set_err(err, pre + "\"" + (flux_up && !d_w_up ? "w_up" : "w_dn") + "\" is a required argument (weights_given = 1 and its direction is asked for)");
    return;
  }
  const int ndir = (up ? 1 : 0) + (dn ? 1 : 0);
  std::vector<int> lv;
  if (ir_levels_refused(pre, "spec_level", nz, nsel, spec_level, lv, err)) return;
  if (n == 0 && (flux_up || flux_dn)) {
    set_err(err, pre + "ncol = 0 gives the weights alone, but " + (d_ir_fup ? "ir_fup" : d_ir_fdn ? "ir_fdn" : d_fup_n ? "fup_n" : "fdn_n") + " was asked for");
    return;
  }
  if (n > 0) {
    if (!d_T) { set_err(err, pre + "\"T\" is a required argument (ncol = " + std::to_string(n) + ")"); return; }
    if (!d_T_surface) { set_err(err, pre + "\"T_surface\" is a required argument (ncol = " + std::to_string(n) + ")"); return; }
  }
  if (ir_rows_not_device(r, pre, {{"T_surface", n > 0 ? d_T_surface : nullptr}, {"T", n > 0 ? d_T : nullptr}, {"ir_fup", d_ir_fup}, {"ir_fdn", d_ir_fdn},
                                  {"fup_n", d_fup_n}, {"fdn_n", d_fdn_n}, {"w_up", up ? d_w_up : nullptr}, {"w_dn", dn ? d_w_dn : nullptr}}, err)) return;
  if (ir_rows_shard_refused(r, pre, err)) return;
  if (!given) {
    if (refuse(r, "ir_spectra_batch_device", NEED_OPACITIES, err)) return;
    if (ir_adjoint_work_refused(r, pre, "levels", "nsel", nsel, ndir, err)) return;
  }
  TRY
  if (given) settle_device_batch(r); else ready_stored_opacities(r);
  wait_for_producer(r, producer_stream);
  const size_t arr_w = (size_t)nw_ir * nsel * nl;
  // the weights of the directions at places 0 and 1: the caller's arrays, or (computed here and not asked for) the handle's
  const double *w[2] = {nullptr, nullptr};
  if (given) {
    w[0] = up ? d_w_up : d_w_dn; w[1] = up && dn ? d_w_dn : nullptr;
  } else {
    double *own = nullptr;
    if ((up && !d_w_up) || (dn && !d_w_dn)) { r->d_rows_w.reserve(std::max<size_t>(1, ndir * arr_w)); own = r->d_rows_w.p; }
    double *const wu = up ? (d_w_up ? d_w_up : own) : nullptr, *const wd = dn ? (d_w_dn ? d_w_dn : own + (up ? arr_w : 0)) : nullptr;
    if (r->ir_n > 0) ir_adjoint_enqueue(r, ir_upload_indices(r, ir_functionals(lv, up, dn), true), nsel, ndir, up, nullptr, wu, wd, true);
    w[0] = up ? wu : wd; w[1] = up && dn ? wd : nullptr;
  }
  if (n > 0) {
    const size_t spec = (size_t)nw_ir * nsel, sums = (size_t)nsel;      // per column and direction
    double *const outs[2] = {up ? d_ir_fup : d_ir_fdn, dn && up ? d_ir_fdn : nullptr};
    double *const fns[2] = {up ? d_fup_n : d_fdn_n, dn && up ? d_fdn_n : nullptr};
    // straight into the caller's arrays; a sum asked for without its spectrum: the spectra of such a direction pass
    // through d_rows_out, in the host form's chunks
    int nstaged = 0;
    for (int d = 0; d < ndir; d++) nstaged += outs[d] ? 0 : 1;
    const int CH = nstaged ? ir_rows_chunk(n, nstaged, spec) : std::min(n, IR_ROWS_DEVICE_CHUNK);
    if (nstaged) r->d_rows_out.reserve(std::max<size_t>(1, (size_t)nstaged * spec * CH));
    double *stage = r->d_rows_out.p;
    IrRowsDst spec_dst[2] = {{nullptr, 0}, {nullptr, 0}}, sum_dst[2] = {{fns[0], sums}, {fns[1], sums}};
    for (int d = 0; d < ndir; d++) {
      if (outs[d]) spec_dst[d] = {outs[d], spec};
      else { spec_dst[d] = {stage, 0}; stage += spec * CH; }
    }
    ir_rows_apply(r, n, CH, nsel, ndir, d_T, d_T_surface, w, spec_dst, sum_dst, nullptr);
  }
  CATCH(err)
}

// The temperature gradient of the spectra batch: device arrays in, device arrays out, enqueued on the handle's stream in
// chunks of columns (kernel id 6).  w / gs / gn: [up, down], null where not given; a direction without a cotangent is left out.
static void ir_rows_vjp_enqueue(Radtran *r, int n, int nsel, const double *d_Ts, const double *d_T, const double *const w[2],
                                const double *const gs[2], const double *const gn[2], double *d_grad_Ts, double *d_grad_T) {
  const int nz = r->nz;
  if (r->ir_n < 1) {   // (no IR bins: nothing depends on the temperatures)
    HIPCHK(hipMemsetAsync(d_grad_T, 0, sizeof(double) * (size_t)n * nz, r->stream));
    HIPCHK(hipMemsetAsync(d_grad_Ts, 0, sizeof(double) * n, r->stream));
    return;
  }
  const size_t spec = (size_t)r->ir.nw * nsel, sums = (size_t)nsel;
  IrRowsVjpParams q;
  std::memset(&q, 0, sizeof(q));
  q.n_ir = r->ir_n; q.nsel = nsel; q.nz = nz;
  q.l0 = r->ir.ind_start + r->ir_lo; q.ir_lo = r->ir_lo;
  q.freq = r->d_freq.p; q.ir_freq = r->ir.d_freq.p;
  for (int c0 = 0; c0 < n; c0 += IR_ROWS_DEVICE_CHUNK) {
    const int nc = std::min(IR_ROWS_DEVICE_CHUNK, n - c0);
    q.ncol = nc; q.ndir = 0;
    q.T = d_T + (size_t)c0 * nz; q.Ts = d_Ts + c0;
    q.grad_T = d_grad_T + (size_t)c0 * nz; q.grad_Ts = d_grad_Ts + c0;
    for (int d = 0; d < 2; d++) {
      if (!gs[d] && !gn[d]) continue;
      (q.ndir ? q.w1 : q.w0) = w[d];
      (q.ndir ? q.gs1 : q.gs0) = gs[d] ? gs[d] + spec * c0 : nullptr;
      (q.ndir ? q.gn1 : q.gn0) = gn[d] ? gn[d] + sums * c0 : nullptr;
      q.ndir++;
    }
    KernelTimer t(r, 6);
    launch_ir_rows_vjp(q, r->stream);
    HIPCHK(hipGetLastError());
    t.stop();
  }
}
// what both gradient forms refuse, with the batch's wording; false: the call can run
static bool ir_rows_vjp_refused(Radtran *r, const std::string &pre, int n, int dim1_T, int dim2_T, int nsel, const void *T_surface,
                                const void *T, const double *const w[2], const double *const gs[2], const double *const gn[2],
                                const void *grad_T_surface, const void *grad_T, char *err) {
  if (n < 1) { set_err(err, pre + "ncol must be at least 1 (ncol = " + std::to_string(n) + ")"); return true; }
  if (dim1_T != r->nz || dim2_T != n) { set_err(err, "\"T\" has the wrong input dimension."); return true; }
  if (nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(nsel) + ")"); return true; }
  if (!T) { set_err(err, pre + "\"T\" is a required argument (ncol = " + std::to_string(n) + ")"); return true; }
  if (!T_surface) { set_err(err, pre + "\"T_surface\" is a required argument (ncol = " + std::to_string(n) + ")"); return true; }
  if (!grad_T) { set_err(err, pre + "\"grad_T\" is a required argument"); return true; }
  if (!grad_T_surface) { set_err(err, pre + "\"grad_T_surface\" is a required argument"); return true; }
  if (!w[0] && !w[1]) { set_err(err, pre + "neither w_up nor w_dn was given"); return true; }
  static const char *const GS[2] = {"g_ir_fup", "g_ir_fdn"}, *const GN[2] = {"g_fup_n", "g_fdn_n"}, *const W[2] = {"w_up", "w_dn"};
  for (int d = 0; d < 2; d++)
    if (!w[d] && (gs[d] || gn[d])) {
      set_err(err, pre + "\"" + (gs[d] ? GS[d] : GN[d]) + "\" was given without \"" + W[d] + "\"");
      return true;
    }
  if (!gs[0] && !gs[1] && !gn[0] && !gn[1]) { set_err(err, pre + "none of g_ir_fup, g_ir_fdn, g_fup_n, g_fdn_n was given"); return true; }
  return ir_rows_shard_refused(r, pre, err);
}

void radtran_ir_spectra_batch_vjp_device(void *ptr, const int *ncol, const double *d_T_surface, const int *dim1_T, const int *dim2_T,
                                         const double *d_T, const int *nsel_, const double *d_w_up, const double *d_w_dn,
                                         const double *d_g_ir_fup, const double *d_g_ir_fdn, const double *d_g_fup_n,
                                         const double *d_g_fdn_n, double *d_grad_T_surface, double *d_grad_T,
                                         const void *producer_stream, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const std::string pre = "ir_spectra_batch_vjp_device: ";
  const double *const w[2] = {d_w_up, d_w_dn}, *const gs[2] = {d_g_ir_fup, d_g_ir_fdn}, *const gn[2] = {d_g_fup_n, d_g_fdn_n};
  if (ir_rows_vjp_refused(r, pre, *ncol, *dim1_T, *dim2_T, *nsel_, d_T_surface, d_T, w, gs, gn, d_grad_T_surface, d_grad_T, err)) return;
  if (ir_rows_not_device(r, pre, {{"T_surface", d_T_surface}, {"T", d_T}, {"w_up", d_w_up}, {"w_dn", d_w_dn}, {"g_ir_fup", d_g_ir_fup},
                                  {"g_ir_fdn", d_g_ir_fdn}, {"g_fup_n", d_g_fup_n}, {"g_fdn_n", d_g_fdn_n},
                                  {"grad_T_surface", d_grad_T_surface}, {"grad_T", d_grad_T}}, err)) return;
  TRY
  settle_device_batch(r);
  wait_for_producer(r, producer_stream);
  ir_rows_vjp_enqueue(r, *ncol, *nsel_, d_T_surface, d_T, w, gs, gn, d_grad_T_surface, d_grad_T);
  CATCH(err)
}

// The host cotangents gs / gn ([up, down], `spec` / `sums` doubles per column, null where absent) of the nc columns from c0
// on, up into d_rows_out back to back (the caller has reserved it); dgs / dgn: where each lies on the device
static void ir_stage_cotangents(Radtran *r, size_t spec, size_t sums, int c0, int nc, const double *const gs[2], const double *const gn[2],
                                const double *dgs[2], const double *dgn[2]) {
  double *at = r->d_rows_out.p;
  for (int d = 0; d < 2; d++) {
    dgs[d] = dgn[d] = nullptr;
    if (gs[d]) {
      if (spec) HIPCHK(hipMemcpyAsync(at, gs[d] + spec * c0, sizeof(double) * spec * nc, hipMemcpyHostToDevice, r->stream));
      dgs[d] = at; at += spec * nc;
    }
    if (gn[d]) {
      HIPCHK(hipMemcpyAsync(at, gn[d] + sums * c0, sizeof(double) * sums * nc, hipMemcpyHostToDevice, r->stream));
      dgn[d] = at; at += sums * nc;
    }
  }
}
// ... with host arrays, synchronous: T and the weights go up whole, the cotangents and the gradient in chunks of columns
// bounded like the batch's, the gradient back through the pinned block
void radtran_ir_spectra_batch_vjp(void *ptr, const int *ncol, const double *T_surface, const int *dim1_T, const int *dim2_T,
                                  const double *T, const int *nsel_, const double *w_up, const double *w_dn, const double *g_ir_fup,
                                  const double *g_ir_fdn, const double *g_fup_n, const double *g_fdn_n, double *grad_T_surface,
                                  double *grad_T, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const std::string pre = "ir_spectra_batch_vjp: ";
  const int nz = r->nz, nl = nz + 1, nw_ir = r->ir.nw, n = *ncol, nsel = *nsel_;
  const double *const w[2] = {w_up, w_dn}, *const gs[2] = {g_ir_fup, g_ir_fdn}, *const gn[2] = {g_fup_n, g_fdn_n};
  if (ir_rows_vjp_refused(r, pre, n, *dim1_T, *dim2_T, nsel, T_surface, T, w, gs, gn, grad_T_surface, grad_T, err)) return;
  if (ir_batch_T_refused(pre, nz, n, T_surface, T, err)) return;
  TRY
  settle_device_batch(r);
  bool use[2];
  int ndir = 0;
  for (int d = 0; d < 2; d++) { use[d] = gs[d] || gn[d]; ndir += use[d] ? 1 : 0; }
  const size_t arr_w = (size_t)nw_ir * nsel * nl, spec = (size_t)nw_ir * nsel, sums = (size_t)nsel;
  r->d_rows_w.reserve(std::max<size_t>(1, ndir * arr_w));
  r->d_bT.reserve((size_t)n * nz); r->d_bTs.reserve(n);
  HIPCHK(hipMemcpyAsync(r->d_bT.p, T, sizeof(double) * (size_t)n * nz, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipMemcpyAsync(r->d_bTs.p, T_surface, sizeof(double) * n, hipMemcpyHostToDevice, r->stream));
  const double *dw[2] = {nullptr, nullptr};
  {
    double *at = r->d_rows_w.p;
    for (int d = 0; d < 2; d++) {
      if (!use[d]) continue;
      if (arr_w) HIPCHK(hipMemcpyAsync(at, w[d], sizeof(double) * arr_w, hipMemcpyHostToDevice, r->stream));
      dw[d] = at; at += arr_w;
    }
  }
  const int CH = ir_rows_chunk(n, ndir, spec);
  r->d_rows_out.reserve(std::max<size_t>(1, (size_t)ndir * (spec + sums) * CH));
  r->d_bout.reserve((size_t)nl * CH);
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int nc = std::min(CH, n - c0);
    const double *dgs[2], *dgn[2];
    ir_stage_cotangents(r, spec, sums, c0, nc, gs, gn, dgs, dgn);
    double *const d_gT = r->d_bout.p, *const d_gTs = d_gT + (size_t)nz * nc;
    ir_rows_vjp_enqueue(r, nc, nsel, r->d_bTs.p + c0, r->d_bT.p + (size_t)c0 * nz, dw, dgs, dgn, d_gTs, d_gT);
    rows_to_host(r, d_gT, grad_T + (size_t)c0 * nz, (size_t)nz * nc);
    rows_to_host(r, d_gTs, grad_T_surface + c0, nc);
  }
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

// Gradient of a loss on one column's IR spectra (and their sums over the bins) in the stored tau, w0, g: one adjoint and one
// forward two-stream solve per (bin, g-point) on the stored opacities (ir_opr_sens.inc).  include/clima_radtran_hip.h has
// the contract.  What both forms refuse, in the header's order; `lv`: the levels TOA-first.  false: the call can run
static bool ir_opr_refused(Radtran *r, const char *who, int dim_T, int nsel, const int *spec_level, const void *T_surface, const void *T,
                           const double *const gs[2], const double *const gn[2], double *const out[3], std::vector<int> &lv, char *err) {
  const std::string pre = std::string(who) + ": ";
  const int nz = r->nz;
  if (dim_T != nz) { set_err(err, pre + "\"T\" has the dimension " + std::to_string(dim_T) + ", not nz = " + std::to_string(nz)); return true; }
  if (nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(nsel) + ")"); return true; }
  if (!spec_level) { set_err(err, pre + "\"spec_level\" is a required argument"); return true; }
  if (ir_levels_refused(pre, "spec_level", nz, nsel, spec_level, lv, err)) return true;
  if (!gs[0] && !gs[1] && !gn[0] && !gn[1]) { set_err(err, pre + "none of g_ir_fup, g_ir_fdn, g_fup_n, g_fdn_n was given"); return true; }
  if (!out[0] && !out[1] && !out[2]) { set_err(err, pre + "none of grad_tau, grad_w0, grad_g was given"); return true; }
  if (!T) { set_err(err, pre + "\"T\" is a required argument"); return true; }
  if (!T_surface) { set_err(err, pre + "\"T_surface\" is a required argument"); return true; }
  return false;
}
// ... and of the handle, once the arguments stand: a bin shard or a communicator, no opacities, the work buffer's bound
static bool ir_opr_handle_refused(Radtran *r, const char *who, char *err) {
  const std::string pre = std::string(who) + ": ";
  if (ir_rows_shard_refused(r, pre, err)) return true;
  if (refuse(r, who, NEED_OPACITIES, err)) return true;
  const int NQ = r->ir_n * r->ng;
  const size_t n_work = ir_opr_work_count(r->nz, NQ), n_part = ir_opr_part_count(r->nz, NQ);
  if (sizeof(double) * ((double)n_work + (double)n_part) > IR_ADJOINT_MAX_BYTES) {
    set_err(err, pre + "the work buffer of " + std::to_string(NQ) + " (bin, g-point) pairs of nz = " + std::to_string(r->nz) + " layers would take " +
                     std::to_string(sizeof(double) * (n_work + n_part)) + " bytes, more than " + std::to_string((long long)IR_ADJOINT_MAX_BYTES));
    return true;
  }
  return false;
}
// The pass itself: device arrays in, device arrays out (each of `out` the whole array of radtran_opr_get's layout, or null),
// enqueued on the handle's stream behind ready_stored_opacities.  The bins outside the IR channel are zeroed here.
static void ir_opr_enqueue(Radtran *r, const std::vector<int> &lv, const double *d_Ts, const double *d_T, const double *const gs[2],
                           const double *const gn[2], double *const out[3]) {
  const int nz = r->nz, nsel = (int)lv.size(), NQ = r->ir_n * r->ng;
  const size_t counts[3] = {r->d_tau.n, r->d_tau.n, r->d_g.n};
  for (int k = 0; k < 3; k++)
    if (out[k]) HIPCHK(hipMemsetAsync(out[k], 0, sizeof(double) * counts[k], r->stream));
  if (r->ir_n < 1) return;
  const size_t n_work = ir_opr_work_count(nz, NQ), n_part = ir_opr_part_count(nz, NQ);
  r->d_adjoint.reserve(n_work + n_part);
  IrOprParams p;
  std::memset(&p, 0, sizeof(p));
  p.g = green_params(r);
  p.T = d_T; p.Ts = d_Ts; p.bplanck = nullptr;
  p.nsel = nsel; p.gs_ld = r->ir.nw; p.level = ir_upload_indices(r, lv, true);   // (the device form only enqueues; the host form goes the same way)
  p.gs_up = gs[0]; p.gs_dn = gs[1]; p.gn_up = gn[0]; p.gn_dn = gn[1];
  p.work = r->d_adjoint.p; p.part_g = p.work + n_work;
  p.grad_tau = out[0]; p.grad_w0 = out[1]; p.grad_g = out[2];
  launch_ir_opr_sens(p, r->stream);
  HIPCHK(hipGetLastError());
}

void radtran_ir_spectra_opr_vjp_device(void *ptr, const double *d_T_surface, const int *dim_T, const double *d_T, const int *nsel_,
                                       const int *spec_level, const double *d_g_ir_fup, const double *d_g_ir_fdn, const double *d_g_fup_n,
                                       const double *d_g_fdn_n, double *d_grad_tau, double *d_grad_w0, double *d_grad_g,
                                       const void *producer_stream, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const char *who = "ir_spectra_opr_vjp_device";
  const double *const gs[2] = {d_g_ir_fup, d_g_ir_fdn}, *const gn[2] = {d_g_fup_n, d_g_fdn_n};
  double *const out[3] = {d_grad_tau, d_grad_w0, d_grad_g};
  std::vector<int> lv;
  if (ir_opr_refused(r, who, *dim_T, *nsel_, spec_level, d_T_surface, d_T, gs, gn, out, lv, err)) return;
  if (ir_rows_not_device(r, std::string(who) + ": ", {{"T_surface", d_T_surface}, {"T", d_T}, {"g_ir_fup", d_g_ir_fup}, {"g_ir_fdn", d_g_ir_fdn},
                                                      {"g_fup_n", d_g_fup_n}, {"g_fdn_n", d_g_fdn_n}, {"grad_tau", d_grad_tau},
                                                      {"grad_w0", d_grad_w0}, {"grad_g", d_grad_g}}, err)) return;
  if (ir_opr_handle_refused(r, who, err)) return;
  TRY
  ready_stored_opacities(r);
  wait_for_producer(r, producer_stream);
  ir_opr_enqueue(r, lv, d_T_surface, d_T, gs, gn, out);
  CATCH(err)
}

// ... with host arrays, synchronous: the column and the cotangents go up, the gradients come back through the pinned block
void radtran_ir_spectra_opr_vjp(void *ptr, const double *T_surface, const int *dim_T, const double *T, const int *nsel_,
                                const int *spec_level, const double *g_ir_fup, const double *g_ir_fdn, const double *g_fup_n,
                                const double *g_fdn_n, double *grad_tau, double *grad_w0, double *grad_g, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const char *who = "ir_spectra_opr_vjp";
  const std::string pre = std::string(who) + ": ";
  const double *const gs[2] = {g_ir_fup, g_ir_fdn}, *const gn[2] = {g_fup_n, g_fdn_n};
  double *const out[3] = {grad_tau, grad_w0, grad_g};
  std::vector<int> lv;
  if (ir_opr_refused(r, who, *dim_T, *nsel_, spec_level, T_surface, T, gs, gn, out, lv, err)) return;
  const int nz = r->nz, nsel = *nsel_;
  if (ir_column_T_refused(pre, nz, T_surface, T, err)) return;
  if (ir_opr_handle_refused(r, who, err)) return;
  TRY
  ready_stored_opacities(r);
  const size_t spec = (size_t)r->ir.nw * nsel, sums = (size_t)nsel;
  const size_t counts[3] = {r->d_tau.n, r->d_tau.n, r->d_g.n};
  r->d_bT.reserve(nz); r->d_bTs.reserve(1);
  HIPCHK(hipMemcpyAsync(r->d_bT.p, T, sizeof(double) * nz, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipMemcpyAsync(r->d_bTs.p, T_surface, sizeof(double), hipMemcpyHostToDevice, r->stream));
  r->d_rows_out.reserve(std::max<size_t>(1, 2 * (spec + sums)));
  const double *dgs[2], *dgn[2];
  ir_stage_cotangents(r, spec, sums, 0, 1, gs, gn, dgs, dgn);
  size_t total = 0;
  for (int k = 0; k < 3; k++) total += out[k] ? counts[k] : 0;
  r->d_bout.reserve(total);
  double *d_out[3] = {nullptr, nullptr, nullptr};
  {
    double *at = r->d_bout.p;
    for (int k = 0; k < 3; k++)
      if (out[k]) { d_out[k] = at; at += counts[k]; }
  }
  ir_opr_enqueue(r, lv, r->d_bTs.p, r->d_bT.p, dgs, dgn, d_out);
  for (int k = 0; k < 3; k++)
    if (out[k]) rows_to_host(r, d_out[k], out[k], counts[k]);
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

// Gradient of a loss on the solar spectra (fup, fdn, amean and the sums of fup, fdn over the bins) in the stored tau, w0, g
// and in the surface albedo, under the handle's zenith angles, albedo and scale factors: one adjoint and one forward
// two-stream solve per (bin, g-point) on the stored opacities (sol_opr_sens.inc).  include/clima_radtran_hip.h has the
// contract.  What both forms refuse of their arguments; `lv`: the levels TOA-first.  false: the call can run
static bool sol_opr_refused(Radtran *r, const char *who, int nsel, const int *spec_level, const double *const gs[3],
                            const double *const gn[2], double *const out[4], std::vector<int> &lv, char *err) {
  const std::string pre = std::string(who) + ": ";
  if (nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(nsel) + ")"); return true; }
  if (!spec_level) { set_err(err, pre + "\"spec_level\" is a required argument"); return true; }
  if (ir_levels_refused(pre, "spec_level", r->nz, nsel, spec_level, lv, err)) return true;
  if (!gs[0] && !gs[1] && !gs[2] && !gn[0] && !gn[1]) {
    set_err(err, pre + "none of g_sol_fup, g_sol_fdn, g_sol_amean, g_fup_n, g_fdn_n was given");
    return true;
  }
  if (!out[0] && !out[1] && !out[2] && !out[3]) { set_err(err, pre + "none of grad_tau, grad_w0, grad_g, grad_albedo was given"); return true; }
  return false;
}
// ... and of the handle, once the arguments stand: a bin shard or a communicator, no solar bins (a property of the handle,
// so before what it holds), no opacities, the work buffer's bound
static bool sol_opr_handle_refused(Radtran *r, const char *who, char *err) {
  const std::string pre = std::string(who) + ": ";
  if (ir_rows_shard_refused(r, pre, err)) return true;
  if (r->sol.nw < 1 || r->sol_n < 1) { set_err(err, pre + "the handle has no solar bins (nw_sol = " + std::to_string(r->sol.nw) + ")"); return true; }
  if (refuse(r, who, NEED_OPACITIES, err)) return true;
  const int nzen = (int)r->zenith_u.size();
  if (nzen < 1) { set_err(err, pre + "the handle has no zenith angle (nzen = " + std::to_string(nzen) + ")"); return true; }
  const int NQ = r->sol_n * r->ng;
  const size_t n_work = sol_opr_work_count(r->nz, NQ), n_part = sol_opr_part_count(r->nz, NQ);
  if (sizeof(double) * ((double)n_work + (double)n_part) > IR_ADJOINT_MAX_BYTES) {
    set_err(err, pre + "the work buffer of " + std::to_string(NQ) + " (bin, g-point) pairs of nz = " + std::to_string(r->nz) + " layers would take " +
                     std::to_string(sizeof(double) * (n_work + n_part)) + " bytes, more than " + std::to_string((long long)IR_ADJOINT_MAX_BYTES));
    return true;
  }
  return false;
}
// doubles of the four outputs: grad_tau, grad_w0, grad_g (radtran_opr_get's layout), grad_albedo (nw_sol)
static void sol_opr_counts(Radtran *r, size_t counts[4]) {
  counts[0] = r->d_tau.n; counts[1] = r->d_tau.n; counts[2] = r->d_g.n; counts[3] = (size_t)r->sol.nw;
}
// The pass itself: device arrays in, device arrays out (each of `out` the whole array, or null), enqueued on the handle's
// stream behind ready_stored_opacities.  The bins outside the solar channel are zeroed here.
static void sol_opr_enqueue(Radtran *r, const std::vector<int> &lv, const double *const gs[3], const double *const gn[2],
                            double *const out[4]) {
  const int nz = r->nz, nsel = (int)lv.size(), NQ = r->sol_n * r->ng;
  size_t counts[4];
  sol_opr_counts(r, counts);
  for (int k = 0; k < 4; k++)
    if (out[k]) HIPCHK(hipMemsetAsync(out[k], 0, sizeof(double) * counts[k], r->stream));
  const size_t n_work = sol_opr_work_count(nz, NQ), n_part = sol_opr_part_count(nz, NQ);
  r->d_adjoint.reserve(n_work + n_part);
  SolOprParams p;
  std::memset(&p, 0, sizeof(p));
  p.nz = nz; p.ng = r->ng; p.n_sol = r->sol_n; p.sol_lo = r->sol_lo; p.sol_start = r->sol.ind_start; p.NQ = NQ;
  p.nzen = (int)r->zenith_u.size();
  p.tau = r->d_tau.p; p.w0 = r->d_w0.p; p.g = r->d_g.p; p.wbin = r->d_wbin.p;
  p.zen_u = r->d_zen_u.p; p.zen_w = r->d_zen_w.p; p.zen_iu = r->d_zen_iu.p;
  p.albedo = r->d_albedo.p; p.photons_sol = r->d_photons.p;
  p.am_f1 = r->d_am_f1.p; p.am_f2 = r->d_am_f2.p; p.am_dw = r->d_am_dw.p;
  p.scale = r->photon_scale_factor * r->diurnal_fac;
  p.sol_freq = r->sol.d_freq.p;
  p.nsel = nsel; p.gs_ld = r->sol.nw; p.level = ir_upload_indices(r, lv, true);
  p.gs_up = gs[0]; p.gs_dn = gs[1]; p.gs_am = gs[2]; p.gn_up = gn[0]; p.gn_dn = gn[1];
  p.work = r->d_adjoint.p; p.part_g = p.work + n_work; p.part_alb = p.part_g + (size_t)NQ * nz;
  p.grad_tau = out[0]; p.grad_w0 = out[1]; p.grad_g = out[2]; p.grad_albedo = out[3];
  launch_sol_opr_sens(p, r->stream);
  HIPCHK(hipGetLastError());
}

void radtran_sol_spectra_opr_vjp_device(void *ptr, const int *nsel_, const int *spec_level, const double *d_g_sol_fup,
                                        const double *d_g_sol_fdn, const double *d_g_sol_amean, const double *d_g_fup_n,
                                        const double *d_g_fdn_n, double *d_grad_tau, double *d_grad_w0, double *d_grad_g,
                                        double *d_grad_albedo, const void *producer_stream, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const char *who = "sol_spectra_opr_vjp_device";
  const double *const gs[3] = {d_g_sol_fup, d_g_sol_fdn, d_g_sol_amean}, *const gn[2] = {d_g_fup_n, d_g_fdn_n};
  double *const out[4] = {d_grad_tau, d_grad_w0, d_grad_g, d_grad_albedo};
  std::vector<int> lv;
  if (sol_opr_refused(r, who, *nsel_, spec_level, gs, gn, out, lv, err)) return;
  if (ir_rows_not_device(r, std::string(who) + ": ", {{"g_sol_fup", d_g_sol_fup}, {"g_sol_fdn", d_g_sol_fdn}, {"g_sol_amean", d_g_sol_amean},
                                                      {"g_fup_n", d_g_fup_n}, {"g_fdn_n", d_g_fdn_n}, {"grad_tau", d_grad_tau},
                                                      {"grad_w0", d_grad_w0}, {"grad_g", d_grad_g}, {"grad_albedo", d_grad_albedo}}, err)) return;
  if (sol_opr_handle_refused(r, who, err)) return;
  TRY
  ready_stored_opacities(r);
  wait_for_producer(r, producer_stream);
  sol_opr_enqueue(r, lv, gs, gn, out);
  CATCH(err)
}

// ... with host arrays, synchronous: the cotangents go up, the gradients come back through the pinned block
void radtran_sol_spectra_opr_vjp(void *ptr, const int *nsel_, const int *spec_level, const double *g_sol_fup, const double *g_sol_fdn,
                                 const double *g_sol_amean, const double *g_fup_n, const double *g_fdn_n, double *grad_tau,
                                 double *grad_w0, double *grad_g, double *grad_albedo, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const char *who = "sol_spectra_opr_vjp";
  const double *const gs[3] = {g_sol_fup, g_sol_fdn, g_sol_amean}, *const gn[2] = {g_fup_n, g_fdn_n};
  double *const out[4] = {grad_tau, grad_w0, grad_g, grad_albedo};
  std::vector<int> lv;
  if (sol_opr_refused(r, who, *nsel_, spec_level, gs, gn, out, lv, err)) return;
  if (sol_opr_handle_refused(r, who, err)) return;
  TRY
  ready_stored_opacities(r);
  const int nsel = *nsel_;
  const size_t spec = (size_t)r->sol.nw * nsel, sums = (size_t)nsel;
  r->d_rows_out.reserve(std::max<size_t>(1, 3 * spec + 2 * sums));
  const double *dgs[3] = {nullptr, nullptr, nullptr}, *dgn[2] = {nullptr, nullptr};
  {
    double *at = r->d_rows_out.p;
    for (int k = 0; k < 3; k++)
      if (gs[k]) {
        HIPCHK(hipMemcpyAsync(at, gs[k], sizeof(double) * spec, hipMemcpyHostToDevice, r->stream));
        dgs[k] = at; at += spec;
      }
    for (int k = 0; k < 2; k++)
      if (gn[k]) {
        HIPCHK(hipMemcpyAsync(at, gn[k], sizeof(double) * sums, hipMemcpyHostToDevice, r->stream));
        dgn[k] = at; at += sums;
      }
  }
  size_t counts[4], total = 0;
  sol_opr_counts(r, counts);
  for (int k = 0; k < 4; k++) total += out[k] ? counts[k] : 0;
  r->d_bout.reserve(total);
  double *d_out[4] = {nullptr, nullptr, nullptr, nullptr};
  {
    double *at = r->d_bout.p;
    for (int k = 0; k < 4; k++)
      if (out[k]) { d_out[k] = at; at += counts[k]; }
  }
  sol_opr_enqueue(r, lv, dgs, dgn, d_out);
  for (int k = 0; k < 4; k++)
    if (out[k]) rows_to_host(r, d_out[k], out[k], counts[k]);
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

// What every column batch refuses before anything else, with the texts of radtran_toa_fluxes_batch
static bool batch_refused(Radtran *r, const int *ncol, const int *has_particles, char *err) {
  if (*ncol < 1) { set_err(err, "\"T\" has the wrong input dimension."); return true; }
  if (refuse(r, "toa_fluxes_batch", NEED_SPECTRUM, err, /*comm_counts=*/false)) return true;
  const int hp = has_particles ? *has_particles : 0;
  if (r->np > 0 && !hp) { set_err(err, "\"pdensities\" and \"radii\" are required arguments."); return true; }
  return false;
}
// The per-bin rows a spectra batch asks for: levels 1..nz+1 ground-first (row_level's convention in
// radtran_ir_jacobian_reduced), any order, repeats allowed; out = ir_fup, ir_fdn, sol_fup, sol_fdn, each (nw, nsel, ncol)
// or NULL.
struct SpectraAsk { int nsel; const int *level; double *out[4]; };
constexpr const char *SPECTRA_NAMES[4] = {"ir_fup", "ir_fdn", "sol_fup", "sol_fdn"};
static bool spectra_refused(Radtran *r, const SpectraAsk &ask, char *err) {
  const std::string pre = "toa_fluxes_batch_spectra: ";
  const int nl = r->nz + 1;
  if (ask.nsel < 1) { set_err(err, pre + "nsel must be at least 1 (nsel = " + std::to_string(ask.nsel) + ")"); return true; }
  if (!ask.level) { set_err(err, pre + "\"spec_level\" is a required argument"); return true; }
  for (int a = 0; a < ask.nsel; a++) {
    const int v = ask.level[a];
    if (v < 1 || v > nl) {
      set_err(err, pre + "spec_level(" + std::to_string(a + 1) + ") = " + std::to_string(v) + " is outside 1.." + std::to_string(nl));
      return true;
    }
  }
  if (!ask.out[0] && !ask.out[1] && !ask.out[2] && !ask.out[3]) {
    set_err(err, pre + "none of ir_fup, ir_fdn, sol_fup, sol_fdn was given (radtran_toa_fluxes_batch is the call without spectra)");
    return true;
  }
  return false;
}
// The sinks of `ask` into the run, behind begin_batch (an earlier batch is settled by then: the copy of its list out of
// the handle's vector is done, and so are its gathers): the level list, 0-based, to the device, once; `to_host`: the
// destinations are slices of the staging buffer, in the order of the arrays given (out_spectra takes them apart the
// same way)
static void stage_spectra(Radtran *r, BatchRun &run, const SpectraAsk &ask, bool to_host) {
  run.nsel = ask.nsel;
  r->spec_level.resize(ask.nsel);
  for (int a = 0; a < ask.nsel; a++) r->spec_level[a] = ask.level[a] - 1;
  r->d_spec_level.reserve(ask.nsel);
  HIPCHK(hipMemcpyAsync(r->d_spec_level.p, r->spec_level.data(), sizeof(int) * ask.nsel, hipMemcpyHostToDevice, r->stream));
  run.spec_level = r->d_spec_level.p;
  if (!to_host) { for (int k = 0; k < 4; k++) run.spec[k] = ask.out[k]; return; }
  size_t off[4], total = 0;
  for (int k = 0; k < 4; k++) {
    off[k] = total;
    if (ask.out[k]) total += (size_t)(k < 2 ? r->ir.nw : r->sol.nw) * ask.nsel * run.n;
  }
  r->d_spec_stage.reserve(total);
  for (int k = 0; k < 4; k++) run.spec[k] = ask.out[k] ? r->d_spec_stage.p + off[k] : nullptr;
  run.spec_host = r->h_spec.reserve(total);
  run.spec_count = total;
}
static void out_spectra(Radtran *r, const BatchRun &run, const SpectraAsk &ask) {
  size_t off = 0;
  for (int k = 0; k < 4; k++) {
    if (!ask.out[k]) continue;
    const size_t cnt = (size_t)(k < 2 ? r->ir.nw : r->sol.nw) * ask.nsel * run.n;
    std::memcpy(ask.out[k], run.spec_host + off, sizeof(double) * cnt);
    off += cnt;
  }
}

// Config 4 of BASELINE.json (many independent columns): every column is one full
// Radtran%TOA_fluxes (clima_radtran.f90:320-342), but the batch is moved to HBM in one copy, the
// calls are enqueued back to back with no host round trip between them, and the level fluxes
// come back in one copy.  Arrays carry the column as their LAST (slowest) dimension:
// T, P, dz (nz, ncol); densities (nz, nsp, ncol); pdensities, radii (nz, np, ncol).
// Outputs: ISR, OLR (ncol); fluxes (nz+1, 5, ncol) = ir up, ir down, solar up, solar down, f_total,
// or NULL.  The handle's own wrk / f_total hold the last column afterwards.
// bnd: a bounds batch (radtran_toa_fluxes_batch_bounds) -- the columns' bounds blocks are built here beside the column
// blocks and go up in the same copy.
static void toa_fluxes_batch_host(void *ptr, const int *ncol, const ColumnArrays &in, const int *has_particles, double *ISR,
                                  double *OLR, double *fluxes, const SpectraAsk *ask, const BoundsArrays *bnd, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (batch_refused(r, ncol, has_particles, err)) return;
  if (ask && spectra_refused(r, *ask, err)) return;
  TRY
  const int n = *ncol;
  const size_t cc = r->col_layout.count;
  const LevelRows &l = r->rows;
  begin_batch(r, n, false, bnd != nullptr);
  std::vector<double> h((size_t)n * (cc + (bnd ? handle_bounds_layout(r).count : 0)), 0.0), out(n * l.stride);
  r->batch_nsrc.resize(n);
  for (int c = 0; c < n; c++) r->batch_nsrc[c] = pack_column(r, h.data() + (size_t)c * cc, in.column(c, r->nz, r->nsp, r->np));
  if (bnd) pack_bounds(r, n, *bnd, h.data() + (size_t)n * cc);
  HIPCHK(hipMemcpyAsync(r->d_cols_arena.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, r->stream));
  BatchRun run = batch_form(r, n);
  run.rows = out.data();
  if (bnd) { run.bounds = batch_bounds_base(r, n); run.bounds_count = handle_bounds_layout(r).count; }
  if (ask) stage_spectra(r, run, *ask, true);
  enqueue_batch(r, run, true);
  batch_leaves_handle(r, run);
  if (settle_batch(r, run)) { set_err(err, OPACITY_FAILED_MSG); return; }
  for (int c = 0; c < n; c++) {
    double *f = out.data() + c * l.stride;
    f_total_row(f, l);
    toa_fluxes(f, l, &ISR[c], &OLR[c]);
    if (fluxes) std::memcpy(fluxes + c * l.stride, f, sizeof(double) * l.stride);
  }
  if (ask) out_spectra(r, run, *ask);
  CATCH(err)
}
void radtran_toa_fluxes_batch(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                              const double *densities, const double *dz, const int *has_particles,
                              const double *pdensities, const double *radii, double *ISR, double *OLR,
                              double *fluxes, char *err) {
  toa_fluxes_batch_host(ptr, ncol, ColumnArrays{T_surface, T, P, densities, dz, pdensities, radii}, has_particles, ISR, OLR, fluxes, nullptr, nullptr, err);
}
// ... and with the per-bin rows `spec_level` of every column: what a batch otherwise keeps of the last column only.
// Copies of the values the batch's own integration sums (k_batch_spectra behind each chunk, enqueue_batch).
void radtran_toa_fluxes_batch_spectra(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                      const double *densities, const double *dz, const int *has_particles,
                                      const double *pdensities, const double *radii, double *ISR, double *OLR,
                                      double *fluxes, const int *nsel, const int *spec_level, double *ir_fup,
                                      double *ir_fdn, double *sol_fup, double *sol_fdn, char *err) {
  const SpectraAsk ask{nsel ? *nsel : 0, spec_level, {ir_fup, ir_fdn, sol_fup, sol_fdn}};
  toa_fluxes_batch_host(ptr, ncol, ColumnArrays{T_surface, T, P, densities, dz, pdensities, radii}, has_particles, ISR, OLR, fluxes, &ask, nullptr, err);
}
// ... and with per-column surface albedo, surface emissivity, zenith angles and photon scale factor (the header states
// the contract): the spectra batch with five optional arrays; nsel = 0: no spectra
void radtran_toa_fluxes_batch_bounds(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                     const double *densities, const double *dz, const int *has_particles,
                                     const double *pdensities, const double *radii, double *ISR, double *OLR,
                                     double *fluxes, const double *surface_albedo, const double *surface_emissivity,
                                     const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                                     const int *nsel, const int *spec_level, double *ir_fup, double *ir_fdn,
                                     double *sol_fup, double *sol_fdn, char *err) {
  const SpectraAsk ask{nsel ? *nsel : 0, spec_level, {ir_fup, ir_fdn, sol_fup, sol_fdn}};
  const BoundsArrays bnd{surface_albedo, surface_emissivity, zenith_u, zenith_weights, photon_scale_factor};
  toa_fluxes_batch_host(ptr, ncol, ColumnArrays{T_surface, T, P, densities, dz, pdensities, radii}, has_particles, ISR, OLR, fluxes,
                        ask.nsel != 0 ? &ask : nullptr, &bnd, err);
}

// The same batch with every array in device memory (the f64 tensors of a GPU-resident ensemble): the column blocks
// are built on the device (k_pack_columns), the chunks run as in the host batch, f_total / ISR / OLR are formed and
// stored on the device (k_batch_finish).  The call returns with the work enqueued on the handle's stream, behind the
// caller's writes of the inputs on `producer_stream` (NULL: they are complete); the results are final when the next
// radtran_synchronize returns with `err` empty (settle_device_batch).  The host stages nothing and waits for
// nothing -- but for a configuration that runs one call per column (the fused grid does not cover it, or
// CLIMA_HIP_BATCH_ONE_LAUNCH=0): plan_radiate picks the opacity kernel and sizes the grids of such a call from the
// column's own source-layer count, and the kernels it chooses between round differently, so the bound nsrc = nz
// would not be the host batch's computation; the ncol counts (4 bytes each) are fetched in one copy first.
// bnd: a bounds batch (radtran_toa_fluxes_batch_bounds_device) -- k_pack_bounds builds the columns' bounds blocks.
static void toa_fluxes_batch_dev(void *ptr, const int *ncol, const ColumnArrays &in, const int *has_particles, double *d_ISR,
                                 double *d_OLR, double *d_fluxes, const SpectraAsk *ask, const BoundsArrays *bnd,
                                 const void *producer_stream, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (batch_refused(r, ncol, has_particles, err)) return;
  TRY
  const bool part = r->np > 0;
  enum { UNUSED, REQUIRED, OPTIONAL };   // (the particle arrays of a handle without particle columns are not read)
  const struct { const char *name; const void *p; int use; } args[] = {
      {"T_surface", in.T_surface, REQUIRED}, {"T", in.T, REQUIRED}, {"P", in.P, REQUIRED}, {"densities", in.dens, REQUIRED},
      {"dz", in.dz, REQUIRED}, {"pdensities", in.pdens, part ? REQUIRED : UNUSED}, {"radii", in.radii, part ? REQUIRED : UNUSED},
      {"ISR", d_ISR, REQUIRED}, {"OLR", d_OLR, REQUIRED}, {"fluxes", d_fluxes, OPTIONAL},
      {"surface_albedo", bnd ? bnd->albedo : nullptr, OPTIONAL}, {"surface_emissivity", bnd ? bnd->emissivity : nullptr, OPTIONAL},
      {"zenith_u", bnd ? bnd->zenith_u : nullptr, OPTIONAL}, {"zenith_weights", bnd ? bnd->zenith_w : nullptr, OPTIONAL},
      {"photon_scale_factor", bnd ? bnd->scale : nullptr, OPTIONAL}};
  for (const auto &a : args) {
    if (a.use == UNUSED || (a.use == OPTIONAL && !a.p)) continue;
    if (!a.p) { set_err(err, std::string("toa_fluxes_batch_device: \"") + a.name + "\" is a required argument"); return; }
    if (!on_handle_device(r, a.p)) {
      set_err(err, std::string("toa_fluxes_batch_device: \"") + a.name + "\" is not device memory of this handle's device");
      return;
    }
  }
  if (ask) {
    if (spectra_refused(r, *ask, err)) return;
    for (int k = 0; k < 4; k++)
      if (ask->out[k] && !on_handle_device(r, ask->out[k])) {
        set_err(err, std::string("toa_fluxes_batch_device: \"") + SPECTRA_NAMES[k] + "\" is not device memory of this handle's device");
        return;
      }
  }
  const int n = *ncol;
  begin_batch(r, n, true, bnd != nullptr);
  if (producer_stream) {
    if (!r->ev_producer) HIPCHK(hipEventCreateWithFlags(&r->ev_producer, hipEventDisableTiming));
    HIPCHK(hipEventRecord(r->ev_producer, reinterpret_cast<hipStream_t>(const_cast<void *>(producer_stream))));
    HIPCHK(hipStreamWaitEvent(r->stream, r->ev_producer, 0));
  }
  launch_pack_columns(make_pack_params(r, n, in, r->d_cols_arena.p, r->d_batch_nsrc.p), r->stream);
  HIPCHK(hipGetLastError());
  if (bnd) {
    upload_fields(r);   // (an array not given is filled from the handle's device copy of the field)
    launch_pack_bounds(make_pack_bounds_params(r, n, *bnd, batch_bounds_base(r, n)), r->stream);
    HIPCHK(hipGetLastError());
  }
  BatchRun run = batch_form(r, n);
  if (bnd) { run.bounds = batch_bounds_base(r, n); run.bounds_count = handle_bounds_layout(r).count; }
  run.ISR = d_ISR; run.OLR = d_OLR; run.fluxes = d_fluxes;
  if (ask) stage_spectra(r, run, *ask, false);
  if (!run.one_launch) fetch_batch_nsrc(r, n);
  enqueue_batch(r, run, true);
  batch_leaves_handle(r, run);
  run.pending = true;
  r->dev_batch = run;
  CATCH(err)
}
void radtran_toa_fluxes_batch_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                     const double *d_P, const double *d_densities, const double *d_dz,
                                     const int *has_particles, const double *d_pdensities, const double *d_radii,
                                     double *d_ISR, double *d_OLR, double *d_fluxes, const void *producer_stream,
                                     char *err) {
  toa_fluxes_batch_dev(ptr, ncol, ColumnArrays{d_T_surface, d_T, d_P, d_densities, d_dz, d_pdensities, d_radii}, has_particles,
                       d_ISR, d_OLR, d_fluxes, nullptr, nullptr, producer_stream, err);
}
// ... and with the per-bin rows (device arrays; spec_level is a HOST array, read before the call returns): final, and
// after an expired hand-off wait refilled by the repeat, at the same radtran_synchronize as ISR / OLR / fluxes.
void radtran_toa_fluxes_batch_spectra_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                             const double *d_P, const double *d_densities, const double *d_dz,
                                             const int *has_particles, const double *d_pdensities, const double *d_radii,
                                             double *d_ISR, double *d_OLR, double *d_fluxes, const int *nsel,
                                             const int *spec_level, double *d_ir_fup, double *d_ir_fdn, double *d_sol_fup,
                                             double *d_sol_fdn, const void *producer_stream, char *err) {
  const SpectraAsk ask{nsel ? *nsel : 0, spec_level, {d_ir_fup, d_ir_fdn, d_sol_fup, d_sol_fdn}};
  toa_fluxes_batch_dev(ptr, ncol, ColumnArrays{d_T_surface, d_T, d_P, d_densities, d_dz, d_pdensities, d_radii}, has_particles,
                       d_ISR, d_OLR, d_fluxes, &ask, nullptr, producer_stream, err);
}
// ... and the bounds batch out of device arrays (the five bounds arrays device memory as well, or NULL)
void radtran_toa_fluxes_batch_bounds_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                            const double *d_P, const double *d_densities, const double *d_dz,
                                            const int *has_particles, const double *d_pdensities, const double *d_radii,
                                            double *d_ISR, double *d_OLR, double *d_fluxes, const double *d_surface_albedo,
                                            const double *d_surface_emissivity, const double *d_zenith_u,
                                            const double *d_zenith_weights, const double *d_photon_scale_factor,
                                            const int *nsel, const int *spec_level, double *d_ir_fup, double *d_ir_fdn,
                                            double *d_sol_fup, double *d_sol_fdn, const void *producer_stream, char *err) {
  const SpectraAsk ask{nsel ? *nsel : 0, spec_level, {d_ir_fup, d_ir_fdn, d_sol_fup, d_sol_fdn}};
  const BoundsArrays bnd{d_surface_albedo, d_surface_emissivity, d_zenith_u, d_zenith_weights, d_photon_scale_factor};
  toa_fluxes_batch_dev(ptr, ncol, ColumnArrays{d_T_surface, d_T, d_P, d_densities, d_dz, d_pdensities, d_radii}, has_particles,
                       d_ISR, d_OLR, d_fluxes, ask.nsel != 0 ? &ask : nullptr, &bnd, producer_stream, err);
}

/* test hooks: the column blocks of a batch (ncol * col_count doubles, host arrays as radtran_toa_fluxes_batch) as
 * k_pack_columns builds them on the device, and as the host's pack_column does */
static bool pack_hook_refused(Radtran *r, const int *ncol, const int *has_particles, const ColumnArrays &in, int *col_count, char *err) {
  const int hp = has_particles ? *has_particles : 0;
  if (*ncol < 1 || (r->np > 0 && !(hp && in.has_particles()))) { set_err(err, "clima_test_pack_columns: bad arguments"); return true; }
  *col_count = (int)r->col_layout.count;
  return false;
}
void clima_test_pack_columns(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                             const double *densities, const double *dz, const int *has_particles, const double *pdensities,
                             const double *radii, double *blocks, int *col_count, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (pack_hook_refused(r, ncol, has_particles, ColumnArrays{T_surface, T, P, densities, dz, pdensities, radii}, col_count, err) || !blocks) return;
  TRY
  const size_t n = *ncol, nz = r->nz;
  DevBuf<double> ts, t, p, de, z, pd, ra, out;
  DevBuf<int> ns;
  auto up = [&](DevBuf<double> &d, const double *h, size_t count) { d.upload(std::vector<double>(h, h + count)); };
  up(ts, T_surface, n); up(t, T, n * nz); up(p, P, n * nz); up(de, densities, n * nz * r->nsp); up(z, dz, n * nz);
  if (r->np > 0) { up(pd, pdensities, n * nz * r->np); up(ra, radii, n * nz * r->np); }
  out.alloc(n * r->col_layout.count);
  ns.alloc(n);
  launch_pack_columns(make_pack_params(r, (int)n, ColumnArrays{ts.p, t.p, p.p, de.p, z.p, pd.p, ra.p}, out.p, ns.p), r->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(blocks, out.p, sizeof(double) * out.n, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}
void clima_test_pack_columns_host(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                  const double *densities, const double *dz, const int *has_particles,
                                  const double *pdensities, const double *radii, double *blocks, int *col_count, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const ColumnArrays in{T_surface, T, P, densities, dz, pdensities, radii};
  if (pack_hook_refused(r, ncol, has_particles, in, col_count, err) || !blocks) return;
  std::memset(blocks, 0, sizeof(double) * (size_t)*ncol * r->col_layout.count);
  for (size_t c = 0; c < (size_t)*ncol; c++) pack_column(r, blocks + c * r->col_layout.count, in.column(c, r->nz, r->nsp, r->np));
}

/* ... and the bounds blocks of a batch (ncol * block_count doubles, host arrays as radtran_toa_fluxes_batch_bounds, any
 * of them NULL) as k_pack_bounds builds them on the device, and as the host's pack_bounds does */
void clima_test_pack_bounds(void *ptr, const int *ncol, const double *surface_albedo, const double *surface_emissivity,
                            const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                            double *blocks, int *block_count, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*ncol < 1) { set_err(err, "clima_test_pack_bounds: bad arguments"); return; }
  const BoundsLayout l = handle_bounds_layout(r);
  *block_count = (int)l.count;
  if (!blocks) return;
  TRY
  const size_t n = *ncol, nzen = r->zenith_u.size();
  DevBuf<double> al, em, zu, zw, sc, out;
  auto up = [&](DevBuf<double> &d, const double *h, size_t count) { if (h) d.upload(std::vector<double>(h, h + count)); };
  up(al, surface_albedo, n * r->sol.nw); up(em, surface_emissivity, n * r->ir.nw); up(zu, zenith_u, n * nzen);
  up(zw, zenith_weights, n * nzen); up(sc, photon_scale_factor, n);
  out.alloc(n * l.count);
  settle_device_batch(r);
  upload_fields(r);
  launch_pack_bounds(make_pack_bounds_params(r, (int)n, BoundsArrays{al.p, em.p, zu.p, zw.p, sc.p}, out.p), r->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(blocks, out.p, sizeof(double) * out.n, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}
void clima_test_pack_bounds_host(void *ptr, const int *ncol, const double *surface_albedo, const double *surface_emissivity,
                                 const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                                 double *blocks, int *block_count, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*ncol < 1) { set_err(err, "clima_test_pack_bounds: bad arguments"); return; }
  *block_count = (int)handle_bounds_layout(r).count;
  if (blocks) pack_bounds(r, *ncol, BoundsArrays{surface_albedo, surface_emissivity, zenith_u, zenith_weights, photon_scale_factor}, blocks);
}

void radtran_synchronize(void *ptr, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  TRY
  settle(r);
  if (!r->deferred_err.empty()) {   // a getter without an `err` argument met a failure since the last check
    const std::string m = r->deferred_err;
    r->deferred_err.clear();
    throw HipFail{m};
  }
  surface_device_error(r, err);
  CATCH(err)
}

void radtran_radiate_wrapper(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                             const int *dim_P, const double *P, const int *dim1_d, const int *dim2_d,
                             const double *densities, const int *dim_dz, const double *dz,
                             const int *has_particles, const int *dim1_p, const int *dim2_p,
                             const double *pdensities, const int *dim1_r, const int *dim2_r, const double *radii,
                             const int *compute_solar, const int *compute_opacity, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  const int hp = has_particles ? *has_particles : 0;
  if (!check_dims(r, *dim_T, *dim_P, *dim1_d, *dim2_d, *dim_dz, hp, dim1_p ? *dim1_p : 0, dim2_p ? *dim2_p : 0,
                  dim1_r ? *dim1_r : 0, dim2_r ? *dim2_r : 0, hp ? pdensities : nullptr, hp ? radii : nullptr, err))
    return;
  TRY
  do_upload(r, ColumnArrays{T_surface, T, P, densities, dz, hp ? pdensities : nullptr, hp ? radii : nullptr});
  enqueue_radiate(r, resident_bufs(r, /*host_out=*/true), *compute_solar != 0, *compute_opacity != 0);
  fetch_small(r);
  surface_device_error(r, err);
  CATCH(err)
}

void radtran_toa_fluxes_wrapper(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                const int *dim_P, const double *P, const int *dim1_d, const int *dim2_d,
                                const double *densities, const int *dim_dz, const double *dz,
                                const int *has_particles, const int *dim1_p, const int *dim2_p,
                                const double *pdensities, const int *dim1_r, const int *dim2_r, const double *radii,
                                const int *compute_solar, const int *compute_opacity, double *ISR, double *OLR,
                                char *err) {
  radtran_radiate_wrapper(ptr, T_surface, dim_T, T, dim_P, P, dim1_d, dim2_d, densities, dim_dz, dz,
                          has_particles, dim1_p, dim2_p, pdensities, dim1_r, dim2_r, radii, compute_solar,
                          compute_opacity, err);
  if (err && err[0]) return;
  if (Radtran *r = as_rad(ptr)) toa_fluxes(r->h_small, r->rows, ISR, OLR);
}

// Bench hook: `n` synchronous radtran_toa_fluxes_wrapper calls (host arrays in, ISR / OLR out, one stream
// synchronise each) timed one by one with the host's steady clock INSIDE the library -- the figure a Fortran or C
// caller of TOA_fluxes sees, without the ~14 us a ctypes call adds (SURVEY.md 8(d) "Metric").  us[n].
void clima_bench_toa_fluxes(void *ptr, const int *n, const double *T_surface, const int *dim_T, const double *T,
                            const int *dim_P, const double *P, const int *dim1_d, const int *dim2_d,
                            const double *densities, const int *dim_dz, const double *dz, const int *has_particles,
                            const int *dim1_p, const int *dim2_p, const double *pdensities, const int *dim1_r,
                            const int *dim2_r, const double *radii, double *us, double *ISR, double *OLR, char *err) {
  clear_err(err);
  for (int i = 0; i < *n; i++) {
    const int one = 1;
    const auto t0 = std::chrono::steady_clock::now();
    radtran_toa_fluxes_wrapper(ptr, T_surface, dim_T, T, dim_P, P, dim1_d, dim2_d, densities, dim_dz, dz, has_particles,
                               dim1_p, dim2_p, pdensities, dim1_r, dim2_r, radii, &one, &one, ISR, OLR, err);
    us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (err && err[0]) return;
  }
}

// Bench hook: `n` resident calls, each followed by its own radtran_synchronize (no PCIe for the column, one host
// round trip per call), timed one by one inside the library.  us[n].
void clima_bench_resident_sync(void *ptr, const int *n, double *us, char *err) {
  clear_err(err);
  const int one = 1;
  for (int i = 0; i < *n; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    radtran_radiate_resident(ptr, &one, &one, err);
    if (err && err[0]) return;
    radtran_synchronize(ptr, err);
    us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (err && err[0]) return;
  }
}

// Bench hook (timing only): ONE resident call's launches captured into a hipGraph, then `n` times hipGraphLaunch +
// stream synchronise, timed one by one -- what a graph would make of clima_bench_resident_sync's loop.  The replayed
// launches carry the captured call's id, so the two-stream blocks of the fused grid find their flags already set and
// do not wait: results are NOT valid (the handle is marked for a fresh call afterwards), the time is a lower bound
// (the missing wait is worth ~1 us).  With mode = 1 each pass replays `k` launches of the graph
// before it synchronises (k calls back to back).  us[n].
void clima_bench_resident_graph(void *ptr, const int *n, const int *k, double *us, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (refuse(r, "resident_graph", NEED_COLUMN, err)) return;   // (no column on a handle that is not constructed either)
  TRY
  const int one = 1;
  radtran_radiate_resident(ptr, &one, &one, err);     // steady state: buffers allocated, fields uploaded
  if (err && err[0]) return;
  settle_device_batch(r);   // (the capture holds one whole call: no integration of the call above in it)
  HIPCHK(hipStreamSynchronize(r->stream));
  // (nothing that synchronises or allocates may run inside the capture: stale fields are uploaded by the call above;
  // per-kernel event profiling records events of its own)
  if (r->fields_dirty || r->profile != 0) throw HipFail{"clima_bench_resident_graph: not with stale fields or profiling on"};
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  HIPCHK(hipStreamBeginCapture(r->stream, hipStreamCaptureModeThreadLocal));
  try {
    enqueue_radiate(r, resident_bufs(r), true, true);
  } catch (...) {
    // a failure inside the captured section must not leave the handle's stream in capture mode (every later call
    // on it would fail): close the capture, drop what was captured, pass the error on
    hipGraph_t g2 = nullptr;
    (void)hipStreamEndCapture(r->stream, &g2);
    if (g2) (void)hipGraphDestroy(g2);
    (void)hipGetLastError();
    throw;
  }
  HIPCHK(hipStreamEndCapture(r->stream, &graph));
  try {
    HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    for (int i = 0; i < 10; i++) HIPCHK(hipGraphLaunch(exec, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
    for (int i = 0; i < *n; i++) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int j = 0; j < std::max(1, *k); j++) HIPCHK(hipGraphLaunch(exec, r->stream));
      HIPCHK(hipStreamSynchronize(r->stream));
      us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
  } catch (...) {
    if (exec) (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    throw;
  }
  (void)hipGraphExecDestroy(exec);
  (void)hipGraphDestroy(graph);
  r->holds.results_dropped();
  radtran_radiate_resident(ptr, &one, &one, err);     // leave the handle with a valid call
  if (err && err[0]) return;
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

void radtran_apply_radiation_enhancement(void *ptr, const double *rad_enhancement) {
  Radtran *r = as_rad(ptr);
  if (!r || r->state != 2) return;
  try {  // clima_radtran.f90:402-411
    const LevelRows &l = r->rows;   // the two solar rows are adjacent
    settle(r);   // the results being scaled are final (a hand-off that timed out has been repaired BEFORE, not after)
    launch_scale(r->wrk_sol.fdn_a.p, r->wrk_sol.fdn_a.n, *rad_enhancement, r->stream);
    launch_scale(r->wrk_sol.fup_a.p, r->wrk_sol.fup_a.n, *rad_enhancement, r->stream);
    launch_scale(r->d_flux_n.p + l.sol_up, 2 * l.nl, *rad_enhancement, r->stream);
    // a bin-sharded handle keeps its PARTIAL solar rows for the IR-only steps that follow: they are scaled too
    if (r->shard_world > 1 && r->d_flux_part.p) launch_scale(r->d_flux_part.p + l.sol_up, 2 * l.nl, *rad_enhancement, r->stream);
    r->holds.rows_changed();   // (f_total is formed from the scaled rows when they are fetched)
    fetch_small(r);
  } catch (...) {
  }
}

void radtran_flux_device_ptr(void *ptr, void **dptr, int *count) {
  Radtran *r = as_rad(ptr);
  *dptr = r ? (void *)r->d_flux_n.p : nullptr;
  *count = r ? (int)r->rows.flux_count : 0;
  if (!r) return;
  // whoever holds the pointer reads the rows in stream order without telling the library: every call of this handle
  // integrates at once from here on, and what is pending goes out now
  r->flux_ptr_taken = true;
  try { settle_device_batch(r); } catch (const HipFail &f) { defer_err(r, f.msg); }
}

void radtran_set_bin_shard(void *ptr, const int *rank, const int *world, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*world < 1 || *rank < 0 || *rank >= *world) { set_err(err, "invalid shard (rank, world)"); return; }
  // a communicator fixes the shard (rank, nranks) -- except a one-rank communicator, on which any shard may be
  // rehearsed (one rank's share of an N-GPU step on one GPU: bench.py CLIMA_BENCH_FAKE_SHARD)
  if (r->comm && r->comm_n > 1 && (*world != r->comm_n || *rank != r->comm_rank)) {
    set_err(err, "the bin shard of a handle with a communicator is (rank, nranks) of the communicator");
    return;
  }
  TRY
  settle_device_batch(r);
  HIPCHK(hipStreamSynchronize(r->stream));
  r->shard_rank = *rank; r->shard_world = *world;
  compute_shard(r);
  // bins outside the shard hold zeros so that sharded per-bin spectra add up across ranks
  for (WrkObj *w : {&r->wrk_ir, &r->wrk_sol}) { w->fup_a.zero(r->stream); w->fdn_a.zero(r->stream); w->amean.zero(r->stream); w->tau_band.zero(r->stream); }
  r->d_flux_n.zero(r->stream);
  if (*world > 1) {
    r->d_flux_part.reserve(r->rows.flux_count);
    r->d_flux_part.zero(r->stream);
  }
  HIPCHK(hipStreamSynchronize(r->stream));
  CATCH(err)
}

// ---- the library's own multi-GPU step ---------------------------------------
// One process per GPU.  Each rank builds the same Radtran, then joins a communicator; from then on every
// radiate() / TOA_fluxes() / radiate_resident() of the handle works on the rank's own spectral bins and ends
// with one ncclAllReduce (sum, f64, 4 (nz+1) + 1 values) on the handle's stream, so that wrk_ir%fup_n ...
// f_total, ISR and OLR are those of the whole spectrum on every rank (per-bin spectra stay sharded: zeros
// outside the rank's bins).  The reduction being distributed: clima_radtran_radiate.f90:184-192.

void radtran_set_device(const int *device, char *err) {
  clear_err(err);
  TRY
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (*device < 0 || *device >= n) throw HipFail{"radtran_set_device: no such HIP device"};
  HIPCHK(hipSetDevice(*device));
  CATCH(err)
}

void radtran_comm_unique_id(char *id, char *err) {
  clear_err(err);
  TRY
  static_assert(sizeof(ncclUniqueId) == CLIMA_COMM_ID_BYTES, "CLIMA_COMM_ID_BYTES is RCCL's NCCL_UNIQUE_ID_BYTES");
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  CATCH(err)
}

static void comm_attach(Radtran *r, int nranks, int rank, const char *id) {
  if (r->comm) throw HipFail{"this handle already has a communicator"};
  settle_device_batch(r);
  HIPCHK(hipSetDevice(r->device));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  NCCLCHK(ncclCommInitRank(&r->comm, nranks, u, rank));
  r->comm_n = nranks; r->comm_rank = rank;
}

void radtran_comm_init_rank(void *ptr, const int *nranks, const int *rank, const char *id, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*nranks < 1 || *rank < 0 || *rank >= *nranks) { set_err(err, "invalid communicator (rank, nranks)"); return; }
  TRY
  comm_attach(r, *nranks, *rank, id);
  CATCH(err)
  if (err && err[0]) return;
  radtran_set_bin_shard(ptr, rank, nranks, err);
}

// The same for hosts without a message layer of their own (a plain Fortran program started once per GPU): rank 0
// writes the id to `path` (created atomically; removed again once every rank has joined), the others wait for it.
// `path` must be new for every job.
void radtran_comm_init_file(void *ptr, const int *nranks, const int *rank, const char *path, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (*nranks < 1 || *rank < 0 || *rank >= *nranks) { set_err(err, "invalid communicator (rank, nranks)"); return; }
  if (!path || !path[0]) { set_err(err, "radtran_comm_init_file: empty path"); return; }
  TRY
  char id[CLIMA_COMM_ID_BYTES];
  const std::string file(path), tmp = file + ".tmp";
  // What is published is a record, not the bare id: magic, the communicator's size and a job nonce (CLIMA_COMM_NONCE,
  // else SLURM_JOB_ID, else empty) in front of it.  A rank other than 0 joins only on a record whose size and nonce are
  // its own -- a leftover of a crashed or re-launched job on the same path (which rank 0 also removes before it
  // publishes) is not taken for this job's id, and a rank that finds nothing valid in time returns an error instead of
  // blocking in ncclCommInitRank on a dead id.  Without a nonce the file's age is the only guard (60 s against this
  // call's start, by this host's clock): hosts sharing a path across jobs should set one.
  struct Record { char magic[8]; int nranks; char nonce[64]; char id[CLIMA_COMM_ID_BYTES]; } rec;
  std::memset(&rec, 0, sizeof(rec));
  std::memcpy(rec.magic, "CLRCOMM1", 8);
  rec.nranks = *nranks;
  const char *nonce = getenv("CLIMA_COMM_NONCE");
  if (!nonce || !nonce[0]) nonce = getenv("SLURM_JOB_ID");
  if (nonce) std::strncpy(rec.nonce, nonce, sizeof(rec.nonce) - 1);
  if (*rank == 0) {
    (void)std::remove(file.c_str());   // whatever an earlier job left there
    ncclUniqueId u;
    NCCLCHK(ncclGetUniqueId(&u));
    std::memcpy(id, &u, sizeof(u));
    std::memcpy(rec.id, id, sizeof(id));
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f || std::fwrite(&rec, 1, sizeof(rec), f) != sizeof(rec) || std::fclose(f) != 0 || std::rename(tmp.c_str(), file.c_str()) != 0)
      throw HipFail{"radtran_comm_init_file: cannot write " + file};
  } else {
    bool got = false, stale = false;
    const time_t t_enter = time(nullptr);
    int max_tries = 6000;   // up to ~120 s (CLIMA_COMM_WAIT_S: another bound, in seconds -- the tests use 1)
    if (const char *w = getenv("CLIMA_COMM_WAIT_S")) max_tries = std::max(1, atoi(w) * 50);
    for (int tries = 0; tries < max_tries && !got; tries++) {
      struct stat st;
      if (stat(file.c_str(), &st) == 0 && st.st_size == (off_t)sizeof(rec)) {
        Record got_rec;
        FILE *f = std::fopen(file.c_str(), "rb");
        const bool read_ok = f && std::fread(&got_rec, 1, sizeof(got_rec), f) == sizeof(got_rec);
        if (f) std::fclose(f);
        const bool mine = read_ok && std::memcmp(got_rec.magic, rec.magic, 8) == 0 && got_rec.nranks == rec.nranks &&
                          std::memcmp(got_rec.nonce, rec.nonce, sizeof(rec.nonce)) == 0 &&
                          (rec.nonce[0] || st.st_mtime >= t_enter - 60);
        if (mine) { std::memcpy(id, got_rec.id, sizeof(id)); got = true; }
        else if (read_ok) stale = true;
      }
      if (!got) usleep(20000);
    }
    if (!got) throw HipFail{std::string("radtran_comm_init_file: rank 0 did not publish a record for this job at ") + file +
                            (stale ? " (a record of another job, communicator size or nonce is there)" : "")};
  }
  comm_attach(r, *nranks, *rank, id);   // collective: returns once every rank has joined
  if (*rank == 0) (void)std::remove(file.c_str());
  CATCH(err)
  if (err && err[0]) return;
  radtran_set_bin_shard(ptr, rank, nranks, err);
}

void radtran_comm_get(void *ptr, int *nranks, int *rank, int *reduces) {
  Radtran *r = as_rad(ptr);
  *nranks = (r && r->comm) ? r->comm_n : 0;
  *rank = (r && r->comm) ? r->comm_rank : 0;
  if (reduces) *reduces = r ? (int)std::min<long>(r->comm_reduces, 2147483647L) : 0;
}

void radtran_comm_destroy(void *ptr) {
  Radtran *r = as_rad(ptr);
  if (!r || !r->comm) return;
  (void)hipStreamSynchronize(r->stream);
  (void)ncclCommDestroy(r->comm);
  r->comm = nullptr; r->comm_n = 1; r->comm_rank = 0;
  const int zero = 0, one = 1;
  char e[CLIMA_ERR_LEN + 1];
  radtran_set_bin_shard(ptr, &zero, &one, e);   // back to the whole spectrum
}

void radtran_bin_shard_get(void *ptr, int *op_lo, int *op_n, int *ir_lo, int *ir_n, int *sol_lo, int *sol_n) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  *op_lo = r->op_lo; *op_n = r->op_n; *ir_lo = r->ir_lo; *ir_n = r->ir_n; *sol_lo = r->sol_lo; *sol_n = r->sol_n;
}

void radtran_finish_reduced(void *ptr, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  // f_total = (sol_dn - sol_up) + (ir_dn - ir_up) of the reduced rows is formed on the host when the
  // results are fetched (fetch_small), like after every call: nothing to launch here, the level
  // rows just have to be read again
  TRY
  settle_device_batch(r);
  CATCH(err)
  r->holds.rows_changed();
}

void radtran_stream_get(void *ptr, void **stream) {
  Radtran *r = as_rad(ptr);
  *stream = r ? (void *)r->stream : nullptr;
  if (!r || r->state != 2) return;
  // whoever orders work of their own behind this stream finds every call enqueued so far on it
  try { join_lanes(r); } catch (const HipFail &f) { defer_err(r, f.msg); }
}

void radtran_profile_set(void *ptr, const int *enable) {
  Radtran *r = as_rad(ptr);
  if (r) r->profile = (*enable == 2) ? 2 : (*enable != 0 ? 1 : 0);
}
void radtran_profile_stride_set(void *ptr, const int *stride) {
  Radtran *r = as_rad(ptr);
  if (r) r->profile_stride = std::max(1, *stride);
}
void radtran_profile_reset(void *ptr) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  for (int i = 0; i < 7; i++) { r->k_ms[i] = 0; r->k_n[i] = 0; }
  r->timer_calls = r->profile_stride - 1;  // with a sampling stride, the next call is a sampled one
}
void radtran_kernel_time_get(void *ptr, const int *kernel_id, double *ms_total, int *launches, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (*kernel_id < 0 || *kernel_id > 6) { set_err(err, "kernel id out of range"); return; }
  TRY
  if (!r->pending.empty()) { drain_lanes(r); resolve_events(r); }
  *ms_total = r->k_ms[*kernel_id];
  *launches = r->k_n[*kernel_id];
  CATCH(err)
}

// Distinct nodes of a 1-D axis that the stencils of `vals` touch, and of a k-table's (P,T) grid that the last uploaded column's do
static double distinct_nodes(const std::vector<double> &axis, const std::vector<double> &vals) {
  std::set<int> s;
  const double lo = *std::min_element(axis.begin(), axis.end()), hi = *std::max_element(axis.begin(), axis.end());
  for (double v : vals) { const int i = host_bracket(axis, std::min(std::max(v, lo), hi)); s.insert(i); s.insert(i + 1); }
  return (double)s.size();
}
static double distinct_pt_nodes(const Radtran *r, const KTabHost *k) {
  std::set<std::pair<int, int>> s;
  const double plo = *std::min_element(k->log10P.begin(), k->log10P.end()), phi = *std::max_element(k->log10P.begin(), k->log10P.end());
  const double tlo = *std::min_element(k->temp.begin(), k->temp.end()), thi = *std::max_element(k->temp.begin(), k->temp.end());
  for (int j = 0; j < r->nz; j++) {
    const int iP = host_bracket(k->log10P, std::min(std::max(std::log10(r->last_P[j]), plo), phi));
    const int iT = host_bracket(k->temp, std::min(std::max(r->last_T[j], tlo), thi));
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) s.insert({iP + a, iT + b});
  }
  return (double)s.size();
}

void radtran_algorithmic_bytes(void *ptr, double *bytes_tables_distinct, double *bytes_in, double *bytes_out,
                               double *bytes_tables_full, char *err) {
  // B_alg = B_tab(distinct interpolation nodes touched by the column)
  // + B_in + B_out; intermediates (opr) get no credit.
  clear_err(err);
  GUARD(r, ptr, err);
  if (refuse(r, "algorithmic_bytes", NEED_COLUMN, err)) return;
  const int nz = r->nz;
  const double nw = r->nw;
  double distinct = 0.0, full = 0.0;
  for (auto *k : r->k) {
    distinct += 8.0 * k->ng * nw * distinct_pt_nodes(r, k);
    full += 8.0 * k->ng * nw * k->nP * k->nT;
  }
  for (auto *v : {&r->cia, &r->pxs, &r->ray})
    for (auto *xs : *v) {
      if (xs->dim) { distinct += 8.0 * nw * distinct_nodes(xs->temp, r->last_T); full += 8.0 * nw * xs->nT; }
      else { distinct += 8.0 * nw; full += 8.0 * nw; }
    }
  if (r->has_cont) { distinct += 2 * 8.0 * nw * distinct_nodes(r->cont_temp, r->last_T); full += 2 * 8.0 * nw * r->cont_nT; }
  for (auto *p : r->part) {
    if (!r->last_radii.empty()) {
      std::vector<double> rr(r->last_radii.begin() + (size_t)p->p_ind * nz, r->last_radii.begin() + (size_t)(p->p_ind + 1) * nz);
      distinct += 3 * 8.0 * nw * distinct_nodes(p->radii, rr);
    }
    full += 3 * 8.0 * nw * p->nrad;
  }
  *bytes_tables_distinct = distinct; *bytes_tables_full = full;
  *bytes_in = 8.0 * (nz * (3.0 + r->nsp + 2.0 * r->np) + 2.0 * nw + (int)r->zenith_u.size() * 2.0 + r->sol.nw);
  *bytes_out = 8.0 * ((2.0 * (nz + 1) + nz) * r->ir.nw + (3.0 * (nz + 1) + nz) * r->sol.nw + 5.0 * (nz + 1));
}

// N_PT = distinct (P,T) nodes of a k-table that the last uploaded column's bilinear
// stencils touch (mean over the k-tables; <= nP*nT), N_T likewise for the 1-D (temperature) tables.
void radtran_algorithmic_nodes(void *ptr, double *n_pt, double *n_pt_full, double *n_t, double *n_t_full, char *err) {
  clear_err(err);
  GUARD(r, ptr, err);
  if (refuse(r, "algorithmic_nodes", NEED_COLUMN, err)) return;
  double spt = 0.0, sptf = 0.0;
  for (auto *k : r->k) { spt += distinct_pt_nodes(r, k); sptf += (double)k->nP * k->nT; }
  double st = 0.0, stf = 0.0;
  int n1 = 0;
  for (auto *v : {&r->cia, &r->pxs})
    for (auto *xs : *v)
      if (xs->dim) { st += distinct_nodes(xs->temp, r->last_T); stf += xs->nT; n1++; }
  if (r->has_cont) { st += 2 * distinct_nodes(r->cont_temp, r->last_T); stf += 2 * r->cont_nT; n1 += 2; }
  *n_pt = r->k.empty() ? 0.0 : spt / r->k.size();
  *n_pt_full = r->k.empty() ? 0.0 : sptf / r->k.size();
  *n_t = n1 ? st / n1 : 0.0;
  *n_t_full = n1 ? stf / n1 : 0.0;
}

#ifdef CLIMA_STAMPS
extern "C" void clima_debug_stamps(void *ptr, long long *out) {
  Radtran *r = as_rad(ptr);
  (void)hipStreamSynchronize(r->stream);
  (void)hipMemcpy(out, r->d_stamps.p, (64 + 2 * 8192) * sizeof(long long), hipMemcpyDeviceToHost);
}
#endif

void radtran_opr_get(void *ptr, double *tau, double *w0, double *g, double *tau_band, char *err) {
  clear_err(err);
  GUARD_BUILT(r, ptr, err);
  if (refuse(r, "opr_get", NEED_OPACITIES, err)) return;
  TRY
  settle(r);       // (a repaired hand-off recomputes the optical properties)
  ensure_w0(r);
  HIPCHK(hipStreamSynchronize(r->stream));
  if (tau) HIPCHK(hipMemcpy(tau, r->d_tau.p, r->d_tau.n * sizeof(double), hipMemcpyDeviceToHost));
  if (w0) HIPCHK(hipMemcpy(w0, r->d_w0.p, r->d_w0.n * sizeof(double), hipMemcpyDeviceToHost));
  if (g) HIPCHK(hipMemcpy(g, r->d_g.p, r->d_g.n * sizeof(double), hipMemcpyDeviceToHost));
  if (tau_band) HIPCHK(hipMemcpy(tau_band, r->d_tau_band.p, r->d_tau_band.n * sizeof(double), hipMemcpyDeviceToHost));
  CATCH(err)
}

void clima_test_device_exp(const int *n, const double *x, double *y, char *err) {
  clear_err(err);
  TRY
  DevBuf<double> dx, dy;
  dx.alloc(*n); dy.alloc(*n);
  HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * *n, hipMemcpyHostToDevice));
  launch_test_exp(dx.p, dy.p, *n, nullptr);
  HIPCHK(hipMemcpy(y, dy.p, sizeof(double) * *n, hipMemcpyDeviceToHost));
  CATCH(err)
}

// the table exp of the zenith-angle loop (base10 = 0: e^x, arguments <= 0) and of the opacity tile's
// table interpolations (base10 = 1: 10^x)
void clima_test_device_exp_table(const int *n, const int *base10, const double *x, double *y, char *err) {
  clear_err(err);
  TRY
  DevBuf<double> dx, dy;
  dx.alloc(*n); dy.alloc(*n);
  HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * *n, hipMemcpyHostToDevice));
  launch_test_exp_tab(dx.p, dy.p, *n, *base10, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(y, dy.p, sizeof(double) * *n, hipMemcpyDeviceToHost));
  CATCH(err)
}

void clima_test_device_rcp(const int *n, const double *x, double *y, char *err) {
  clear_err(err);
  TRY
  DevBuf<double> dx, dy;
  dx.alloc(*n); dy.alloc((size_t)4 * *n);
  HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * *n, hipMemcpyHostToDevice));
  launch_test_rcp(dx.p, dy.p, *n, nullptr);
  HIPCHK(hipMemcpy(y, dy.p, sizeof(double) * 4 * *n, hipMemcpyDeviceToHost));
  CATCH(err)
}

void clima_test_wave_scan(const int *nwaves, const double *a, const double *b, double *out, char *err) {
  clear_err(err);
  TRY
  const size_t n = (size_t)*nwaves * 64;
  DevBuf<double> da, db, dout;
  da.alloc(n); db.alloc(n); dout.alloc(4 * n);
  HIPCHK(hipMemcpy(da.p, a, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db.p, b, sizeof(double) * n, hipMemcpyHostToDevice));
  launch_test_wscan(da.p, db.p, dout.p, *nwaves, nullptr);
  HIPCHK(hipMemcpy(out, dout.p, sizeof(double) * 4 * n, hipMemcpyDeviceToHost));
  CATCH(err)
}


// Test hook: ONE column through the production two-stream kernels with its optical properties
// and Planck values given directly -- the inputs and outputs of the reference's two_stream_ir /
// two_stream_solar (src/radtran/clima_radtran_twostream.f90:10-295), which is what
// tests/golden/twostream_golden.npz holds.  The column is presented as one bin that lies in both
// channels, `ng` g-points carrying the same tau/w0 with weights wbin (sum 1), one zenith angle u0 of
// weight 1, unit stellar flux and unit factors, so the kernels' weighted sums reproduce the solver's
// own outputs.  form: 0 wave-per-column kernel (k_twostream_w<slots>), 1 workgroup-per-bin kernel
// (k_twostream), 2 the two-stream part of the fused grid (k_fused, whole-wave form, slots 2..8, ng = 8), 4 the
// same in the half-wave form (two g-point columns per wave, slots = ceil(nz/32) = 3..7), 5 the same in the
// paired form (every layer 2m+1 a copy of layer 2m: even nz, slots 2, 4, 6, 8; the caller passes such a column),
// 3 batched shared-opacity IR kernel (k_twostream_ir_batch<slots, NW>, IR outputs only: slots 1..4 in blocks of 8
// g-point waves, 5..8 in blocks of 4), 6 the same with blocks of 4 waves at every slot count.
// slots = layer slots per lane (>= ceil(nz/64)).  Outputs are TOA-first like the solver's.
void clima_test_two_stream(const int *nz_, const int *ng_, const int *form, const int *slots, const double *tau,
                           const double *w0, const double *g, const double *bplanck, const double *ir_par,
                           const double *sol_par, const double *wbin, double *ir_fup, double *ir_fdn,
                           double *sol_fup, double *sol_fdn, double *sol_amean, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nl = nz + 1;
  if (nz < 1 || ng < 1 || ng > 32) throw HipFail{"clima_test_two_stream: bad nz / ng"};
  std::vector<double> h_tau((size_t)ng * nz), h_w0((size_t)ng * nz);
  for (int c = 0; c < ng; c++)
    for (int i = 0; i < nz; i++) { h_tau[(size_t)c * nz + i] = tau[i]; h_w0[(size_t)c * nz + i] = w0[i]; }
  DevBuf<double> d_tau, d_w0, d_g, d_tb, d_bp, d_wbin, d_freq, d_T, d_one, d_em, d_alb, d_zu, d_zw, d_ziu, d_out;
  d_tau.upload(h_tau); d_w0.upload(h_w0);
  d_g.upload(std::vector<double>(g, g + nz));
  d_tb.upload(std::vector<double>(nz, 0.0));
  d_bp.upload(std::vector<double>(bplanck, bplanck + nl));
  d_wbin.upload(std::vector<double>(wbin, wbin + ng));
  d_freq.upload(std::vector<double>{2.0e13, 1.0e13});
  d_T.upload(std::vector<double>(nl, 250.0));
  d_one.upload(std::vector<double>{1.0});
  d_em.upload(std::vector<double>{ir_par[0]});
  d_alb.upload(std::vector<double>{sol_par[1]});
  d_zu.upload(std::vector<double>{sol_par[0]});
  d_zw.upload(std::vector<double>{1.0});
  d_ziu.upload(std::vector<double>{1.0 / sol_par[0]});
  d_out.alloc((size_t)7 * nl); d_out.zero();
  DevBuf<int> d_qm;
  TwoStreamParams ts;
  std::memset(&ts, 0, sizeof(ts));
  ts.nz = nz; ts.ng = ng;
  ts.n_sol = (*form == 3 || *form == 6) ? 0 : 1; ts.n_ir = 1;
  ts.tau = d_tau.p; ts.w0 = d_w0.p; ts.g = d_g.p; ts.tau_band = d_tb.p;
  ts.wbin = d_wbin.p; ts.freq = d_freq.p;
  ts.bplanck = d_bp.p; ts.force_slots = *slots;
  ts.T = d_T.p; ts.T_surface = d_T.p;
  ts.emissivity = d_em.p; ts.has_hard_surface = ir_par[1] != 0.0 ? 1 : 0; ts.ir_tau_min = ir_par[2];
  ts.nzen = 1; ts.zen_u = d_zu.p; ts.zen_w = d_zw.p; ts.zen_iu = d_ziu.p;
  ts.zen_u_v[0] = sol_par[0]; ts.zen_w_v[0] = 1.0; ts.zen_iu_v[0] = 1.0 / sol_par[0];
  ts.albedo = d_alb.p; ts.photons_sol = d_one.p; ts.photon_scale_factor = 1.0; ts.diurnal_fac = 1.0;
  ts.am_f1 = d_one.p; ts.am_f2 = d_one.p; ts.am_dw = d_one.p;
  auto out_arr = [&](int k) { return d_out.p + (size_t)k * nl; };   // seven arrays of nl; the first five go back
  ts.ir_fup_a = out_arr(0); ts.ir_fdn_a = out_arr(1); ts.sol_fup_a = out_arr(2); ts.sol_fdn_a = out_arr(3);
  ts.sol_amean = out_arr(4); ts.ir_tau_band = out_arr(5); ts.sol_tau_band = out_arr(6);
  bool ok = false;
  PlanIn in{};   // a call on stored opacities, no handle: forms 0 and 1 are the plan's stand-alone forms
  in.nz = nz; in.ng = ng; in.nzen = 1; in.n_ir = ts.n_ir; in.n_sol = ts.n_sol; in.ncol = 1;
  in.force_slots = *slots; in.no_half = sw_no_half();
  const LaunchPlan plan = plan_radiate(in);
  if (*form == 0) ok = launch_twostream_w(ts, plan.ts, nullptr);
  else if (*form == 1) ok = launch_twostream(ts, plan.block, nullptr);
  else if (*form == 2 || *form == 4 || *form == 5) {   // 4: the half-wave form (two g-point columns per wave), 5: the paired form
    if (*form == 5)
      for (int i = 0; i + 1 < nz; i += 2)
        if (tau[i] != tau[i + 1] || w0[i] != w0[i + 1] || g[i] != g[i + 1])
          throw HipFail{"clima_test_two_stream: form 5 needs a column of pairwise identical layers"};
    d_qm.upload(std::vector<int>{nz});  // the column's source-layer count
    ok = launch_fused_twostream_only(ts, *slots, d_qm.p, nullptr, *form == 4, *form == 5);
  }
  else if (*form == 3 || *form == 6) { ts.b_T = 0; ts.b_Ts = 0; ts.b_out = 0; ok = launch_twostream_ir_batch(ts, 1, nullptr, *form == 6 ? 4 : 0); }
  HIPCHK(hipGetLastError());
  if (!ok) throw HipFail{"clima_test_two_stream: this form does not cover the requested shape"};
  HIPCHK(hipDeviceSynchronize());
  double *dst[5] = {ir_fup, ir_fdn, sol_fup, sol_fdn, sol_amean};
  std::vector<double> out(out_arr(5) - d_out.p);
  HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  for (int a = 0; a < 5; a++)
    for (int n = 0; n < nl; n++) dst[a][n] = out[(size_t)a * nl + (nz - n)];  // the kernels store ground-first (radiate.f90:140-154)
  CATCH(err)
}

// Test hook of the sums over the bins: the production integration kernels on per-bin arrays, channels and owned ranges
// given directly, no handle.  ir_dims / sol_dims = {bins of the channel, first owned bin (0-based), owned bins}, freq
// [bins + 1]; the per-bin arrays [ncol][bins][nz+1] dense, staged on the device spec_stride doubles apart per column
// with NaN between the columns.  form 0: launch_integrate as a call issues it (nchunk of the larger owned range, one
// launch or two by integrate_fits_one_launch); 1: launch_integrate_two whatever the bin count.  Both: flux_n
// [ncol][4][nz+1] goes in (flux_stride apart on the device) and comes back -- with do_solar = 0 its solar rows stay, or
// are put back from flux_part --, flux_part (optional, one column) [4][nz+1] likewise.  2: launch_integrate_batch on the
// IR arrays: flux_n [4][nz+1] is read for f_total, out [3][col0 + ncol][nz+1] goes in and comes back with the rows
// from col0 on written.  tests/test_gpu_integration_sums.py holds what comes back to exact rational sums.
void clima_test_integrate(const int *form_, const int *nz_, const int *ncol_, const int *spec_stride_, const int *flux_stride_,
                          const int *ir_dims, const double *ir_freq, const int *sol_dims, const double *sol_freq,
                          const double *ir_fup_a, const double *ir_fdn_a, const double *sol_fup_a, const double *sol_fdn_a,
                          const int *do_solar, double *flux_n, double *flux_part, const int *col0_, double *out, char *err) {
  clear_err(err);
  TRY
  const int form = *form_, nz = *nz_, nl = nz + 1, ncol = *ncol_, col0 = *col0_;
  const int nw[2] = {ir_dims[0], sol_dims[0]}, lo[2] = {ir_dims[1], sol_dims[1]}, cnt[2] = {ir_dims[2], sol_dims[2]};
  const size_t spec_stride = (size_t)*spec_stride_, flux_stride = (size_t)*flux_stride_;
  if (form < 0 || form > 2 || nz < 1 || ncol < 1 || col0 < 0) throw HipFail{"clima_test_integrate: bad form / nz / ncol / col0"};
  const int nch = form == 2 ? 1 : 2;   // the batch form sums the IR channel only
  for (int c = 0; c < nch; c++)
    if (nw[c] < 1 || lo[c] < 0 || cnt[c] < 0 || lo[c] + cnt[c] > nw[c]) throw HipFail{"clima_test_integrate: an owned range outside its channel"};
  if (spec_stride < (size_t)std::max(nw[0], nch == 2 ? nw[1] : 0) * nl || (form != 2 && flux_stride < (size_t)4 * nl))
    throw HipFail{"clima_test_integrate: a stride shorter than a column"};
  const int nchunk = integrate_chunks(form == 2 ? cnt[0] : std::max(cnt[0], cnt[1]));
  const bool two = form == 1 || (form == 0 && !integrate_fits_one_launch(nchunk));
  if (two && ncol != 1) throw HipFail{"clima_test_integrate: the two-launch form takes one column"};
  if (form != 2 && flux_part && ncol != 1) throw HipFail{"clima_test_integrate: flux_part belongs to one column"};
  // (integrate_block keeps or puts back the solar rows of the FIRST column's flux_n whatever the column: a batch always computes them)
  if (form != 2 && !*do_solar && ncol != 1) throw HipFail{"clima_test_integrate: do_solar = 0 takes one column"};
  const double gap = std::numeric_limits<double>::quiet_NaN();
  auto staged = [&](const double *src, size_t per_col, size_t stride, int n) {   // n columns `stride` apart, NaN between them
    std::vector<double> h(stride * n, gap);
    for (int c = 0; c < n; c++) std::copy(src + per_col * c, src + per_col * (c + 1), h.begin() + stride * c);
    return h;
  };
  const double *spec[4] = {ir_fup_a, ir_fdn_a, sol_fup_a, sol_fdn_a};
  DevBuf<double> d_spec[4], d_freq[2], d_flux, d_part, d_partial, d_out;
  for (int a = 0; a < 2 * nch; a++) d_spec[a].upload(staged(spec[a], (size_t)nw[a / 2] * nl, spec_stride, ncol));
  d_freq[0].upload(std::vector<double>(ir_freq, ir_freq + nw[0] + 1));
  if (nch == 2) d_freq[1].upload(std::vector<double>(sol_freq, sol_freq + nw[1] + 1));
  if (form == 2) {
    const size_t out_arr = (size_t)(col0 + ncol) * nl;
    d_flux.upload(std::vector<double>(flux_n, flux_n + (size_t)4 * nl));
    d_out.upload(std::vector<double>(out, out + 3 * out_arr));
    d_partial.upload(std::vector<double>((size_t)ncol * 2 * nchunk * nl, gap));
    BatchIntegrateParams bp;
    std::memset(&bp, 0, sizeof(bp));
    bp.nz = nz; bp.ir_lo = lo[0]; bp.ir_n = cnt[0]; bp.nchunk = nchunk; bp.col0 = col0;
    bp.fup_a = d_spec[0].p; bp.fdn_a = d_spec[1].p; bp.spec_stride = spec_stride;
    bp.freq = d_freq[0].p; bp.partial = d_partial.p; bp.flux_n = d_flux.p; bp.out = d_out.p; bp.out_arr = out_arr;
    launch_integrate_batch(bp, ncol, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out.p, sizeof(double) * 3 * out_arr, hipMemcpyDeviceToHost));
  } else {
    d_flux.upload(staged(flux_n, (size_t)4 * nl, flux_stride, ncol));
    if (flux_part) d_part.upload(std::vector<double>(flux_part, flux_part + (size_t)4 * nl));
    d_partial.upload(std::vector<double>((size_t)4 * nchunk * nl, gap));
    IntegrateParams ip;
    std::memset(&ip, 0, sizeof(ip));
    ip.ncol = ncol; ip.bs.res = spec_stride; ip.bs.flux = flux_stride;
    ip.nz = nz; ip.nw_ir = nw[0]; ip.nw_sol = nw[1];
    ip.ir_lo = lo[0]; ip.ir_n = cnt[0]; ip.sol_lo = lo[1]; ip.sol_n = cnt[1];
    ip.do_solar = *do_solar != 0;
    ip.ir_fup_a = d_spec[0].p; ip.ir_fdn_a = d_spec[1].p; ip.sol_fup_a = d_spec[2].p; ip.sol_fdn_a = d_spec[3].p;
    ip.ir_freq = d_freq[0].p; ip.sol_freq = d_freq[1].p;
    ip.flux_n = d_flux.p; ip.flux_part = flux_part ? d_part.p : nullptr;
    ip.partial = d_partial.p; ip.nchunk = nchunk;
    if (form == 0) launch_integrate(ip, nullptr);
    else launch_integrate_two(ip, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> h(flux_stride * ncol);
    HIPCHK(hipMemcpy(h.data(), d_flux.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < ncol; c++) std::copy(h.begin() + flux_stride * c, h.begin() + flux_stride * c + (size_t)4 * nl, flux_n + (size_t)4 * nl * c);
    if (flux_part) HIPCHK(hipMemcpy(flux_part, d_part.p, sizeof(double) * 4 * nl, hipMemcpyDeviceToHost));
  }
  CATCH(err)
}

// Test hook of k_twostream_sol_batch, the counterpart of clima_test_two_stream for it: one column's tau / w0 / g (nz,
// TOA-first; the same for every one of the ng g-points, weights wbin) as one solar bin, `ncol` cases of nzen angles
// (zen_u, zen_w (nzen, ncol)) and surface reflectance rsfc (ncol) through the production kernel with unit stellar flux
// and unit factors.  force_nw = 4: blocks of four waves at every slot count.  Outputs (nz+1, ncol), TOA-first.
void clima_test_solar_batch(const int *nz_, const int *ng_, const int *force_nw, const double *tau, const double *w0,
                            const double *g, const double *wbin, const int *ncol, const int *nzen_, const double *zen_u,
                            const double *zen_w, const double *rsfc, double *fup, double *fdn, double *amean, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nl = nz + 1, n = *ncol, nzen = *nzen_;
  if (nz < 1 || ng < 1 || ng > 32 || n < 1 || nzen < 1 || nzen > MAX_ZEN) throw HipFail{"clima_test_solar_batch: bad nz / ng / ncol / nzen"};
  std::vector<double> h_tau((size_t)ng * nz), h_w0((size_t)ng * nz), h_zen((size_t)n * 3 * nzen);
  for (int c = 0; c < ng; c++)
    for (int i = 0; i < nz; i++) { h_tau[(size_t)c * nz + i] = tau[i]; h_w0[(size_t)c * nz + i] = w0[i]; }
  for (int c = 0; c < n; c++)
    for (int z = 0; z < nzen; z++) {
      double *q = h_zen.data() + (size_t)c * 3 * nzen;
      q[z] = zen_u[(size_t)c * nzen + z]; q[nzen + z] = zen_w[(size_t)c * nzen + z]; q[2 * nzen + z] = 1.0 / q[z];
    }
  DevBuf<double> d_tau, d_w0, d_g, d_wbin, d_zen, d_alb, d_ones, d_out;
  d_tau.upload(h_tau); d_w0.upload(h_w0);
  d_g.upload(std::vector<double>(g, g + nz));
  d_wbin.upload(std::vector<double>(wbin, wbin + ng));
  d_zen.upload(h_zen);
  d_alb.upload(std::vector<double>(rsfc, rsfc + n));
  d_ones.upload(std::vector<double>(std::max(n, 1), 1.0));
  d_out.alloc((size_t)3 * n * nl); d_out.zero();
  SolBatchParams sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.nz = nz; sp.ng = ng; sp.n_sol = 1; sp.ncase = n; sp.nzen = nzen;
  sp.tau = d_tau.p; sp.w0 = d_w0.p; sp.g = d_g.p; sp.wbin = d_wbin.p;
  sp.zen = d_zen.p; sp.albedo = d_alb.p; sp.alb_stride = 1; sp.scale = d_ones.p;
  sp.photons_sol = d_ones.p; sp.am_f1 = d_ones.p; sp.am_f2 = d_ones.p; sp.am_dw = d_ones.p; sp.diurnal_fac = 1.0;
  sp.fup = d_out.p; sp.fdn = d_out.p + (size_t)n * nl; sp.amean = d_out.p + (size_t)2 * n * nl; sp.out_stride = nl;
  const bool ok = launch_twostream_sol_batch(sp, nullptr, *force_nw);
  HIPCHK(hipGetLastError());
  if (!ok) throw HipFail{"clima_test_solar_batch: the kernel does not cover the requested shape"};
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> out((size_t)3 * n * nl);
  HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  double *dst[3] = {fup, fdn, amean};
  for (int k = 0; k < 3; k++)
    for (int c = 0; c < n; c++)
      for (int i = 0; i < nl; i++) dst[k][(size_t)c * nl + i] = out[((size_t)k * n + c) * nl + (nz - i)];  // the kernel stores ground-first
  CATCH(err)
}
void clima_test_solar_batch_cases_per_block(const int *ncol, int *cases) { *cases = solar_batch_cases_per_block(*ncol); }

// What the three IR test hooks below run on: one column's tau / w0 / g as `nbin` IR bins of ng g-points each, every g-point
// of every bin carrying the same column, on the device with wbin and the emissivity, and the GreenParams of such a handle
// (ir_par = {emissivity, has_hard_surface, ir_tau_min}; no frequency grids: the hooks hand the Planck terms over)
namespace {
struct TestIrColumn {
  DevBuf<double> tau, w0, g, wbin, em;
  GreenParams params;
  TestIrColumn(int nz, int ng, int nbin, const double *tau_, const double *w0_, const double *g_, const double *ir_par, const double *wbin_) {
    const int NQ = nbin * ng;
    std::vector<double> h_tau((size_t)NQ * nz), h_w0((size_t)NQ * nz), h_g((size_t)nbin * nz);
    for (int c = 0; c < NQ; c++)
      for (int i = 0; i < nz; i++) { h_tau[(size_t)c * nz + i] = tau_[i]; h_w0[(size_t)c * nz + i] = w0_[i]; }
    for (int b = 0; b < nbin; b++)
      for (int i = 0; i < nz; i++) h_g[(size_t)b * nz + i] = g_[i];
    tau.upload(h_tau); w0.upload(h_w0); g.upload(h_g);
    wbin.upload(std::vector<double>(wbin_, wbin_ + ng)); em.upload(std::vector<double>((size_t)nbin, ir_par[0]));
    std::memset(&params, 0, sizeof(params));
    params.nz = nz; params.ng = ng; params.n_ir = nbin; params.NQ = NQ;
    params.tau = tau.p; params.w0 = w0.p; params.g = g.p; params.wbin = wbin.p; params.emissivity = em.p;
    params.has_hard_surface = ir_par[1] != 0.0 ? 1 : 0; params.ir_tau_min = ir_par[2];
  }
};
}  // namespace

// Test hook of the response form (ir_green.inc), the counterpart of clima_test_two_stream for it: one column's tau / w0 /
// g (the same for every g-point, weights wbin) and ndev deviations (level k TOA-first, k = nz the surface; change of the
// Planck value there) -> per deviation the change of the level fluxes (TOA-first), sum over the g-points, exactly as the
// production kernels form it (k_green_factor / unit / local / accum_far / accum_mixed); only the Planck differences come
// from the caller instead of k_green_db.
void clima_test_ir_response(const int *nz_, const int *ng_, const double *tau, const double *w0, const double *g,
                            const double *ir_par, const double *wbin, const int *ndev_, const int *dev_k,
                            const double *dev_db, double *resp_up, double *resp_dn, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nl = nz + 1, ndev = *ndev_;
  if (nz < 4 || ng < 1 || ng > 32 || ndev < 1) throw HipFail{"clima_test_ir_response: bad nz / ng / ndev"};
  std::vector<int> order(ndev);
  for (int i = 0; i < ndev; i++) { order[i] = i; if (dev_k[i] < 0 || dev_k[i] > nz) throw HipFail{"clima_test_ir_response: bad level"}; }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return dev_k[a] < dev_k[b]; });
  const int ndev_pad = green_ndev_pad(ndev);
  std::vector<double> h_db(ndev_pad + 64, 0.0);
  std::vector<int> hi(ndev_pad, 0), mdev, mblk;
  for (int d = 0; d < ndev; d++) { hi[d] = dev_k[order[d]]; h_db[d] = dev_db[order[d]]; }
  green_mixed_list(std::vector<int>(hi.begin(), hi.begin() + ndev), nz, mdev, mblk);
  const int nmix = (int)mdev.size();
  hi.insert(hi.end(), mdev.begin(), mdev.end());
  hi.insert(hi.end(), mblk.begin(), mblk.end());
  TestIrColumn col(nz, ng, 1, tau, w0, g, ir_par, wbin);
  DevBuf<double> d_db, d_work;
  DevBuf<int> d_idx;
  d_db.upload(h_db); d_idx.upload(hi);
  const size_t work = green_work_views(nz, ng, nullptr).count;
  d_work.alloc(work + (size_t)ndev_pad * 2 * nl); d_work.zero();   // ... and the one array of partial sums behind them
  GreenParams gp = col.params;
  const GreenWork w = green_work_views(nz, ng, d_work.p);
  gp.RW = w.RW; gp.IS = w.IS; gp.FS = w.FS; gp.DS = w.DS; gp.D0 = w.D0;
  gp.partial = d_work.p + work;
  gp.DB = d_db.p;
  gp.ndev = ndev; gp.ndev_pad = ndev_pad; gp.qsplit = 1; gp.msplit = 1; gp.partial_m = gp.partial;   // (disjoint pairs: one array)
  gp.dev_k = d_idx.p; gp.nmix = nmix; gp.mix_dev = gp.dev_k + ndev_pad; gp.mix_blk = gp.mix_dev + nmix;
  launch_green_factor(gp, nullptr);
  HIPCHK(hipGetLastError());
  launch_green_accumulate(gp, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> out((size_t)ndev_pad * 2 * nl);
  HIPCHK(hipMemcpy(out.data(), gp.partial, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  for (int d = 0; d < ndev; d++)
    for (int lv = 0; lv < nl; lv++) {
      resp_up[(size_t)order[d] * nl + lv] = out[((size_t)d * 2 + 0) * nl + lv];
      resp_dn[(size_t)order[d] * nl + lv] = out[((size_t)d * 2 + 1) * nl + lv];
    }
  CATCH(err)
}

// Test hook of the adjoint rows (ir_adjoint.inc), the counterpart of clima_test_ir_response for them: one column's tau /
// w0 / g (the same for every g-point, weights wbin) as one IR bin and nrow levels (0..nz, TOA-first) -> d fup(level) /
// d bplanck(k) and d fdn(level) / d bplanck(k), (nrow, nz+1) row after row, k TOA-first, summed over the g-points by the
// production kernels with unit amplitudes in place of the Planck derivatives.
void clima_test_ir_adjoint(const int *nz_, const int *ng_, const double *tau, const double *w0, const double *g,
                           const double *ir_par, const double *wbin, const int *nrow_, const int *level,
                           double *dfup, double *dfdn, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nl = nz + 1, nr = *nrow_, nfun = 2 * nr;
  if (nz < 1 || ng < 1 || ng > 32 || nr < 1) throw HipFail{"clima_test_ir_adjoint: bad nz / ng / nrow"};
  std::vector<int> fun((size_t)nfun);
  for (int a = 0; a < nr; a++) {
    if (level[a] < 0 || level[a] > nz) throw HipFail{"clima_test_ir_adjoint: bad level"};
    fun[2 * a] = 2 * level[a]; fun[2 * a + 1] = 2 * level[a] + 1;
  }
  TestIrColumn col(nz, ng, 1, tau, w0, g, ir_par, wbin);
  DevBuf<double> d_work, d_out;
  DevBuf<int> d_fun;
  d_fun.upload(fun);
  const size_t n_work = ir_adjoint_work_count(nz, ng, nfun), n_part = ir_adjoint_part_count(nz, ng, nfun), arr = (size_t)nr * nl;
  d_work.alloc(n_work + n_part); d_work.zero();
  d_out.alloc(2 * arr); d_out.zero();
  IrAdjointParams p;
  std::memset(&p, 0, sizeof(p));
  p.g = col.params;
  p.nfun = nfun; p.nrow = nr; p.ndir = 2; p.fun = d_fun.p;
  p.work = d_work.p; p.part = p.work + n_work; p.out_up = d_out.p; p.out_dn = d_out.p + arr;
  launch_ir_adjoint(p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> out(2 * arr);
  HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  for (int a = 0; a < nr; a++)
    for (int k = 0; k < nl; k++) {      // the kernel writes (bin, a, j = nz - k)
      dfup[(size_t)a * nl + k] = out[a + (size_t)nr * (nz - k)];
      dfdn[(size_t)a * nl + k] = out[arr + a + (size_t)nr * (nz - k)];
    }
  CATCH(err)
}

// Test hook of the optical-property gradient (ir_opr_sens.inc), in the shape of clima_test_ir_adjoint: one column's tau /
// w0 / g (the same for every g-point, weights wbin), its Planck values bplanck (nz+1, TOA-first) and nrow levels (0..nz,
// TOA-first) -> d fup(level(a)) / d tau(n), / d w0(n), / d g(n) and the same of fdn, (nrow, nz) row after row, n TOA-first,
// summed over the g-points.  ONE launch of the production kernels: every (row, direction) is a bin of its own with the
// column's opacities and a unit cotangent on that row and direction alone.
void clima_test_ir_opr_sens(const int *nz_, const int *ng_, const double *tau, const double *w0, const double *g,
                            const double *bplanck, const double *ir_par, const double *wbin, const int *nrow_, const int *level,
                            double *up_tau, double *up_w0, double *up_g, double *dn_tau, double *dn_w0, double *dn_g, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nl = nz + 1, nr = *nrow_, nb = 2 * nr, NQ = nb * ng;
  if (nz < 1 || ng < 1 || ng > 32 || nr < 1) throw HipFail{"clima_test_ir_opr_sens: bad nz / ng / nrow"};
  for (int a = 0; a < nr; a++)
    if (level[a] < 0 || level[a] > nz) throw HipFail{"clima_test_ir_opr_sens: bad level"};
  const size_t ntau = (size_t)NQ * nz, ngg = (size_t)nb * nz;
  std::vector<double> h_gs(2 * (size_t)nb * nr, 0.0);
  for (int a = 0; a < nr; a++) {
    h_gs[(size_t)(2 * a) + (size_t)nb * a] = 1.0;                               // up: bin 2a
    h_gs[(size_t)nb * nr + (size_t)(2 * a + 1) + (size_t)nb * a] = 1.0;         // down: bin 2a+1
  }
  TestIrColumn col(nz, ng, nb, tau, w0, g, ir_par, wbin);
  DevBuf<double> d_bp, d_gs, d_work, d_out;
  DevBuf<int> d_lv;
  d_bp.upload(std::vector<double>(bplanck, bplanck + nl)); d_gs.upload(h_gs);
  d_lv.upload(std::vector<int>(level, level + nr));
  const size_t n_work = ir_opr_work_count(nz, NQ), n_part = ir_opr_part_count(nz, NQ);
  d_work.alloc(n_work + n_part); d_work.zero();
  d_out.alloc(2 * ntau + ngg); d_out.zero();
  IrOprParams p;
  std::memset(&p, 0, sizeof(p));
  p.g = col.params;
  p.bplanck = d_bp.p;
  p.nsel = nr; p.gs_ld = nb; p.level = d_lv.p;
  p.gs_up = d_gs.p; p.gs_dn = d_gs.p + (size_t)nb * nr;
  p.work = d_work.p; p.part_g = p.work + n_work;
  p.grad_tau = d_out.p; p.grad_w0 = d_out.p + ntau; p.grad_g = d_out.p + 2 * ntau;
  launch_ir_opr_sens(p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> out(2 * ntau + ngg);
  HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  double *const o_tau[2] = {up_tau, dn_tau}, *const o_w0[2] = {up_w0, dn_w0}, *const o_g[2] = {up_g, dn_g};
  for (int a = 0; a < nr; a++)
    for (int d = 0; d < 2; d++) {
      const int b = 2 * a + d;
      for (int i = 0; i < nz; i++) {
        double st = 0.0, sw = 0.0;
        for (int c = 0; c < ng; c++) {      // the g-points in g order
          st = st + out[((size_t)b * ng + c) * nz + i];
          sw = sw + out[ntau + ((size_t)b * ng + c) * nz + i];
        }
        o_tau[d][(size_t)a * nz + i] = st; o_w0[d][(size_t)a * nz + i] = sw;
        o_g[d][(size_t)a * nz + i] = out[2 * ntau + (size_t)b * nz + i];
      }
    }
  CATCH(err)
}

// Test hook of the solar optical-property gradient (sol_opr_sens.inc), in the shape of clima_test_ir_opr_sens with
// clima_test_solar_batch's inputs: one column's tau / w0 / g (the same for every g-point, weights wbin), nzen zenith
// angles with their weights, the surface reflectance rsfc and nrow levels (0..nz, TOA-first) -> the derivatives of fup,
// fdn and amean at level(a) in tau(n), w0(n), g(n) ((nrow, nz) row after row, n TOA-first, summed over the g-points) and in
// rsfc ((nrow)).  ONE launch of the production kernels with unit stellar flux and unit factors: every (row, quantity) is a
// solar bin of its own with the column's opacities and a unit cotangent on that row and quantity alone.
void clima_test_sol_opr_sens(const int *nz_, const int *ng_, const double *tau, const double *w0, const double *g,
                             const double *wbin, const int *nzen_, const double *zen_u, const double *zen_w, const double *rsfc,
                             const int *nrow_, const int *level, double *up_tau, double *up_w0, double *up_g, double *up_rsfc,
                             double *dn_tau, double *dn_w0, double *dn_g, double *dn_rsfc, double *am_tau, double *am_w0,
                             double *am_g, double *am_rsfc, char *err) {
  clear_err(err);
  TRY
  const int nz = *nz_, ng = *ng_, nr = *nrow_, nzen = *nzen_, nb = 3 * nr, NQ = nb * ng;
  if (nz < 1 || ng < 1 || ng > 32 || nr < 1 || nzen < 1 || nzen > MAX_ZEN) throw HipFail{"clima_test_sol_opr_sens: bad nz / ng / nrow / nzen"};
  for (int a = 0; a < nr; a++)
    if (level[a] < 0 || level[a] > nz) throw HipFail{"clima_test_sol_opr_sens: bad level"};
  const size_t ntau = (size_t)NQ * nz, ngg = (size_t)nb * nz;
  std::vector<double> h_tau(ntau), h_w0(ntau), h_g(ngg), h_zen((size_t)3 * nzen), h_gs(3 * (size_t)nb * nr, 0.0);
  for (int c = 0; c < NQ; c++)
    for (int i = 0; i < nz; i++) { h_tau[(size_t)c * nz + i] = tau[i]; h_w0[(size_t)c * nz + i] = w0[i]; }
  for (int b = 0; b < nb; b++)
    for (int i = 0; i < nz; i++) h_g[(size_t)b * nz + i] = g[i];
  for (int z = 0; z < nzen; z++) { h_zen[z] = zen_u[z]; h_zen[nzen + z] = zen_w[z]; h_zen[2 * nzen + z] = 1.0 / zen_u[z]; }
  for (int a = 0; a < nr; a++)
    for (int k = 0; k < 3; k++) h_gs[(size_t)k * nb * nr + (size_t)(3 * a + k) + (size_t)nb * a] = 1.0;   // quantity k of row a: bin 3a + k
  DevBuf<double> d_tau, d_w0, d_g, d_wbin, d_zen, d_alb, d_ones, d_freq, d_gs, d_work, d_out;
  DevBuf<int> d_lv;
  d_tau.upload(h_tau); d_w0.upload(h_w0); d_g.upload(h_g);
  d_wbin.upload(std::vector<double>(wbin, wbin + ng));
  d_zen.upload(h_zen);
  d_alb.upload(std::vector<double>((size_t)nb, *rsfc));
  d_ones.upload(std::vector<double>((size_t)nb, 1.0));
  d_freq.upload(std::vector<double>((size_t)nb + 1, 0.0));
  d_gs.upload(h_gs);
  d_lv.upload(std::vector<int>(level, level + nr));
  const size_t n_work = sol_opr_work_count(nz, NQ), n_part = sol_opr_part_count(nz, NQ);
  d_work.alloc(n_work + n_part); d_work.zero();
  d_out.alloc(2 * ntau + ngg + nb); d_out.zero();
  SolOprParams p;
  std::memset(&p, 0, sizeof(p));
  p.nz = nz; p.ng = ng; p.n_sol = nb; p.NQ = NQ; p.nzen = nzen;
  p.tau = d_tau.p; p.w0 = d_w0.p; p.g = d_g.p; p.wbin = d_wbin.p;
  p.zen_u = d_zen.p; p.zen_w = d_zen.p + nzen; p.zen_iu = d_zen.p + 2 * nzen;
  p.albedo = d_alb.p; p.photons_sol = d_ones.p; p.am_f1 = d_ones.p; p.am_f2 = d_ones.p; p.am_dw = d_ones.p; p.scale = 1.0;
  p.sol_freq = d_freq.p;
  p.nsel = nr; p.gs_ld = nb; p.level = d_lv.p;
  p.gs_up = d_gs.p; p.gs_dn = d_gs.p + (size_t)nb * nr; p.gs_am = d_gs.p + (size_t)2 * nb * nr;
  p.work = d_work.p; p.part_g = p.work + n_work; p.part_alb = p.part_g + (size_t)NQ * nz;
  p.grad_tau = d_out.p; p.grad_w0 = d_out.p + ntau; p.grad_g = d_out.p + 2 * ntau; p.grad_albedo = d_out.p + 2 * ntau + ngg;
  launch_sol_opr_sens(p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  std::vector<double> out(2 * ntau + ngg + nb);
  HIPCHK(hipMemcpy(out.data(), d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  double *const o_tau[3] = {up_tau, dn_tau, am_tau}, *const o_w0[3] = {up_w0, dn_w0, am_w0}, *const o_g[3] = {up_g, dn_g, am_g},
         *const o_r[3] = {up_rsfc, dn_rsfc, am_rsfc};
  for (int a = 0; a < nr; a++)
    for (int k = 0; k < 3; k++) {
      const int b = 3 * a + k;
      for (int i = 0; i < nz; i++) {
        double st = 0.0, sw = 0.0;
        for (int c = 0; c < ng; c++) {      // the g-points in g order
          st = st + out[((size_t)b * ng + c) * nz + i];
          sw = sw + out[ntau + ((size_t)b * ng + c) * nz + i];
        }
        o_tau[k][(size_t)a * nz + i] = st; o_w0[k][(size_t)a * nz + i] = sw;
        o_g[k][(size_t)a * nz + i] = out[2 * ntau + (size_t)b * nz + i];
      }
      o_r[k][a] = out[2 * ntau + ngg + b];
    }
  CATCH(err)
}

// which form of the response form's far accumulation the process uses from here on: 0 the matrix-core kernel
// (k_green_accum_far_mfma, the default), 1 the vector kernel (k_green_accum_far)
void clima_test_green_far_form_set(const int *vector_form) { green_vector_form_set(*vector_form); }

// ---- reference-named getters / setters (clima/fortran/Radtran.f90) -------------------

static double bolometric(Radtran *r) {  // Radtran_bolometric_flux, clima_radtran.f90:353-364
  double flux = 0.0;
  for (int i = 0; i < r->sol.nw; i++) flux = flux + r->photons_sol[i] * (r->sol.freq[i] - r->sol.freq[i + 1]);
  return r->photon_scale_factor * flux / 1.0e3;
}
void radtran_set_bolometric_flux_wrapper(void *ptr, const double *flux) {  // :345-350
  Radtran *r = as_rad(ptr);
  if (!r) return;
  r->photon_scale_factor = 1.0;
  r->photon_scale_factor = *flux / bolometric(r);
}
void radtran_bolometric_flux_wrapper(void *ptr, double *flux) {
  Radtran *r = as_rad(ptr);
  if (r) *flux = bolometric(r);
}
static double equilibrium_temperature(double stellar_radiation, double bond_albedo) {  // clima_eqns.f90:248-254
  return std::pow((stellar_radiation * (1.0 - bond_albedo)) / (4.0 * SIGMA_SI), 0.25);
}
void radtran_skin_temperature_wrapper(void *ptr, const double *bond_albedo, double *T_skin) {  // clima_eqns.f90:256-261
  Radtran *r = as_rad(ptr);
  if (r) *T_skin = equilibrium_temperature(bolometric(r), *bond_albedo) * std::pow(0.5, 0.25);
}
void radtran_equilibrium_temperature_wrapper(void *ptr, const double *bond_albedo, double *T_eq) {
  Radtran *r = as_rad(ptr);
  if (r) *T_eq = equilibrium_temperature(bolometric(r), *bond_albedo);
}

#define VEC_GETSET(name, field)                                                                 \
  void radtran_##name##_get_size(void *ptr, int *dim1) {                                        \
    Radtran *r = as_rad(ptr);                                                                   \
    *dim1 = r ? (int)r->field.size() : 0;                                                       \
  }                                                                                             \
  void radtran_##name##_get(void *ptr, const int *dim1, double *arr) {                          \
    Radtran *r = as_rad(ptr);                                                                   \
    if (!r) return;                                                                             \
    for (int i = 0; i < *dim1 && i < (int)r->field.size(); i++) arr[i] = r->field[i];           \
  }                                                                                             \
  void radtran_##name##_set(void *ptr, const int *dim1, const double *arr) {                    \
    Radtran *r = as_rad(ptr);                                                                   \
    if (!r) return;                                                                             \
    /* dirty only when a value changes: the Fortran module pushes every public field before every radiate, \
       and an upload costs a stream synchronise and six copies */                                \
    for (int i = 0; i < *dim1 && i < (int)r->field.size(); i++)                                 \
      if (r->field[i] != arr[i]) { r->field[i] = arr[i]; r->fields_dirty = true; }              \
  }
VEC_GETSET(zenith_u, zenith_u)
VEC_GETSET(surface_albedo, surface_albedo)
VEC_GETSET(surface_emissivity, surface_emissivity)

void radtran_zenith_weights_get(void *ptr, const int *dim1, double *arr) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  for (int i = 0; i < *dim1 && i < (int)r->zenith_w.size(); i++) arr[i] = r->zenith_w[i];
}
void radtran_zenith_weights_set(void *ptr, const int *dim1, const double *arr) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  for (int i = 0; i < *dim1 && i < (int)r->zenith_w.size(); i++)
    if (r->zenith_w[i] != arr[i]) { r->zenith_w[i] = arr[i]; r->fields_dirty = true; }
}
// logical(c_bool) in the reference (clima/fortran/Radtran.f90:211-227; Radtran_pxd.pxd:45-46 binds bool*):
// exactly one byte is read or written
static_assert(sizeof(bool) == 1, "logical(c_bool) is one byte");
void radtran_has_hard_surface_get(void *ptr, bool *val) { Radtran *r = as_rad(ptr); if (r) *val = r->has_hard_surface; }
void radtran_has_hard_surface_set(void *ptr, const bool *val) {
  Radtran *r = as_rad(ptr);
  if (r) r->has_hard_surface = (*reinterpret_cast<const unsigned char *>(val) != 0);
}
void radtran_photon_scale_factor_get(void *ptr, double *val) { Radtran *r = as_rad(ptr); if (r) *val = r->photon_scale_factor; }
void radtran_photon_scale_factor_set(void *ptr, const double *val) { Radtran *r = as_rad(ptr); if (r) r->photon_scale_factor = *val; }
void radtran_ir_tau_min_get(void *ptr, double *val) { Radtran *r = as_rad(ptr); if (r) *val = r->ir_tau_min; }
void radtran_ir_tau_min_set(void *ptr, const double *val) { Radtran *r = as_rad(ptr); if (r) r->ir_tau_min = *val; }
void radtran_diurnal_fac_get(void *ptr, double *val) { Radtran *r = as_rad(ptr); if (r) *val = r->diurnal_fac; }
void radtran_diurnal_fac_set(void *ptr, const double *val) { Radtran *r = as_rad(ptr); if (r) r->diurnal_fac = *val; }
void radtran_ir_get(void *ptr, void **ptr1) { Radtran *r = as_rad(ptr); *ptr1 = r ? (void *)&r->ir : nullptr; }
void radtran_sol_get(void *ptr, void **ptr1) { Radtran *r = as_rad(ptr); *ptr1 = r ? (void *)&r->sol : nullptr; }
void radtran_wrk_ir_get(void *ptr, void **ptr1) { Radtran *r = as_rad(ptr); *ptr1 = r ? (void *)&r->wrk_ir : nullptr; }
void radtran_wrk_sol_get(void *ptr, void **ptr1) { Radtran *r = as_rad(ptr); *ptr1 = r ? (void *)&r->wrk_sol : nullptr; }
void radtran_f_total_get_size(void *ptr, int *dim1) { Radtran *r = as_rad(ptr); *dim1 = r ? r->nz + 1 : 0; }
void radtran_f_total_get(void *ptr, const int *dim1, double *arr) {
  Radtran *r = as_rad(ptr);
  if (!r || r->state != 2) return;
  try {
    fetch_small(r);
    for (int i = 0; i < *dim1 && i < r->nz + 1; i++) arr[i] = r->h_small[r->rows.f_total + i];
  } catch (const HipFail &f) {
    defer_err(r, f.msg);   // no `err` here (clima/fortran/Radtran.f90 getters have none): radtran_synchronize reports it
  } catch (...) {
    defer_err(r, "radtran_f_total_get failed");
  }
}
void radtran_photons_sol_get_size(void *ptr, int *dim1) { Radtran *r = as_rad(ptr); *dim1 = r ? (int)r->photons_sol.size() : 0; }
void radtran_photons_sol_get(void *ptr, const int *dim1, double *arr) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  for (int i = 0; i < *dim1 && i < (int)r->photons_sol.size(); i++) arr[i] = r->photons_sol[i];
}

// extents of a handle (whatever built it): layers, gases, particles, opacity bins, g-points
void radtran_dims_get(void *ptr, int *nz, int *nsp, int *np, int *nw, int *ngauss) {
  Radtran *r = as_rad(ptr);
  *nz = r ? r->nz : 0; *nsp = r ? r->nsp : 0; *np = r ? r->np : 0; *nw = r ? r->nw : 0; *ngauss = r ? r->ng : 0;
}
// the species / particle names the handle holds (radtran_set_names), newline-separated, into caller buffers of `cap` bytes
void radtran_names_get(void *ptr, const int *cap, char *species_names, char *particle_names) {
  Radtran *r = as_rad(ptr);
  auto put = [&](const std::vector<std::string> &v, char *out) {
    std::string o;
    for (size_t i = 0; i < v.size(); i++) o += (i ? "\n" : "") + v[i];
    std::strncpy(out, o.c_str(), (size_t)std::max(*cap - 1, 0));
    if (*cap > 0) out[*cap - 1] = 0;
  };
  if (r) { put(r->species_names, species_names); put(r->particle_names, particle_names); }
  else if (*cap > 0) { species_names[0] = 0; particle_names[0] = 0; }
}

// Test hook: FNV-1a (64 bit) over the handle's HOST-side tables in the order they were handed over -- metadata as
// int32, values as float64 bytes.  The from-files loader (radtran_loader.hip) is held to clima_amd/data_loader.py with
// it where there is no device: identical tables <=> identical digests (tests/test_loader_cabi.py).
void clima_test_host_tables_digest(void *ptr, unsigned long long *digest) {
  // digest[0..7]: extents + opacity grid | k-tables | CIA | Rayleigh | absorption / photolysis | continuum | particles |
  // channels + stellar photons (each hash starts afresh: a difference names its group)
  Radtran *r = as_rad(ptr);
  unsigned long long h = 0;
  auto start = [&] { h = 1469598103934665603ULL; };
  auto bytes = [&](const void *p0, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p0);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ULL; }
  };
  auto ints = [&](std::initializer_list<int> v) { for (int x : v) bytes(&x, sizeof(int)); };
  auto vals = [&](const std::vector<double> &v) { if (!v.empty()) bytes(v.data(), v.size() * sizeof(double)); };
  for (int g = 0; g < 8; g++) digest[g] = 0;
  if (!r) return;
  start(); ints({r->nz, r->nsp, r->np, r->nw}); vals(r->wavl); digest[0] = h;
  start();
  for (auto *k : r->k) { ints({k->sp, k->ng, k->nP, k->nT}); vals(k->weights); vals(k->log10P); vals(k->temp); vals(k->log10k); }
  digest[1] = h;
  int g = 2;
  for (auto *lst : {&r->cia, &r->ray, &r->pxs}) {
    start();
    for (auto *x : *lst) { ints({x->type, x->dim, x->sp1, x->sp2, x->nT}); vals(x->temp); vals(x->data); }
    digest[g++] = h;
  }
  start(); ints({r->has_cont ? 1 : 0, r->LH2O, r->cont_nT}); vals(r->cont_temp); vals(r->cont_H2O); vals(r->cont_foreign); digest[5] = h;
  start();
  for (auto *q : r->part) { ints({q->p_ind, q->nrad}); vals(q->radii); vals(q->w0); vals(q->qext); vals(q->gt); }
  digest[6] = h;
  start(); vals(r->ir.wavl); vals(r->sol.wavl); vals(r->photons_sol); digest[7] = h;
}

// ---- all per-bin spectra of the last call in one go ------------------------------------
// The reference's result holder is plain allocatables the caller reads after every call (clima_radtran.f90:11-25); a
// host that does the same through the seven reference-named getters pays seven synchronous copies to pageable memory
// (6.7 MB at ~12 GB/s: 530 of a 648 us call at config 2).  Here the caller's seven arrays are page-locked on first
// use (hipHostRegister; they stay so until the handle is destroyed or radtran_spectra_release) and filled by seven
// asynchronous copies on the handle's stream and ONE synchronise.  An array that cannot be registered is still
// filled (staged by the runtime, slower).  do_solar false: the IR channel's three arrays only.
static void register_host(Radtran *r, void *p, size_t bytes) {
  if (!p || !bytes) return;
  for (auto &e : r->host_registered)
    if (e.first == p && e.second >= bytes) return;
  for (auto it = r->host_registered.begin(); it != r->host_registered.end(); ++it)
    if (it->first == p) { (void)hipHostUnregister(p); r->host_registered.erase(it); break; }   // (re-allocated larger at the same address)
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) r->host_registered.emplace_back(p, bytes);
  else (void)hipGetLastError();
}
static bool host_is_registered(const Radtran *r, const void *p, size_t bytes) {
  for (auto &e : r->host_registered)
    if (e.first == p && e.second >= bytes) return true;
  return false;
}
void radtran_spectra_get_all(void *ptr, const bool *do_solar, const int *nlev, const int *nw_ir, const int *nw_sol,
                             double *ir_fup_a, double *ir_fdn_a, double *ir_tau_band,
                             double *sol_fup_a, double *sol_fdn_a, double *sol_amean, double *sol_tau_band, char *err) {
  err[0] = 0;
  GUARD(r, ptr, err)
  TRY
  if (r->state != 2) throw HipFail{"radtran_spectra_get_all: the handle is not constructed"};
  if (*nlev != r->nz + 1 || *nw_ir != r->ir.nw || *nw_sol != r->sol.nw)
    throw HipFail{"radtran_spectra_get_all: array extents do not match the handle (nz+1, ir%nw, sol%nw)"};
  if (!r->holds.rows_on_host) settle(r);   // (after a synchronous call the results are final already)
  struct Job { double *dst; DevBuf<double> *src; };
  Job jobs[7] = {{ir_fup_a, &r->wrk_ir.fup_a}, {ir_fdn_a, &r->wrk_ir.fdn_a}, {ir_tau_band, &r->wrk_ir.tau_band},
                 {sol_fup_a, &r->wrk_sol.fup_a}, {sol_fdn_a, &r->wrk_sol.fdn_a}, {sol_amean, &r->wrk_sol.amean},
                 {sol_tau_band, &r->wrk_sol.tau_band}};
  const int n = *do_solar ? 7 : 3;
  for (int i = 0; i < n; i++) register_host(r, jobs[i].dst, jobs[i].src->n * sizeof(double));
  // the results are final (settled above): the copies need no ordering among themselves and go out over four
  // queues -- one copy engine sustains ~34 GB/s of the link, several of them more
  HIPCHK(hipStreamSynchronize(r->stream));
  for (auto &cs : r->copy_streams)
    if (!cs) HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipStream_t qs[4] = {r->stream, r->copy_streams[0], r->copy_streams[1], r->copy_streams[2]};
  const int order[7] = {3, 4, 5, 0, 1, 6, 2};   // the four large solar / IR arrays first, one per queue
  int q = 0;
  for (int k = 0; k < 7; k++) {
    const int i = order[k];
    if (i >= n || !jobs[i].dst || !jobs[i].src->n) continue;
    HIPCHK(hipMemcpyAsync(jobs[i].dst, jobs[i].src->p, jobs[i].src->n * sizeof(double), hipMemcpyDeviceToHost, qs[q & 3]));
    q++;
  }
  for (int k = 0; k < 4; k++) HIPCHK(hipStreamSynchronize(qs[k]));
  CATCH(err)
}
void radtran_batch_pin_results_set(void *ptr, const int *flag) {
  Radtran *r = as_rad(ptr);
  if (r && r->batch_pin_results != (*flag != 0)) { r->batch_pin_results = *flag != 0; r->batch_out_n = 0; }
}
void radtran_batch_pin_results_get(void *ptr, int *flag) {
  Radtran *r = as_rad(ptr);
  *flag = r && r->batch_pin_results ? 1 : 0;
}
void radtran_spectra_release(void *ptr) {
  Radtran *r = as_rad(ptr);
  if (!r) return;
  for (auto &e : r->host_registered) (void)hipHostUnregister(e.first);
  r->host_registered.clear();
  r->batch_out_n = 0;
}

// ---- ClimaRadtranWrk (clima/fortran/ClimaRadtranWrk.f90) ------------------------------
static int ch_nw(WrkObj *w) { return w->which ? w->parent->sol.nw : w->parent->ir.nw; }
#define WRK2D(name, field, rows)                                                          \
  void climaradtranwrk_##name##_get_size(void *ptr, int *dim1, int *dim2) {               \
    WrkObj *w = reinterpret_cast<WrkObj *>(ptr);                                          \
    *dim1 = w->parent->nz + (rows);                                                       \
    *dim2 = ch_nw(w);                                                                     \
  }                                                                                       \
  void climaradtranwrk_##name##_get(void *ptr, const int *dim1, const int *dim2, double *arr) { \
    WrkObj *w = reinterpret_cast<WrkObj *>(ptr);                                          \
    try { get2d(w, w->field, *dim1, *dim2, arr); }                                        \
    catch (const HipFail &f) { defer_err(w->parent, f.msg); }                             \
    catch (...) { defer_err(w->parent, "climaradtranwrk getter failed"); }                \
  }
WRK2D(fup_a, fup_a, 1)
WRK2D(fdn_a, fdn_a, 1)
WRK2D(amean, amean, 1)
WRK2D(tau_band, tau_band, 0)
#define WRK1D(name, up)                                                                   \
  void climaradtranwrk_##name##_get_size(void *ptr, int *dim1) {                          \
    WrkObj *w = reinterpret_cast<WrkObj *>(ptr);                                          \
    *dim1 = w->parent->nz + 1;                                                            \
  }                                                                                       \
  void climaradtranwrk_##name##_get(void *ptr, const int *dim1, double *arr) {            \
    WrkObj *w = reinterpret_cast<WrkObj *>(ptr);                                          \
    Radtran *r = w->parent;                                                               \
    try {                                                                                 \
      fetch_small(r);                                                                     \
      const int nl = r->nz + 1;                                                           \
      const int a = (w->which ? 2 : 0) + ((up) ? 0 : 1);                                  \
      for (int i = 0; i < *dim1 && i < nl; i++) arr[i] = r->h_small[r->rows.row(a) + i];  \
    } catch (const HipFail &f) { defer_err(r, f.msg);                                     \
    } catch (...) { defer_err(r, "climaradtranwrk getter failed"); }                      \
  }
WRK1D(fup_n, 1)
WRK1D(fdn_n, 0)

// ---- RTChannel (clima/fortran/RTChannel.f90) ------------------------------------------
void rtchannel_wavl_get_size(void *ptr, int *dim1) { *dim1 = (int)reinterpret_cast<ChannelObj *>(ptr)->wavl.size(); }
void rtchannel_wavl_get(void *ptr, const int *dim1, double *arr) {
  ChannelObj *c = reinterpret_cast<ChannelObj *>(ptr);
  for (int i = 0; i < *dim1 && i < (int)c->wavl.size(); i++) arr[i] = c->wavl[i];
}
void rtchannel_freq_get_size(void *ptr, int *dim1) { *dim1 = (int)reinterpret_cast<ChannelObj *>(ptr)->freq.size(); }
void rtchannel_freq_get(void *ptr, const int *dim1, double *arr) {
  ChannelObj *c = reinterpret_cast<ChannelObj *>(ptr);
  for (int i = 0; i < *dim1 && i < (int)c->freq.size(); i++) arr[i] = c->freq[i];
}

}  // extern "C"
