/*
 * clima_radtran_hip.h -- C ABI of the MI355X-native Radtran hot path.
 *
 * Drop-in boundary for Clima's `type Radtran` (src/radtran/clima_radtran.f90:31-85) and the
 * bind(c) shim above it (clima/fortran/Radtran.f90, ClimaRadtranWrk.f90, RTChannel.f90).
 * Conventions are the reference's (clima/fortran/clima_c_api.f90:5, AdiabatClimate.f90:169-190):
 *   - handles are opaque `void*` passed BY VALUE; every scalar is passed BY REFERENCE;
 *   - arrays are bare pointers with explicit extents; 2-D arrays are column-major;
 *   - errors: `char err[CLIMA_ERR_LEN+1]`, err[0]==0 <=> success; message text is API;
 *   - species / particle indices are 1-based (Fortran `sp_ind`, `p_ind`);
 *   - the object is not thread-safe; calls on one handle are serialised on its HIP stream.
 * No torch / C++ types cross this boundary.  All symbols are implemented by
 * clima_amd/csrc/libclima_radtran_hip.so; there is no CPU fallback: every entry point
 * that needs the GPU fails with a message in `err` when HIP is unavailable.
 */
#ifndef CLIMA_RADTRAN_HIP_H
#define CLIMA_RADTRAN_HIP_H

#ifndef __cplusplus
#include <stdbool.h>  /* logical(c_bool) <-> bool (1 byte), clima/fortran/Radtran.f90:211-227 */
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define CLIMA_ERR_LEN 1024

/* Xsection kinds: enum at src/radtran/clima_radtran_types.f90:40-42 */
#define CLIMA_XS_CIA 0
#define CLIMA_XS_RAYLEIGH 1
#define CLIMA_XS_ABSORPTION 2
#define CLIMA_XS_PHOTOLYSIS 3

/* ------------------------------------------------------------------------------------
 * Construction.  Replaces create_Radtran_2 (src/radtran/clima_radtran.f90:128-219): the
 * HDF5/YAML loaders (clima_radtran_types_create.f90) stay on the host side of the
 * boundary and hand over the tables they produce.
 * ---------------------------------------------------------------------------------- */

/* allocate / free an empty handle (pattern of allocate_adiabatclimate /
 * deallocate_adiabatclimate, clima/fortran/AdiabatClimate.f90:7-22) */
void allocate_radtran(void **ptr);
void deallocate_radtran(void *ptr);

/* nz layers, nsp gases (rad%ng), np particles, nw opacity bins, wavl[nw+1] nm ascending
 * (OpticalProperties%wavl, clima_radtran_types.f90:96-99) */
void radtran_create_begin(void *ptr, const int *nz, const int *nsp, const int *np,
                          const int *nw, const double *wavl, char *err);
/* Ktable (clima_radtran_types.f90:23-38).  log10k is the on-disk array
 * log10k(ngauss,npress,ntemp,nwav), column-major (types_create.f90:1349-1358). */
void radtran_add_ktable(void *ptr, const int *sp_ind, const int *ngauss,
                        const double *weights, const int *npress, const double *log10P,
                        const int *ntemp, const double *temp, const double *log10k,
                        char *err);
/* Xsection (clima_radtran_types.f90:44-55) after regridding to the bin grid
 * (types_create.f90:1171-1257): dim 0 -> data(nw) = xs; dim 1 -> data(ntemp,nw) = log10 xs.
 * sp_ind2 is used by CIA only. */
void radtran_add_xsection(void *ptr, const int *xs_type, const int *dim, const int *sp_ind1,
                          const int *sp_ind2, const int *ntemp, const double *temp,
                          const double *data, char *err);
/* WaterContinuum (clima_radtran_types.f90:68-77): log10_xs_*(ntemp,nw) */
void radtran_set_water_continuum(void *ptr, const int *LH2O, const int *ntemp,
                                 const double *temp, const double *log10_xs_H2O,
                                 const double *log10_xs_foreign, char *err);
/* ParticleXsection (clima_radtran_types.f90:57-66): w0,qext,gt (nrad,nw) */
void radtran_add_particle(void *ptr, const int *p_ind, const int *nrad, const double *radii,
                          const double *w0, const double *qext, const double *gt, char *err);
/* RTChannel edges in nm; index ranges resolved like create_RTChannel
 * (types_create.f90:226-270), same error text on mismatch. */
void radtran_set_channels(void *ptr, const int *n_ir_edges, const double *ir_wavl,
                          const int *n_sol_edges, const double *sol_wavl, char *err);
/* rad%photons_sol(sol%nw), mW/m^2/Hz -- output of read_stellar_flux (types_create.f90:9-78) */
void radtran_set_photons_sol(void *ptr, const int *n, const double *photons_sol, char *err);
/* zenith angles (Gauss-Legendre, clima_eqns.f90:26-41), albedo/emissivity defaults,
 * result arrays (clima_radtran.f90:162-217); uploads the tables to HBM. */
void radtran_create_end(void *ptr, const int *num_zenith_angles, const double *surface_albedo,
                        char *err);

/* ------------------------------------------------------------------------------------
 * The path.  The reference exposes no C symbol for Radtran%radiate itself (it is reached
 * through adiabatclimate_* only); these two are the ones a maintainer binds instead.
 * ---------------------------------------------------------------------------------- */

/* Radtran%radiate (clima_radtran.f90:221-318).  densities(dim1_d,dim2_d),
 * pdensities(dim1_p,dim2_p), radii(dim1_r,dim2_r) column-major; pass has_particles=0 and NULLs
 * when the optional arguments are absent.  Dimension errors reproduce check_inputs (:417-491),
 * including the separate `"radii" has the wrong input dimension.` of check_dimensions_p (:459). */
void radtran_radiate_wrapper(void *ptr, const double *T_surface, const int *dim_T,
                             const double *T, const int *dim_P, const double *P,
                             const int *dim1_d, const int *dim2_d, const double *densities,
                             const int *dim_dz, const double *dz, const int *has_particles,
                             const int *dim1_p, const int *dim2_p, const double *pdensities,
                             const int *dim1_r, const int *dim2_r, const double *radii,
                             const int *compute_solar,
                             const int *compute_opacity, char *err);
/* Radtran%TOA_fluxes (clima_radtran.f90:320-342) */
void radtran_toa_fluxes_wrapper(void *ptr, const double *T_surface, const int *dim_T,
                                const double *T, const int *dim_P, const double *P,
                                const int *dim1_d, const int *dim2_d, const double *densities,
                                const int *dim_dz, const double *dz, const int *has_particles,
                                const int *dim1_p, const int *dim2_p, const double *pdensities,
                                const int *dim1_r, const int *dim2_r, const double *radii,
                                const int *compute_solar,
                                const int *compute_opacity, double *ISR, double *OLR,
                                char *err);
/* Radtran%apply_radiation_enhancement (clima_radtran.f90:402-411) */
void radtran_apply_radiation_enhancement(void *ptr, const double *rad_enhancement);
/* clima/fortran/Radtran.f90:77-118 (same names and argument lists): custom optical properties,
 * wv nm, P dynes/cm^2 decreasing, dtau_dz / w0 / g0 (size(P), size(wv)) column-major
 * (src/radtran/clima_radtran_types.f90:432-548) */
void radtran_set_custom_optical_properties(void *ptr, const int *dim_wv, const double *wv, const int *dim_P,
                                           const double *P, const int *dim1_dtau_dz, const int *dim2_dtau_dz,
                                           const double *dtau_dz, const int *dim1_w0, const int *dim2_w0,
                                           const double *w0, const int *dim1_g0, const int *dim2_g0,
                                           const double *g0, char *err);
void radtran_unset_custom_optical_properties(void *ptr);

/* ---- HBM-resident form of the same call (no PCIe inside the timed region) ----
 * upload_column copies the column into the handle's device buffers; radiate_resident
 * enqueues opacity + IR + solar + integration on the handle's stream and returns without
 * a host sync; synchronize waits and surfaces device-side failures (e.g. the particle
 * radius clamp of interpolate_Particle, clima_radtran_types.f90:973-976). */
void radtran_upload_column(void *ptr, const double *T_surface, const double *T, const double *P,
                           const double *densities, const double *dz, const double *pdensities,
                           const double *radii, char *err);
void radtran_radiate_resident(void *ptr, const int *compute_solar, const int *compute_opacity,
                              char *err);
void radtran_synchronize(void *ptr, char *err);
/* device pointer to the packed level fluxes [ir_up, ir_dn, sol_up, sol_dn][nz+1] (f64):
 * the buffer a bin-sharded run all-reduces over RCCL. */
void radtran_flux_device_ptr(void *ptr, void **dptr, int *count);
/* restrict this handle to opacity bins of shard `rank` out of `world` (work-balanced
 * contiguous ranges; rank 0-based).  world=1 restores the full grid.  The stored optical properties stay what they
 * were: a call on them (compute_opacity = 0, radtran_radiate_ir_batch, the Jacobians, radtran_opr_get) runs where they
 * were computed for every bin of the new shard -- an unsharded pass, then a shard -- and otherwise refuses
 * ("... needs opacities: call radiate with compute_opacity first"). */
void radtran_set_bin_shard(void *ptr, const int *rank, const int *world, char *err);
/* the ranges this handle owns: first opacity bin / count (0-based), then the channel-local
 * IR and solar sub-ranges */
void radtran_bin_shard_get(void *ptr, int *op_lo, int *op_n, int *ir_lo, int *ir_n, int *sol_lo,
                           int *sol_n);
/* after an external all-reduce of the flux buffer: the level rows have changed; f_total is formed
 * from them when the results are next read */
void radtran_finish_reduced(void *ptr, char *err);

/* ---- The multi-GPU step owned by the library (bins shard over the GPUs of a node, one RCCL
 * all-reduce of the per-layer integrated fluxes).  One process per GPU; every rank constructs the same Radtran
 * (after radtran_set_device) and joins a communicator.  From then on radtran_radiate_wrapper /
 * radtran_toa_fluxes_wrapper / radtran_radiate_resident work on the rank's own spectral bins and end with ONE
 * ncclAllReduce (sum, f64, 4 (nz+1) + 1 values) enqueued on the handle's stream: the level fluxes, f_total, ISR
 * and OLR every rank reads are those of the whole spectrum; per-bin spectra stay sharded (zeros outside the
 * rank's bins).  What is distributed is the sum over bins of src/radtran/clima_radtran_radiate.f90:184-192 and
 * f_total of clima_radtran.f90:287, 316.  A fused hand-off timeout on any rank is repeated by all of them
 * (the flag travels on the same all-reduce), never reported as an error. */
#define CLIMA_COMM_ID_BYTES 128   /* = NCCL_UNIQUE_ID_BYTES */
/* select the HIP device of this process (before radtran_create_end) */
void radtran_set_device(const int *device, char *err);
/* rank 0: a fresh communicator id, to be handed to every rank by the caller's own means (MPI_Bcast, a file ...) */
void radtran_comm_unique_id(char *id /* [CLIMA_COMM_ID_BYTES] */, char *err);
/* collective over the nranks processes; also restricts the handle to the bins of shard (rank, nranks) */
void radtran_comm_init_rank(void *ptr, const int *nranks, const int *rank, const char *id, char *err);
/* the same with the id exchanged through a file that rank 0 creates (hosts without a message layer);
 * `path` (NUL-terminated) must be new for every job (a file older than ten minutes is taken for a leftover and ignored) */
void radtran_comm_init_file(void *ptr, const int *nranks, const int *rank, const char *path, char *err);
/* nranks (0: no communicator), rank, all-reduces enqueued so far */
void radtran_comm_get(void *ptr, int *nranks, int *rank, int *reduces);
/* leave the communicator; the handle works on the whole spectrum again */
void radtran_comm_destroy(void *ptr);
/* Column batch (BASELINE.json config 4): ncol independent Radtran%TOA_fluxes calls
 * (src/radtran/clima_radtran.f90:320-342), moved to HBM in one copy and enqueued back to back.
 * Inputs as radtran_toa_fluxes_wrapper with the column as the last dimension: T, P, dz (nz, ncol),
 * densities (nz, nsp, ncol), pdensities / radii (nz, np, ncol), T_surface (ncol).  ISR, OLR (ncol);
 * fluxes (nz+1, 5, ncol) = ir up, ir down, solar up, solar down, f_total, or NULL.
 * Afterwards the handle holds the last column's level rows and spectra.  Where the batch ran one launch per chunk its
 * optical properties stayed in the batch's own memory: a call with compute_opacity = 0, radtran_radiate_ir_batch and the
 * Jacobians then refuse ("... needs opacities: call radiate with compute_opacity first") until a compute_opacity call. */
void radtran_toa_fluxes_batch(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                              const double *densities, const double *dz, const int *has_particles,
                              const double *pdensities, const double *radii, double *ISR, double *OLR,
                              double *fluxes, char *err);
/* The same batch with every array in device memory of the handle's device (f64, dense, same shapes and order):
 * nothing is staged on the host -- the column blocks and the pair-reuse tables are built, and f_total / ISR / OLR
 * formed, by kernels -- and the call RETURNS WITHOUT WAITING for the device.  d_fluxes may be NULL.
 * producer_stream: the HIP stream on which the caller's writes of the inputs were enqueued (the library records an
 * event on it and makes the handle's stream, radtran_stream_get, wait for that event; the host is not
 * synchronised), or NULL when the inputs are complete.
 * The results are final when the next radtran_synchronize returns with `err` empty; inputs and outputs must stay
 * allocated until then: a fused hand-off wait that expired in the batch is found there, and the batch is then
 * computed again through the separate launches into the SAME output arrays (radtran_fused_fallbacks_get + 1); an
 * opacity failure is reported there with the reference's text.  Any later call on the handle that enqueues work or
 * reads results settles a pending batch first.  Bit for bit radtran_toa_fluxes_batch on the same columns; the handle
 * holds the last column afterwards, as there.  Refused with nothing enqueued: what the host batch refuses, a NULL
 * required array, an array that is not device memory of the handle's device (`"T" is not device memory ...`).
 * Configurations that run one call per column (at most 64 layers, g-point counts other than 8, ...) fetch the
 * columns' source-layer counts (4 bytes each) before enqueuing, which waits for the inputs. */
void radtran_toa_fluxes_batch_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                     const double *d_P, const double *d_densities, const double *d_dz,
                                     const int *has_particles, const double *d_pdensities, const double *d_radii,
                                     double *d_ISR, double *d_OLR, double *d_fluxes, const void *producer_stream,
                                     char *err);
/* Both batches with per-bin spectra of EVERY column (a plain batch keeps the last column's only, in the handle):
 * spec_level(nsel) lists levels 1..nz+1, ground-first (nz+1: the top of the atmosphere; row_level's convention in
 * radtran_ir_jacobian_reduced), in any order, repeats allowed.  ir_fup, ir_fdn (nw_ir, nsel, ncol) and sol_fup,
 * sol_fdn (nw_sol, nsel, ncol), the bin fastest and in the channel's own order (rtchannel_freq_get); any of them may
 * be NULL, not all four.  Element (l, a, c) of ir_fup is wrk_ir%fup_a(spec_level(a), l) as the handle would hold it
 * after column c's own TOA_fluxes call, same units -- copied out of the batch before its buffers are reused, not
 * recomputed, so bit for bit the value the batch's integration summed -- and likewise fdn_a / wrk_sol.  Everything
 * else is radtran_toa_fluxes_batch (radtran_toa_fluxes_batch_device): ISR, OLR, fluxes bit for bit, the handle left
 * holding the last column.  Device form: spec_level is a HOST array, read before the call returns; the spectrum
 * arrays are final, and after an expired hand-off wait refilled by the repeat, at the same radtran_synchronize as the
 * other results.  Refused with nothing enqueued: what the plain batch refuses, with its texts; nsel < 1; a level
 * outside 1..nz+1 (`spec_level(2) = 0 is outside 1..51`); all four arrays NULL; in the device form a spectrum array
 * that is not device memory of the handle's device (`toa_fluxes_batch_device: "ir_fup" is not device memory ...`).
 * After an opacity failure the spectrum arrays hold unspecified values, as fluxes does. */
void radtran_toa_fluxes_batch_spectra(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                      const double *densities, const double *dz, const int *has_particles,
                                      const double *pdensities, const double *radii, double *ISR, double *OLR,
                                      double *fluxes, const int *nsel, const int *spec_level, double *ir_fup,
                                      double *ir_fdn, double *sol_fup, double *sol_fdn, char *err);
void radtran_toa_fluxes_batch_spectra_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                             const double *d_P, const double *d_densities, const double *d_dz,
                                             const int *has_particles, const double *d_pdensities, const double *d_radii,
                                             double *d_ISR, double *d_OLR, double *d_fluxes, const int *nsel,
                                             const int *spec_level, double *d_ir_fup, double *d_ir_fdn, double *d_sol_fup,
                                             double *d_sol_fdn, const void *producer_stream, char *err);
/* The spectra batches with per-column surface, zenith and stellar scaling: five optional arrays, the column last --
 * surface_albedo (nw_sol, ncol), surface_emissivity (nw_ir, ncol), the bins in the channel's own order
 * (radtran_surface_albedo_get); zenith_u, zenith_weights (nzen, ncol), nzen the handle's; photon_scale_factor (ncol).
 * A NULL array: every column takes the handle's current value of that field.  Column c is TOA_fluxes on that column
 * after surface_albedo = surface_albedo(:, c), surface_emissivity, zenith_u, zenith_weights likewise and
 * photon_scale_factor = photon_scale_factor(c) had been set on the handle, bit for bit; diurnal_fac, has_hard_surface
 * and ir_tau_min are the handle's.  The values are used as given (the setters check nothing either).  The handle's own
 * fields are NOT changed by the call and not marked changed -- a later single call runs under them.
 * Afterwards the handle holds the last column's rows and spectra, and of the opacities what the plain batch leaves.
 * nsel = 0 (spec_level and the four spectrum arrays then unread, NULL will do): no spectra, unlike the spectra batches.
 * Device form: the five arrays are device memory as well; everything else is
 * radtran_toa_fluxes_batch_spectra_device, the repeat after an expired hand-off wait under the same bounds included.
 * Refused with nothing enqueued: what the plain batch refuses, with its texts; with nsel != 0 what the spectra batch
 * refuses; in the device form a given array that is not device memory of the handle's device
 * (`toa_fluxes_batch_device: "surface_albedo" is not device memory ...`). */
void radtran_toa_fluxes_batch_bounds(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                     const double *densities, const double *dz, const int *has_particles,
                                     const double *pdensities, const double *radii, double *ISR, double *OLR,
                                     double *fluxes, const double *surface_albedo, const double *surface_emissivity,
                                     const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                                     const int *nsel, const int *spec_level, double *ir_fup, double *ir_fdn,
                                     double *sol_fup, double *sol_fdn, char *err);
void radtran_toa_fluxes_batch_bounds_device(void *ptr, const int *ncol, const double *d_T_surface, const double *d_T,
                                            const double *d_P, const double *d_densities, const double *d_dz,
                                            const int *has_particles, const double *d_pdensities, const double *d_radii,
                                            double *d_ISR, double *d_OLR, double *d_fluxes, const double *d_surface_albedo,
                                            const double *d_surface_emissivity, const double *d_zenith_u,
                                            const double *d_zenith_weights, const double *d_photon_scale_factor,
                                            const int *nsel, const int *spec_level, double *d_ir_fup, double *d_ir_fdn,
                                            double *d_sol_fup, double *d_sol_fdn, const void *producer_stream, char *err);
/* test hooks: the bounds blocks (ncol * block_count doubles; blocks NULL: block_count alone) of a bounds batch given as
 * host arrays (any of them NULL), built by the device batch's kernel and by the host batch's pack_bounds */
void clima_test_pack_bounds(void *ptr, const int *ncol, const double *surface_albedo, const double *surface_emissivity,
                            const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                            double *blocks, int *block_count, char *err);
void clima_test_pack_bounds_host(void *ptr, const int *ncol, const double *surface_albedo, const double *surface_emissivity,
                                 const double *zenith_u, const double *zenith_weights, const double *photon_scale_factor,
                                 double *blocks, int *block_count, char *err);
/* test hooks: the column blocks (ncol * col_count doubles; blocks NULL: col_count alone) of a batch given as host
 * arrays, built by the device batch's kernel and by the host batch's pack_column */
void clima_test_pack_columns(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                             const double *densities, const double *dz, const int *has_particles, const double *pdensities,
                             const double *radii, double *blocks, int *col_count, char *err);
void clima_test_pack_columns_host(void *ptr, const int *ncol, const double *T_surface, const double *T, const double *P,
                                  const double *densities, const double *dz, const int *has_particles,
                                  const double *pdensities, const double *radii, double *blocks, int *col_count, char *err);
/* Batched shared-opacity IR calls: what the RCE Jacobian does one call at a time
 * (src/adiabat/clima_adiabat_solve.f90:798-812 -> clima_radtran.f90:221-318 with
 * compute_solar = compute_opacity = .false.).  T is (nz, ncol) column-major, T_surface (ncol);
 * column c receives that call's wrk_ir%fup_n, wrk_ir%fdn_n and f_total in (nz+1, ncol) arrays.
 * Uses the opacities of the last compute_opacity call and the solar fluxes of the last solar
 * call; the handle's own wrk_ir / f_total are left untouched.  On a handle with a communicator
 * (radtran_comm_init_rank) every rank passes the same columns, works on its share of the bins and the library
 * all-reduces the batch's up / down arrays once (2 (nz+1) ncol doubles) before f_total is formed: every rank
 * receives the whole result.  A bin shard without a communicator (radtran_set_bin_shard) is refused.
 * The results come back through the handle's pinned block, in pieces the host copies out while the next one is on the
 * link.  After radtran_batch_pin_results_set(handle, 1) a caller that passes the same three result arrays as in its
 * previous batch call (the Jacobian's work arrays) has them page-locked from that second call on, like the arrays of
 * radtran_spectra_get_all, and filled by the device directly (402 x 403: 0.66 instead of 0.80 ms): they must then stay
 * allocated until radtran_spectra_release or the handle's end.  Off by default. */
void radtran_radiate_ir_batch(void *ptr, const int *ncol, const double *T_surface, const int *dim1_T,
                              const int *dim2_T, const double *T, double *fup_n, double *fdn_n,
                              double *f_total, char *err);
/* Batched solar calls on shared opacities: many illumination cases of ONE atmosphere (an albedo as a function of zenith
 * angle, latitude bands, a surface-albedo sweep, an insolation loop).  Case c is radiate(..., compute_solar = .true.,
 * compute_opacity = .false.) (clima_radtran.f90:291-316) on the handle's stored optical properties, the handle taken as
 * constructed with `nzen` zenith angles, after zenith_u = zenith_u(:, c), zenith_weights = zenith_weights(:, c),
 * surface_albedo = surface_albedo(:, c) and photon_scale_factor = photon_scale_factor(c) had been set.
 *   zenith_u, zenith_weights  (nzen, ncol); nzen is the batch's own, 1 <= nzen <= 16, independent of the handle's (nzen =
 *                             1 with weight 1: one zenith angle per case)
 *   surface_albedo            (nw_sol, ncol), or NULL: the handle's current albedo in every case
 *   photon_scale_factor       (ncol), or NULL: the handle's current value.  diurnal_fac is always the handle's.  Values are
 *                             used as given.
 *   fup_n, fdn_n              (nz+1, ncol): that call's wrk_sol%fup_n, wrk_sol%fdn_n, ground-first
 *   f_total                   (nz+1, ncol) or NULL: (fdn_n - fup_n) plus the IR rows the handle holds from its last IR call
 *                             (as radtran_radiate_ir_batch uses the last solar rows)
 *   nsel, spec_level(nsel)    levels 1..nz+1 ground-first, any order, repeats allowed (the spectra batches' convention);
 *                             nsel = 0: no spectra, the arrays below are unread
 *   sol_fup, sol_fdn, sol_amean  (nw_sol, nsel, ncol), any of them NULL: element (l, a, c) is wrk_sol%fup_a(spec_level(a),
 *                             l) of case c (fdn_a, amean -- photons cm^-2 s^-1 -- likewise), in the same units
 * The handle's wrk_ir, wrk_sol, f_total, spectra, stored opacities and its five fields are left untouched.  Synchronous,
 * host arrays; the results come back as radtran_radiate_ir_batch's do, the cases run in chunks of 512 so that the
 * per-case spectra in device memory stay bounded.  Two forms give the same results to rounding: k_twostream_sol_batch
 * (nz <= 512), which does what the opacities alone decide once per (bin, g-point) and block of cases, and one full solve
 * per case by the stand-alone two-stream kernels (nz > 512, and whatever else the shared kernel does not cover).
 * Refused (err) with nothing enqueued, the text naming the argument and its value: a handle that is not constructed or
 * holds no opacities ("radiate_solar_batch needs opacities: ..."); a bin shard or a communicator ("needs the whole
 * spectrum": a multi-GPU form is out of scope); ncol < 1; nzen outside 1..16; NULL zenith_u, zenith_weights, fup_n or
 * fdn_n; f_total on a handle that holds no level rows; nsel < 0; nsel > 0 with NULL spec_level; a level outside 1..nz+1;
 * nsel > 0 with all three spectrum arrays NULL. */
void radtran_radiate_solar_batch(void *ptr, const int *ncol, const int *nzen, const double *zenith_u,
                                 const double *zenith_weights, const double *surface_albedo,
                                 const double *photon_scale_factor, double *fup_n, double *fdn_n, double *f_total,
                                 const int *nsel, const int *spec_level, double *sol_fup, double *sol_fdn,
                                 double *sol_amean, char *err);
/* ... its forms, for tests and measurements: on = 0 forces one full solve per case (default 1: the shared kernel where
 * it covers the shape); `batches` counts the batches that took the shared kernel. */
void radtran_solar_batch_shared_set(void *ptr, const int *on);
void radtran_solar_batch_shared_get(void *ptr, int *on, int *batches);
/* The exact IR temperature Jacobian of the level fluxes at fixed opacities: the limit, as the step goes to 0, of what
 * the RCE Jacobian's one-sided differences compute (src/adiabat/clima_adiabat_solve.f90:768-822), in one call.  For the
 * base profile T_surface, T (dim_T = nz) and the opacities of the last compute_opacity call, jac_up, jac_dn and
 * jac_total are (nz+1, nz+1) column-major (dim1 = dim2 = nz+1):
 *   jac_up(i, j) = d wrk_ir%fup_n(i) / d x(j),  jac_dn(i, j) = d wrk_ir%fdn_n(i) / d x(j),  jac_total = jac_dn - jac_up
 * with x(1) = T_surface, x(1+m) = T(m) (the reference's T_in order) and i the level, ground-first; mW m^-2 K^-1.  Each
 * column is the derivative of radiate(..., compute_solar = .false., compute_opacity = .false.) (clima_radtran.f90:221-318),
 * both surface forms, per-bin emissivity and thin layers (ir_tau_min) included; solar terms do not depend on T at
 * fixed opacity.  Built on radtran_radiate_ir_batch's response form (two_stream_ir is linear in the Planck values):
 * the opacity-only part, then every level one deviation whose amplitude is dnu dB/dT at its base temperature -- no
 * base solve, no step.  A convective zone's column is the sum of its levels' columns.  The handle's wrk_ir, wrk_sol,
 * f_total and spectra are left untouched.  Refused (err): a handle that is not constructed or has no opacities yet,
 * wrong extents ("jac has the wrong dimension"), a temperature that is not finite and positive, a bin shard without a
 * communicator, and shapes outside the response form's range -- 4 <= nz <= 512, at most 65535 (bin, g-point) pairs,
 * work arrays of at most 16 GB.  On a handle with a communicator (radtran_comm_init_rank) every rank passes the same
 * profile and works on its bins (a rank without IR bins contributes zeros); one all-reduce of the up and down matrices
 * (2 (nz+1)^2 doubles) precedes jac_total, and every rank receives the whole result. */
void radtran_ir_jacobian(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                         const int *dim1, const int *dim2, double *jac_up, double *jac_dn, double *jac_total, char *err);
/* radtran_ir_jacobian in the unknowns of the RCE solver (AdiabatClimate_jacobian_from_base,
 * src/adiabat/clima_adiabat_solve.f90:768-822), in one call.  That caller moves several x at once with one unknown --
 * the two copies of a layer on the doubled radiative grid and the two ghost layers above the top one
 * (src/adiabat/clima_adiabat.f90:729-773), a whole convective zone with its lower unknown -- reads f_total at some
 * levels only (every other one on the doubled grid, clima_adiabat_solve.f90:731-733) and needs the net flux alone.
 *   group_of_x (dim_x = nz+1): one entry per x of radtran_ir_jacobian (x(1) = T_surface, x(1+m) = T(m));
 *                              0 = held fixed, g in 1..ngroup = moves with unknown g
 *   row_level (nrow):          levels 1..nz+1, ground-first, in any order, repeats allowed
 *   jac_up, jac_dn, jac_total: (nrow, ngroup) column-major, dim1 = nrow, dim2 = ngroup; jac_up and jac_dn may both be
 *                              NULL (the total alone is written and copied), jac_total is required
 *   jac_up(a, g) = sum over the j with group_of_x(j) = g, in ascending j, of J_up(row_level(a), j), J_up the matrix
 *   radtran_ir_jacobian returns for the same handle state; jac_dn likewise; jac_total = jac_dn - jac_up.
 * The sums are formed on the device in exactly that order, entry by entry as radtran_ir_jacobian forms them, so the
 * result is bit for bit the caller's own loop over the full matrices -- which are never written, copied or reduced:
 * (nrow, ngroup) doubles per requested matrix come back instead of 3 (nz+1)^2.  The handle's wrk_ir, wrk_sol, f_total
 * and spectra are left untouched.  Refused (err): everything radtran_ir_jacobian refuses, with its texts; and, each
 * naming the index and the value, a group_of_x of the wrong dimension, an entry outside 0..ngroup, a group without a
 * member, a row outside 1..nz+1, nrow or ngroup below 1, only one of jac_up and jac_dn; wrong dim1 or dim2:
 * "jac has the wrong dimension".  On a handle with a communicator every rank passes the same map; one all-reduce of the
 * reduced up and down matrices (2 nrow ngroup doubles) precedes jac_total. */
void radtran_ir_jacobian_reduced(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                 const int *dim_x, const int *group_of_x, const int *ngroup,
                                 const int *nrow, const int *row_level,
                                 const int *dim1, const int *dim2,
                                 double *jac_up, double *jac_dn, double *jac_total, char *err);
/* Rows of the same derivative BEFORE the sum over the bins: the spectral contribution function of the emission spectrum
 * and spectral radiative kernels dOLR_nu / dT(p) at the top, the downward flux's at the surface.
 *   row_level (nrow):   levels 1..nz+1, ground-first, in any order, repeats allowed (radtran_ir_jacobian_reduced's)
 *   jac_up_a, jac_dn_a: (nw_ir, nrow, nz+1) column-major, the bin fastest and in the channel's own order
 *                       (rtchannel_freq_get); dim1 = nw_ir, dim2 = nrow, dim3 = nz+1.  Either may be NULL, not both.
 *   jac_up_a(l, a, j) = d wrk_ir%fup_a(row_level(a), l) / d x(j), x(1) = T_surface, x(1+m) = T(m) (radtran_ir_jacobian's
 *   x); jac_dn_a likewise with fdn_a; mW m^-2 Hz^-1 K^-1.
 * The derivative of radiate(..., compute_solar = .false., compute_opacity = .false.) on the stored opacities at the base
 * profile T_surface, T, as this library computes that call: both surface forms, per-bin emissivity and thin layers
 * (ir_tau_min) included; the library's IR solve does not read the zenith weights (the constructor's sum to 1, which is
 * what clima_radtran_radiate.f90:83-134 multiplies the IR fluxes by), and neither does this call.  The amplitude at level k is dB/dT(avg_freq(l), T_k), NOT times the bin's width; the g-points
 * are summed with wbin in g order, so the result is bitwise repeatable.  Contract:
 *   sum over l of jac_up_a(l, a, j) (freq(l) - freq(l+1)) is jac_up(row_level(a), j) of radtran_ir_jacobian (to
 *   rounding: another algorithm); the same for dn;
 *   the dn row of level nz+1 is exactly 0.0 (fdn(1) = 0, clima_radtran_twostream.f90:289);
 *   without a hard surface the emissivity is not read.
 * Not the response form: two_stream_ir solves M Y = E with E linear in the Planck values and every level flux is
 * c . Y + s . bplanck, so ONE transposed tridiagonal solve M^T lambda = c per (bin, g-point, row, direction) gives the
 * whole row (clima_amd/csrc/ir_adjoint.inc).  Every nz >= 1 and every g-point count of the single call; what bounds the
 * call is its work buffer, 8 NQ ((4 + nfun) 2 nz + nfun (nz+1)) bytes for NQ (bin, g-point) pairs and nfun = nrow x
 * directions functionals, at most 4 GiB.  Synchronous, host arrays.  The handle's wrk_ir, wrk_sol, f_total, spectra,
 * stored opacities and fields are left untouched.  Refused (err; nothing is enqueued, the argument and its value are
 * named): a handle that is not constructed; one without opacities ("ir_jacobian_spectral_rows needs opacities: ...");
 * a bin shard or a communicator ("needs the whole spectrum"); dim_T /= nz ('"T" has the wrong input dimension.');
 * wrong dim1..3 ("jac has the wrong dimension"); nrow < 1; a NULL row_level; a level outside 1..nz+1; both arrays
 * NULL; a temperature that is not finite and positive; a work buffer above the bound. */
void radtran_ir_jacobian_spectral_rows(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                       const int *nrow, const int *row_level,
                                       const int *dim1, const int *dim2, const int *dim3,
                                       double *jac_up_a, double *jac_dn_a, char *err);
/* Per-bin IR spectra of MANY temperature profiles on the stored opacities, at chosen levels: column c is
 * radiate(T_surface(c), T(:, c), ..., compute_solar = .false., compute_opacity = .false.) read at wrk_ir%fup_a / fdn_a
 * (spec_level(a), l) -- day / night or latitude profiles of one atmosphere, a Monte-Carlo spread of a retrieved T(p), an
 * OLR(T_surface) sweep at fixed opacity -- without a solve per column.
 *   T (nz, ncol) column-major, T_surface (ncol): as in radtran_radiate_ir_batch; dim1_T = nz, dim2_T = ncol
 *   spec_level (nsel):  levels 1..nz+1, ground-first, any order, repeats allowed (the spectra batches' convention)
 *   ir_fup, ir_fdn (nw_ir, nsel, ncol): the bin fastest and in rtchannel_freq_get order; element (l, a, c) is
 *                       wrk_ir%fup_a(spec_level(a), l) (fdn_a likewise) of column c, in its units, to rounding (another
 *                       algorithm than the single call's)
 *   fup_n, fdn_n (nsel, ncol): sum over l of ir_fup(l, a, c) (freq(l) - freq(l+1)), summed on the device in ascending l:
 *                       wrk_ir%fup_n(spec_level(a)) to rounding; available without ir_fup being given
 *   w_up, w_dn (nw_ir, nsel, nz+1): the weights, j ground-first in radtran_ir_jacobian's x order (x(1) = T_surface,
 *                       x(1+m) = T(m)):  ir_fup(l, a, c) = sum over j of w_up(l, a, j) B(avg_freq(l), x_c(j)) with B the
 *                       library's planck_fcn -- the temperature-independent weighting function of the emission spectrum
 * Any of the six outputs may be NULL, not all; the up direction is solved only if an up output is asked for, down
 * likewise.  ncol = 0 is allowed when only w_* are asked for (T and T_surface are then unread).
 * Method: at fixed opacities two_stream_ir is homogeneously linear in the Planck values of the levels (the surface term,
 * both surface forms and the thin-layer source rule included), so a level flux of a bin is a fixed row of weights times
 * Planck values.  The weights are radtran_ir_jacobian_spectral_rows' adjoint rows with unit amplitudes: ONE adjoint
 * pass per call (clima_amd/csrc/ir_adjoint.inc), then nw_ir (nz+1) Planck evaluations and as many FMAs per requested
 * row and column (clima_amd/csrc/ir_rows_apply.inc).  Contract:
 *   the dn outputs of level nz+1 are exactly 0.0 (w_dn too);
 *   a column's results do not depend on ncol or on the other columns, bit for bit;
 *   the call is bitwise repeatable (no atomics, fixed summation orders: j ascending, then l ascending);
 *   w_up(l, a, j) dB/dT(avg_freq(l), x(j)) is radtran_ir_jacobian_spectral_rows' jac_up_a(l, a, j) at the same T, to
 *   rounding; the same for dn;
 *   without a hard surface the emissivity is not read; the zenith weights are not read, as in the library's IR solve.
 * Synchronous, host arrays; columns run in chunks of at most 512 (fewer where a chunk's spectra would exceed 256 MiB) and
 * results come back through the handle's pinned block.  The handle's wrk_ir, wrk_sol, f_total, spectra, stored
 * opacities and fields are left untouched; a pending deferred integration is settled first.  Every nz >= 1 and every
 * g-point count of the single call.  Refused (err; nothing is enqueued, the argument and its value are named): a handle
 * that is not constructed; one without opacities ("ir_spectra_batch needs opacities: ..."); a bin shard or a
 * communicator ("needs the whole spectrum"); dim1_T /= nz or dim2_T /= ncol ('"T" has the wrong input dimension.');
 * ncol < 0; ncol = 0 with a flux output asked for; nsel < 1; a NULL spec_level; a level outside 1..nz+1
 * ("spec_level(2) = 0 is outside 1..51"); all six outputs NULL; a NULL T or T_surface with ncol > 0; a temperature that
 * is not finite and positive ("T(i, c) = ..." or "T_surface(c) = ..."); an adjoint work buffer above
 * radtran_ir_jacobian_spectral_rows' 4 GiB bound. */
void radtran_ir_spectra_batch(void *ptr, const int *ncol, const double *T_surface,
                              const int *dim1_T, const int *dim2_T, const double *T,
                              const int *nsel, const int *spec_level,
                              double *ir_fup, double *ir_fdn, double *fup_n, double *fdn_n,
                              double *w_up, double *w_dn, char *err);
/* radtran_ir_spectra_batch for arrays that live in device memory, with the weights in the caller's keeping: every array
 * but spec_level (HOST, read before the call returns) is device memory of the handle's device, shapes and order as above
 * (T (nz, ncol) column-major is a C-contiguous (ncol, nz) tensor; the spectra (ncol, nsel, nw_ir); the weights
 * (nz+1, nsel, nw_ir)).  The call returns with its work enqueued on the handle's stream, behind the caller's writes of the
 * inputs on `producer_stream` (NULL: they are complete); the results are final at the next radtran_synchronize.  The
 * kernels are the host form's, writing straight into the caller's arrays (columns in launches of at most 262144; a sum
 * asked for without its spectrum stages that direction's spectra through the handle, in the host form's chunks): the
 * results are bit for bit the host form's on the same inputs.
 *   weights_given = 0: the adjoint pass runs on the stored opacities; a non-NULL d_w_up / d_w_dn receives the weights
 *                      (NULL: they stay in the handle, as in the host form).
 *   weights_given = 1: d_w_up / d_w_dn are INPUTS, the weights an earlier call computed with the same nsel and
 *                      spec_level; no adjoint pass runs and the handle needs no opacities -- the frequency grid is all the
 *                      call reads.  Results are bit for bit those of the call that computed them.  The caller owns the
 *                      validity of the weights: they describe the atmosphere, the emissivity, has_hard_surface and
 *                      ir_tau_min of the time they were computed; the library keeps no cache of them.
 * The temperatures are NOT checked (a check would need a host read): they are used as given, and a T that is not positive
 * or not finite gives whatever planck_fcn gives for it, without an error.
 * Refused, in the host form's words under the name ir_spectra_batch_device: what the host form refuses but for the
 * temperatures; an array that is not device memory of the handle's device ('"T" is not device memory of this handle's
 * device'); weights_given = 1 with a direction asked for whose w_* is NULL, or with no flux output at all.  Opacities are
 * needed with weights_given = 0 only.  The handle's state is left as the host form leaves it; a pending deferred
 * integration is settled first. */
void radtran_ir_spectra_batch_device(void *ptr, const int *ncol, const double *d_T_surface,
                                     const int *dim1_T, const int *dim2_T, const double *d_T,
                                     const int *nsel, const int *spec_level,
                                     double *d_ir_fup, double *d_ir_fdn, double *d_fup_n, double *d_fdn_n,
                                     double *d_w_up, double *d_w_dn, const int *weights_given,
                                     const void *producer_stream, char *err);
/* The temperature gradient of radtran_ir_spectra_batch (a vector-Jacobian product): for cotangents g_ir_fup / g_ir_fdn
 * (nw_ir, nsel, ncol) of the spectra and g_fup_n / g_fdn_n (nsel, ncol) of their sums, any of them NULL (counted as 0),
 *   grad_x(j, c) = sum over directions d, levels a and bins l of
 *                  (g_spec_d(l, a, c) + g_n_d(a, c) (freq(l) - freq(l+1))) w_d(l, a, j) dB/dT(avg_freq(l), x_c(j))
 * with x_c(1) = T_surface(c), x_c(1+m) = T(m, c): grad_T_surface (ncol) takes j = 1, grad_T (nz, ncol) the rest.  w_up /
 * w_dn (nw_ir, nsel, nz+1) are the weights of radtran_ir_spectra_batch for the levels the cotangents belong to; dB/dT is
 * the function radtran_ir_jacobian_spectral_rows uses.  No solve, no row of the Jacobian: one dB/dT per (bin, level,
 * column) (clima_amd/csrc/ir_rows_vjp.inc).  Contract: the result for (j, c) is bitwise repeatable and does not depend on
 * ncol or on the other columns (each lane sums its bins in ascending l, a inside that and up before down; the 64 lanes
 * are added in a fixed order; no atomics); all-zero cotangents give exactly 0.0; a direction without a cotangent is not
 * read.  A constructed handle is needed, and the whole spectrum; NO opacities (the frequency grid is all that is read).
 * Synchronous, host arrays, columns in chunks bounded like radtran_ir_spectra_batch's, results through the pinned block.
 * The handle's wrk_ir, wrk_sol, f_total, spectra, stored opacities and fields are left untouched; a pending deferred
 * integration is settled first.  Refused (err; nothing is written): a handle that is not constructed; ncol < 1; dim1_T /= nz
 * or dim2_T /= ncol ('"T" has the wrong input dimension.'); nsel < 1; a NULL T, T_surface, grad_T or grad_T_surface
 * ('"grad_T" is a required argument'); neither w_up nor w_dn; a cotangent whose direction has no weights ('"g_fdn_n" was
 * given without "w_dn"'); no cotangent at all; a bin shard or a communicator; a temperature that is not finite and
 * positive (radtran_ir_spectra_batch's text). */
void radtran_ir_spectra_batch_vjp(void *ptr, const int *ncol, const double *T_surface,
                                  const int *dim1_T, const int *dim2_T, const double *T, const int *nsel,
                                  const double *w_up, const double *w_dn,
                                  const double *g_ir_fup, const double *g_ir_fdn,
                                  const double *g_fup_n, const double *g_fdn_n,
                                  double *grad_T_surface, double *grad_T, char *err);
/* ... with every array in device memory of the handle's device (refused by name otherwise), enqueued on the handle's
 * stream behind `producer_stream` and final at the next radtran_synchronize, as radtran_ir_spectra_batch_device; bit for
 * bit the host form's gradient.  The temperatures are not checked: a T that is not positive or not finite gives whatever
 * adjoint_dbdt (clima_amd/csrc/ir_adjoint.inc) gives for it, without an error. */
void radtran_ir_spectra_batch_vjp_device(void *ptr, const int *ncol, const double *d_T_surface,
                                         const int *dim1_T, const int *dim2_T, const double *d_T, const int *nsel,
                                         const double *d_w_up, const double *d_w_dn,
                                         const double *d_g_ir_fup, const double *d_g_ir_fdn,
                                         const double *d_g_fup_n, const double *d_g_fdn_n,
                                         double *d_grad_T_surface, double *d_grad_T,
                                         const void *producer_stream, char *err);
/* The gradient of a loss on one column's IR spectra in the STORED optical properties (a vector-Jacobian product in tau,
 * w0, g at fixed temperatures).  The column is T_surface, T(nz) on the stored opacities; what is differentiated is
 * radiate(..., compute_solar=.false., compute_opacity=.false.) read at wrk_ir%fup_a / fdn_a (spec_level(a), l) and at
 * fup_n / fdn_n (spec_level(a)); levels 1..nz+1 ground-first, repeats allowed.  The cotangents g_ir_fup / g_ir_fdn (nw_ir,
 * nsel) and g_fup_n / g_fdn_n (nsel) follow radtran_ir_spectra_batch_vjp: a NULL counts as 0, g_*_n enters as g_n(a)
 * (freq(l) - freq(l+1)); the Planck values are planck_fcn(avg_freq(l), x(j)).  Outputs in radtran_opr_get's layout, so
 * that they line up with opr() element by element: grad_tau, grad_w0 (nz, ngauss, nw) and grad_g (nz, nw), TOA-first,
 * opacity-bin index, 0.0 in the bins outside the IR channel; any one or two may be NULL.  grad_tau(n, i, l) is the
 * derivative of the loss in the stored tau(n, i, l), the g-point's weight included, grad_w0 likewise; grad_g(n, l) sums
 * the g-points in g order.  tau, w0 and g are independent inputs, as two_stream_ir takes them (the max_w0 cap and the
 * tau <= tau_min -> w0 = 0 rule belong to the opacity step, not to this derivative); a layer with tau <= ir_tau_min is
 * differentiated inside its thin branch (exactly at the switch: unspecified); both surface forms and the per-bin
 * emissivity are covered; zenith weights are not read.  One adjoint and one forward two-stream solve per (bin, g-point)
 * whatever nsel is (clima_amd/csrc/ir_opr_sens.inc).  Contract: bitwise repeatable, no atomics, fixed summation orders;
 * all-zero cotangents give exactly 0.0 (a bin without a cotangent is not solved); a loss on fdn at level nz+1 alone gives
 * exactly 0; the handle's wrk_ir, wrk_sol, f_total, spectra, stored opacities and fields are left untouched; a pending
 * deferred integration and a two-in-flight join are settled first; every nz >= 1 and every g-point count of the single
 * call.  Refused (err; nothing is enqueued or written), naming the argument and its value: a handle that is not
 * constructed; dim_T /= nz; nsel < 1; a NULL spec_level; a level outside 1..nz+1; no cotangent at all; all three outputs
 * NULL; a NULL T or T_surface; a temperature that is not finite and positive; a bin shard or a communicator ("needs the
 * whole spectrum"); no opacities ("ir_spectra_opr_vjp needs opacities: ..."); a work buffer (6 x 2 nz + nz doubles per
 * (bin, g-point)) above the 4 GiB bound of radtran_ir_jacobian_spectral_rows. */
void radtran_ir_spectra_opr_vjp(void *ptr, const double *T_surface, const int *dim_T, const double *T,
                                const int *nsel, const int *spec_level,
                                const double *g_ir_fup, const double *g_ir_fdn,
                                const double *g_fup_n, const double *g_fdn_n,
                                double *grad_tau, double *grad_w0, double *grad_g, char *err);
/* ... with every array but spec_level in device memory of the handle's device (refused by name otherwise), enqueued on
 * the handle's stream behind `producer_stream` and final at the next radtran_synchronize, as
 * radtran_ir_spectra_batch_vjp_device; the temperatures are not checked; bit for bit the host form's gradient. */
void radtran_ir_spectra_opr_vjp_device(void *ptr, const double *d_T_surface, const int *dim_T, const double *d_T,
                                       const int *nsel, const int *spec_level,
                                       const double *d_g_ir_fup, const double *d_g_ir_fdn,
                                       const double *d_g_fup_n, const double *d_g_fdn_n,
                                       double *d_grad_tau, double *d_grad_w0, double *d_grad_g,
                                       const void *producer_stream, char *err);
/* The gradient of a loss on the SOLAR spectra in the STORED optical properties and in the surface albedo (a
 * vector-Jacobian product in tau, w0, g and surface_albedo).  What is differentiated is radiate(..., compute_solar=.true.,
 * compute_opacity=.false.) on the stored opacities under the handle's current zenith_u, zenith_weights, surface_albedo,
 * photon_scale_factor and diurnal_fac, read at wrk_sol%fup_a / fdn_a / amean (spec_level(a), l) and at wrk_sol%fup_n /
 * fdn_n (spec_level(a)); levels 1..nz+1 ground-first, any order, repeats allowed.  Everything is in the call's own units:
 * photons_sol, the photon scale factor and diurnal_fac, and amean's unit factors (clima_radtran_radiate.f90:164-179).  The
 * cotangents g_sol_fup / g_sol_fdn / g_sol_amean are (nw_sol, nsel), the bin fastest in rtchannel_freq_get order; g_fup_n /
 * g_fdn_n (nsel) enter as g_n(a) (freq(l) - freq(l+1)); a NULL counts as 0.  Outputs: grad_tau, grad_w0 (nz, ngauss, nw)
 * and grad_g (nz, nw) in radtran_opr_get's layout, TOA-first, opacity-bin index, 0.0 in the bins outside the solar channel,
 * the g-point's weight included, grad_g summed over the g-points in g order; grad_albedo (nw_sol), the derivative in
 * surface_albedo(l), a by-product of the same solve; any of the four may be NULL, not all.  tau, w0 and g are independent
 * inputs, as two_stream_solar takes them: its delta-Eddington scaling is part of the function and is differentiated, the
 * opacity step's max_w0 cap and tau_min rule are not.  One adjoint and one forward two-stream solve per (bin, g-point)
 * whatever nsel and the number of zenith angles are (clima_amd/csrc/sol_opr_sens.inc).  Contract: bitwise repeatable, no
 * atomics, fixed summation orders (the angles in their order inside a g-point, the g-points in g order); all-zero
 * cotangents give exactly 0.0 (a bin without a cotangent is not solved); a loss on fdn at level nz+1 alone gives exactly
 * 0 (direct(1) = u0 is a constant); the handle's wrk_ir, wrk_sol, f_total, spectra, stored opacities and fields are left
 * untouched; a pending deferred integration and a two-in-flight join are settled first; every nz >= 1 and every g-point
 * count of the single call, the handle's zenith angles.  In a (bin, g-point) without any scattering (w0 = 0 in every layer)
 * the cotangents of fdn give exactly 0 in the albedo.  Where lambda = 1 / u0 exactly in a layer the derivative is
 * unspecified (the forward call divides by lambda^2 - 1 / u0^2 there as well).  Refused (err; nothing is enqueued or
 * written), naming the argument and its value: a handle that is not constructed; nsel < 1; a NULL spec_level; a level
 * outside 1..nz+1; no cotangent at all; all four outputs NULL; a bin shard or a communicator ("needs the whole
 * spectrum"); a handle without solar bins; no opacities ("sol_spectra_opr_vjp needs opacities: ..."); a work buffer (9 x
 * 2 nz + nz + 1 doubles per (bin, g-point)) above the 4 GiB bound of radtran_ir_jacobian_spectral_rows. */
void radtran_sol_spectra_opr_vjp(void *ptr, const int *nsel, const int *spec_level,
                                 const double *g_sol_fup, const double *g_sol_fdn, const double *g_sol_amean,
                                 const double *g_fup_n, const double *g_fdn_n,
                                 double *grad_tau, double *grad_w0, double *grad_g, double *grad_albedo, char *err);
/* ... with every array but spec_level in device memory of the handle's device (refused by name otherwise), enqueued on
 * the handle's stream behind `producer_stream` and final at the next radtran_synchronize, as
 * radtran_ir_spectra_opr_vjp_device; bit for bit the host form's gradient. */
void radtran_sol_spectra_opr_vjp_device(void *ptr, const int *nsel, const int *spec_level,
                                        const double *d_g_sol_fup, const double *d_g_sol_fdn, const double *d_g_sol_amean,
                                        const double *d_g_fup_n, const double *d_g_fdn_n,
                                        double *d_grad_tau, double *d_grad_w0, double *d_grad_g, double *d_grad_albedo,
                                        const void *producer_stream, char *err);
/* clima/fortran/Radtran.f90:41-75 (same names and argument lists): the YAML text of
 * OpticalProperties_opacities2yaml (src/radtran/clima_radtran_types.f90:328-430).  _1 allocates
 * the string and returns its length, _2 copies it into out_c (out_len + 1 chars) and frees it.
 * The names it prints come from radtran_set_names / radtran_set_opacity_labels (what the loaders
 * know: species and particle names one per line in index order; k-method, water-continuum model,
 * one data-set name per added particle cross section). */
void radtran_opacities2yaml_wrapper_1(void *ptr, int *out_len, void **out_cp);
void radtran_opacities2yaml_wrapper_2(void *ptr, void **out_cp, const int *out_len, char *out_c);
void radtran_set_names(void *ptr, const char *species_names, const char *particle_names, char *err);
void radtran_set_opacity_labels(void *ptr, const char *k_method, const char *water_continuum_model,
                                const char *particle_data, char *err);
/* Launch form of a compute_opacity call: 1 (default) = opacity and two-stream work in one grid
 * (k_fused: two-stream blocks start as soon as the opacity blocks of their bin are done),
 * 0 = one launch per kernel.  Same results to rounding; CLIMA_HIP_FUSED=0 sets the default off. */
void radtran_fused_set(void *ptr, const int *enable);
void radtran_fused_get(void *ptr, int *enabled);
/* Construction from files: `Radtran(settings_f, star_f, num_zenith_angles, surface_albedo, nz, datadir, err)`
 * (src/radtran/clima_radtran.f90:98-126) for hosts that do not link the reference's loaders
 * (src/radtran/clima_radtran_types_create.f90): the settings YAML's optical-properties block, the stellar spectrum and a
 * `photochem_clima_data`-style directory (kdistributions/, CIA/, xsections/, water_continuum/, rayleigh/,
 * aerosol_xsections/) are read on the host (HDF5 C library opened at run time, CLIMA_HDF5_LIB names it) and handed to
 * radtran_create_begin ... radtran_create_end.  Strings are NUL-terminated; error texts are the reference's.
 * radtran_load_from_files is the same without the upload (radtran_create_end): the handle is left in the "begun" state. */
void radtran_create_from_files(void *ptr, const char *settings_file, const char *star_file, const int *num_zenith_angles,
                               const double *surface_albedo, const int *nz, const char *datadir, char *err);
void radtran_load_from_files(void *ptr, const char *settings_file, const char *star_file, const int *nz, const char *datadir, char *err);
/* extents of a handle (layers, gases, particles, opacity bins, g-points) and the names it holds (newline-separated, into
 * caller buffers of `cap` bytes each): what a host needs to size its arrays after radtran_create_from_files */
void radtran_dims_get(void *ptr, int *nz, int *nsp, int *np, int *nw, int *ngauss);
void radtran_names_get(void *ptr, const int *cap, char *species_names, char *particle_names);
/* All per-bin spectra of the last call in one go: the seven arrays of the two result holders (`ClimaRadtranWrk`,
 * src/radtran/clima_radtran.f90:11-25: fup_a, fdn_a (nz+1, nw), tau_band (nz, nw) per channel, amean for the solar
 * one), column-major as the reference-named getters fill them.  The caller's arrays are page-locked on first use
 * (hipHostRegister) and stay so until the handle is destroyed or radtran_spectra_release is called -- call that
 * before freeing them; they are filled by asynchronous copies on the handle's stream and one synchronise
 * (config 2: 6.7 MB in ~0.16 ms where the seven getters take ~0.53).  do_solar false: the IR arrays only. */
void radtran_spectra_get_all(void *ptr, const bool *do_solar, const int *nlev, const int *nw_ir, const int *nw_sol,
                             double *ir_fup_a, double *ir_fdn_a, double *ir_tau_band,
                             double *sol_fup_a, double *sol_fdn_a, double *sol_amean, double *sol_tau_band, char *err);
void radtran_spectra_release(void *ptr);
void radtran_batch_pin_results_set(void *ptr, const int *flag);
void radtran_batch_pin_results_get(void *ptr, int *flag);
/* With 8 g-points, calls with at most `items` (bin, source layer) items -- a bin-sharded rank, a short
 * column -- run the opacity work in the group-of-lanes kernel (8 lanes per item: a fifth of the
 * dependent chain of the lane-per-item kernel at 2.4x its total work) with one launch per kernel;
 * larger calls take the lane-per-item kernel inside the fused grid.  Default 34816
 * (CLIMA_HIP_COOP_ITEMS); 0 turns the group-of-lanes form off.  Same results to rounding (6e-14). */
void radtran_coop_items_set(void *ptr, const int *items);
void radtran_coop_items_get(void *ptr, int *items);
/* How many polls a two-stream block of the fused grid spends on its opacity tiles' flags before it gives up and the call
 * is repeated through separate launches (radtran_fused_fallbacks_get counts those).  Default 400000 (~0.2 s;
 * CLIMA_HIP_FUSED_SPINS); 0 makes every wait expire -- how the tests and bench.py's multi-GPU probe force the repeat. */
void radtran_fused_spins_set(void *ptr, const int *spins);
void radtran_fused_spins_get(void *ptr, int *spins);
/* radtran_radiate_ir_batch, response form.  With the opacities fixed two_stream_ir
 * (src/radtran/clima_radtran_twostream.f90:156-295) is linear in the Planck values of the levels, and the columns of
 * the RCE Jacobian (src/adiabat/clima_adiabat_solve.f90:798-812) are one base profile with one or a few temperatures
 * changed each: such a column is F(base) + unit responses x Planck differences, which costs one exp and two FMAs per
 * (level, deviation, bin, g-point) instead of a solve per (column, bin, g-point).  mode 1 (default): taken when at least
 * 48 columns differ from the profile the batch's columns share in at most 8 temperatures and a cost model of the two
 * forms favours it -- tall grids, few changes per column -- (the others, and the base profile itself, go through the
 * general kernel); not on handles whose ir_tau_min was lowered below 1e-7 (the source slope dB / tau of such thin layers
 * costs the response form digits first: 1e-8 against 5e-10 of a row's maximum in the fuzz sweep); 0: never; 2: whenever
 * any column qualifies (tests).  CLIMA_HIP_IR_GREEN sets the default.  Same results to rounding (1e-12 of the level
 * fluxes at the reference's ir_tau_min).  `batches` counts the batches that took it. */
void radtran_ir_green_set(void *ptr, const int *mode);
void radtran_ir_green_get(void *ptr, int *mode, int *batches);
/* A two-stream block of the fused grid waits (bounded) for the opacity blocks of its bin.  If that
 * wait ever expires the call is NOT failed: the library computes it again through the separate
 * launches before results are handed out.  This counts such re-issues on the handle (0 in normal
 * operation; CLIMA_HIP_FUSED_SPINS=0 forces them, for tests). */
void radtran_fused_fallbacks_get(void *ptr, int *count);
/* radtran_radiate_resident returns without anyone reading a result, so on a handle where this is on (the default) it
 * keeps the call's frequency integration back: the next compute_opacity call on the handle launches it in ONE grid with
 * its own prep pass (k_prep_integrate; the two are independent and each far too small to fill the device), and anything
 * else that enqueues work or reads results -- radtran_synchronize, every getter, an IR-only call, the batches, the
 * Jacobians, a call whose prep pass clears the spectra (columns of at most 64 layers, the whole-wave forms) -- launches
 * it first, alone, exactly as the call itself would have.  Results are bitwise the same either way.  Never on a
 * bin-sharded handle or one with a communicator, with radtran_profile_set(1), while the handle's stream is being
 * captured, or once radtran_flux_device_ptr has been called (its caller reads the rows in stream order, unannounced).
 * Where the handle keeps two calls in flight (radtran_calls_in_flight_set below) a call's integration stays in its call
 * slot and goes out with the prep pass of the next call INTO THAT SLOT, two calls on; whatever joins launches both
 * slots' pending integrations alone, the older call's first.
 * merged_integrations_get: pending integrations that went out with a later prep pass / alone, on either slot.  N >= 2
 * pipelined calls of a shape that merges and one radtran_synchronize: (N - 2, 2) where two are in flight -- the older
 * of the last two is launched too, not dropped -- against (N - 1, 1) one at a time. */
void radtran_defer_integration_set(void *ptr, const int *enable);
void radtran_defer_integration_get(void *ptr, int *enabled);
void radtran_merged_integrations_get(void *ptr, int *merged, int *standalone);
/* test hook: the rule above as a function of its inputs (no handle, no device) */
void clima_test_defer_allowed(const int *switch_on, const int *shard_world, const int *has_comm, const int *profile,
                              const int *capturing, const int *flux_ptr_taken, int *allowed);
/* Two resident calls in flight.  Nothing orders the bulk of a pipelined radtran_radiate_resident call behind the one
 * before it but the work buffers and the stream they share, so the handle keeps a second set of everything a call
 * writes (a second call slot, allocated the first time it is used) and a second stream: a call that computes opacities
 * and solar fluxes runs BESIDE the previous such call, in the slot that is not current, when it may keep its results
 * back (the conditions of radtran_defer_integration_set above), when nobody has waited for or joined the previous call
 * since it was enqueued, when its dominant kernel carries no event pair (radtran_profile_set(2): a timed launch runs
 * alone), and when the mode allows it.  Such a call, where its own prep pass cleared nothing, keeps its frequency
 * integration back in its slot, and the call that next takes the slot -- two calls on, on the same stream -- launches
 * it in one grid with its own prep pass (k_prep_integrate): two launches per call on each stream,
 * `[integrate(i-2) | prep(i)] -> fused(i)`.  Where the prep pass clears the spectra (never merged) the call integrates
 * at once, and a kept-back integration that meets such a pass goes out first, alone, on that stream.  An integration
 * pending from a call that was not pipelined keeps the next call from running beside; a slot's own pipelined one does
 * not.  Everything else -- every other call, every getter, radtran_synchronize, the batches, the Jacobians, a setter
 * that rewrites device memory -- first joins: the handle's stream waits for an event behind the other stream's work (no
 * host wait), the other slot's pending integration goes out on it, alone, and the handle's buffers are those of the
 * slot the latest call took.  radtran_upload_column between pipelined calls goes to the slot its next call will take.
 * Results are bitwise those of mode 1.
 *   mode 0 (default): automatic -- when the call's grid does not fit the device in one residency round of two waves per
 *          SIMD (waves of the fused grid, or of the separate form's opacity launch, > 8 x compute units); smaller calls
 *          are launch-bound and keep the chain described above
 *   mode 1: one call at a time   mode 2: two whenever eligible, whatever the size
 * overlapped_calls_get: calls enqueued on a slot while the other slot's call had not been joined.
 * radtran_stream_get stays the handle's first stream, and asking for it joins: ask AFTER the calls whose work is to be
 * ordered against.  A stream obtained before them does not cover a call that ran on the second stream since (its work
 * is ordered behind that call only by the next join: any entry point but a pipelined resident call or its upload). */
void radtran_calls_in_flight_set(void *ptr, const int *mode);
void radtran_calls_in_flight_get(void *ptr, int *mode);
void radtran_overlapped_calls_get(void *ptr, int *count);
/* test hook: the rule above as a function of its inputs (no handle, no device).  rule[CLIMA_TWO_IN_FLIGHT_RULE_N]:
 *    0 mode   1..6 clima_test_defer_allowed's inputs in its order   7 the previous call is unjoined
 *    8 the call's dominant kernel carries an event pair   9 compute units of the device
 *   10 the handle's fields are stale on the device   11 an integration is pending
 * (whether the integration fits the one-launch kernel is taken from in[20], the wider channel's bins)
 * in[CLIMA_PLAN_IN_N]: the call, as clima_test_plan_radiate below takes it.  out[0]: the call takes the other slot;
 * out[1]: the waves of its grid. */
#define CLIMA_TWO_IN_FLIGHT_RULE_N 12
void clima_test_two_in_flight(const int *rule, const int *in, int *out);
/* test hook: the launch plan of one radiate call as the library's own planner (plan_radiate) decides it; no handle, no
 * device.  in[CLIMA_PLAN_IN_N], the planner's inputs in this order:
 *    0 nz   1 ng   2 nzen   3 n_ir   4 n_sol   5 op_n   6 nsrc   7 ncol   8 batch   9 ir_batch   10 rebin_mode
 *   11 cust_on   12 compute_opacity   13 all_pairs   14 fused   15 allow_fused   16 ts_block_mode   17 no_half
 *   18 coop_items   19 force_slots   20 nbins (of the wider channel: what the frequency integration is sized by)
 * out[CLIMA_PLAN_OUT_N]:
 *    0 opacity (0 stored opacities, 1 lane per item, 2 group of lanes, 3 unsupported)   1 coop_ng
 *    2..6 the fused grid, 7..11 the stand-alone wave forms, 12..16 the workgroup-per-bin form, each as
 *         form (0 none, 1 whole wave, 2 half wave, 3 exact pairs, 4 workgroup per bin), slots, groups, per_launch, zero_launch
 *   17 prep_clears   18 caller_clears   19 write_w0
 *   20 the frequency integration of nbins bins fits the one-launch kernel (a column batch takes one launch per chunk
 *      only where this holds and the plan of a chunk is fused) */
#define CLIMA_PLAN_IN_N 21
#define CLIMA_PLAN_OUT_N 21
void clima_test_plan_radiate(const int *in, int *out);
/* test hook: the account of what a handle holds between calls (Holds, clima_amd/csrc/radtran_dev.h) replayed on a bare
 * one; no handle, no device.  events: the question's shard_world, has_comm, op_lo, op_n (the opacity bins
 * [op_lo, op_lo + op_n) a call would work on), then n transitions of CLIMA_HOLDS_EVENT_N ints each, a code and its
 * arguments in order (the rest 0):
 *   0 uploaded(has_particles)   1 opacities_written(own_block, w0_stored, from_resident, lo, n)   2 w0_formed
 *   3 rows_enqueued(in_pinned)   4 rows_changed   5 rows_fetched   6 batch_left(one_launch, np)   7 batch_repeated
 *   8 results_dropped            (another code: out[0] = -1)
 * out[CLIMA_HOLDS_OUT_N]:
 *    0 column loaded   1 given with particles   2 uploads so far
 *    3 optical properties valid   4 w0 stored   5 the upload they were computed from   6, 7 their bins: first, count
 *    8 level rows current on the host   9 the last integration stored them into the pinned block itself
 *   10, 11, 12 a call that needs a column / opacities / the whole spectrum is refused (1) or not (0)
 *   13 the optical properties are the resident column's (what a repair after an expired hand-off wait asks) */
#define CLIMA_HOLDS_EVENT_N 6
#define CLIMA_HOLDS_OUT_N 14
void clima_test_handle_holds(const int *n, const int *events, int *out);
/* test hook: the rebin form (0 window, 1 streaming, 2 streaming multi-edge) a handle takes for these ng g-point weights;
 * stream != 0: as under CLIMA_HIP_REBIN=stream */
void clima_test_rebin_mode_for(const int *ng, const double *weights, const int *stream, int *mode);
/* HIP stream the handle launches on (for callers that order other work against it).  Always the same stream.  The
 * call joins the handle's second stream into it (radtran_calls_in_flight_set): ask after the calls to be ordered
 * against -- a value cached earlier does not cover pipelined calls that ran on the second stream since. */
void radtran_stream_get(void *ptr, void **stream);
/* per-kernel device time (HIP events on the handle's stream).  enable = 1 records events
 * around every kernel, enable = 2 around the dominant kernel (id 1, opacity) only, 0 turns
 * them off; kernel_time_get returns accumulated ms and launch count for kernel id
 * (0 prep, 1 opacity, 2 twostream, 3 integrate; of radtran_ir_spectra_batch and its device form: 4 the weights' adjoint
 * pass, 5 the apply and integrate kernels of all its chunks; 6 the gradient kernel of all chunks of
 * radtran_ir_spectra_batch_vjp and its device form) and resets nothing. */
void radtran_profile_set(void *ptr, const int *enable);
/* record the events on every stride-th call only (default 1): an event pair drains the queue for a
 * few microseconds, which a throughput measurement should not pay on every call */
void radtran_profile_stride_set(void *ptr, const int *stride);
void radtran_kernel_time_get(void *ptr, const int *kernel_id, double *ms_total, int *launches,
                             char *err);
void radtran_profile_reset(void *ptr);
/* algorithmic-byte accounting of SURVEY.md 8(d) for the last uploaded column */
void radtran_algorithmic_bytes(void *ptr, double *bytes_tables_distinct, double *bytes_in,
                               double *bytes_out, double *bytes_tables_full, char *err);

/* N_PT (distinct (P,T) k-table nodes the last uploaded column touches, mean over the
 * k-tables, and the table's nP*nT) and N_T (the same for the 1-D temperature tables) */
void radtran_algorithmic_nodes(void *ptr, double *n_pt, double *n_pt_full, double *n_t, double *n_t_full, char *err);

/* bench hooks: n calls timed one by one with the host's steady clock INSIDE the library (us[n]) -- what a
 * Fortran / C caller sees, without a foreign-function layer's own cost.  clima_bench_toa_fluxes: the synchronous
 * drop-in call radtran_toa_fluxes_wrapper (arguments as there; compute_solar = compute_opacity = 1);
 * clima_bench_resident_sync: radtran_radiate_resident + radtran_synchronize per call (column already in HBM). */
void clima_bench_toa_fluxes(void *ptr, const int *n, const double *T_surface, const int *dim_T, const double *T,
                            const int *dim_P, const double *P, const int *dim1_d, const int *dim2_d,
                            const double *densities, const int *dim_dz, const double *dz, const int *has_particles,
                            const int *dim1_p, const int *dim2_p, const double *pdensities, const int *dim1_r,
                            const int *dim2_r, const double *radii, double *us, double *ISR, double *OLR, char *err);
void clima_bench_resident_sync(void *ptr, const int *n, double *us, char *err);
/* Timing only: one resident call's launches captured into a hipGraph and replayed (k launches per synchronise), us[n]
 * per pass; the replayed results are not valid (the captured call id makes the fused grid's waits trivial). */
void clima_bench_resident_graph(void *ptr, const int *n, const int *k, double *us, char *err);

/* test hook: y[i] = the kernels' device exp(x[i]) (used where the reference calls exp) */
void clima_test_device_exp(const int *n, const double *x, double *y, char *err);
/* FNV-1a (64 bit) over the handle's host-side tables (metadata as int32, values as float64 bytes, in the order they were
 * handed over), one digest per group -- digest[0..7]: extents + grid, k-tables, CIA, Rayleigh, absorption / photolysis,
 * continuum, particles, channels + stellar photons: how the from-files loader is held to the Python one without a device */
void clima_test_host_tables_digest(void *ptr, unsigned long long *digest);
void clima_test_device_exp_table(const int *n, const int *base10, const double *x, double *y, char *err);
/* test hook: the device reciprocal with 0, 1 and 2 Newton steps, and the device sqrt of |x|
 * (y: 4 arrays of n) */
void clima_test_device_rcp(const int *n, const double *x, double *y, char *err);
/* test hook: the DPP wave scans of the kernels on nwaves*64 values (out: 4 arrays of that length:
 * affine inclusive scan, the same through build+apply, shift up by one lane, lane reversal) */
void clima_test_wave_scan(const int *nwaves, const double *a, const double *b, double *out, char *err);

/* test hook: one column through the PRODUCTION two-stream kernels with tau, w0, g (nz, TOA-first) and
 * the Planck values of the levels (nz+1) given directly -- the arguments of the reference's
 * two_stream_ir / two_stream_solar (src/radtran/clima_radtran_twostream.f90:10-295).  ir_par =
 * {emissivity, has_hard_surface, ir_tau_min}, sol_par = {u0, Rsfc}; ng g-points of weights wbin (sum
 * 1) carry the same column.  form 0: k_twostream_w<slots>, 1: k_twostream, 2: two-stream part of
 * k_fused in its whole-wave form (slots 2..8, ng 8), 4: the same in the half-wave form (two g-point columns
 * per wave, slots = ceil(nz/32) = 3..7), 5: the same in the paired form (a column of pairwise identical
 * layers -- AdiabatClimate's doubled radiative grid -- even nz, slots 2, 4, 6, 8),
 * 3: k_twostream_ir_batch<slots, NW> (IR only; slots 1..4 in blocks of 8 g-point waves, 5..8 in blocks of 4),
 * 6: the same in blocks of 4 waves at every slot count.  Outputs (nz+1) TOA-first. */
void clima_test_two_stream(const int *nz, const int *ng, const int *form, const int *slots, const double *tau,
                           const double *w0, const double *g, const double *bplanck, const double *ir_par,
                           const double *sol_par, const double *wbin, double *ir_fup, double *ir_fdn,
                           double *sol_fup, double *sol_fdn, double *sol_amean, char *err);
/* The same for k_twostream_sol_batch (solar_batch.inc): one column of tau, w0, g (nz, TOA-first) carried by ng g-points of
 * weights wbin as one solar bin; ncol cases of nzen angles (zen_u, zen_w (nzen, ncol)) and surface reflectance rsfc (ncol)
 * go through the production kernel with photon factor 1.  force_nw = 4 selects the 4-wave form at every slot count.
 * Outputs (nz+1, ncol), TOA-first.  ..._cases_per_block: the launcher's rule for the cases a block takes. */
void clima_test_solar_batch(const int *nz, const int *ng, const int *force_nw, const double *tau, const double *w0,
                            const double *g, const double *wbin, const int *ncol, const int *nzen, const double *zen_u,
                            const double *zen_w, const double *rsfc, double *fup, double *fdn, double *amean, char *err);
void clima_test_solar_batch_cases_per_block(const int *ncol, int *cases);
/* The same for the response form of radtran_radiate_ir_batch (ir_green.inc): the column of clima_test_two_stream and
 * `ndev` changes of the Planck value at levels dev_k (TOA-first, nz = the surface) -> per change the change of the level
 * fluxes, resp_up / resp_dn (nz+1, ndev) TOA-first, summed over the g-points with the weights wbin -- produced by the
 * production kernels (k_green_factor, k_green_unit, k_green_local, k_green_accum_far, k_green_accum_mixed).
 * tests/test_gpu_golden.py holds F(base) + the changes to what the reference's two_stream_ir
 * (src/radtran/clima_radtran_twostream.f90:156-295) returns for the changed Planck profile.  nz >= 4. */
void clima_test_ir_response(const int *nz, const int *ng, const double *tau, const double *w0, const double *g,
                            const double *ir_par, const double *wbin, const int *ndev, const int *dev_k,
                            const double *dev_db, double *resp_up, double *resp_dn, char *err);
/* The same for the adjoint rows of radtran_ir_jacobian_spectral_rows (ir_adjoint.inc): the column of
 * clima_test_two_stream as one IR bin and nrow levels (0..nz, TOA-first) -> dfup(a, k) = d fup(level(a)) / d bplanck(k)
 * and dfdn likewise, (nrow, nz+1) row after row, k TOA-first, summed over the g-points with the weights wbin -- produced
 * by the production kernels (k_adjoint_rows, k_adjoint_sum) with unit amplitudes.  nz >= 1. */
void clima_test_ir_adjoint(const int *nz, const int *ng, const double *tau, const double *w0, const double *g,
                           const double *ir_par, const double *wbin, const int *nrow, const int *level,
                           double *dfup, double *dfdn, char *err);
/* The same for the optical-property gradient of radtran_ir_spectra_opr_vjp (ir_opr_sens.inc): that column with the Planck
 * values bplanck (nz+1, TOA-first) and nrow levels (0..nz, TOA-first) -> up_tau(a, n) = d fup(level(a)) / d tau(n), up_w0,
 * up_g and dn_* likewise, (nrow, nz) row after row, n TOA-first, summed over the g-points with the weights wbin --
 * produced by ONE launch of the production kernels (k_opr_adjoint, k_opr_sum_g), each (row, direction) a bin of its own
 * with a unit cotangent.  nz >= 1. */
void clima_test_ir_opr_sens(const int *nz, const int *ng, const double *tau, const double *w0, const double *g,
                            const double *bplanck, const double *ir_par, const double *wbin, const int *nrow,
                            const int *level, double *up_tau, double *up_w0, double *up_g,
                            double *dn_tau, double *dn_w0, double *dn_g, char *err);

/* The same for the solar optical-property gradient of radtran_sol_spectra_opr_vjp (sol_opr_sens.inc): the column of
 * clima_test_solar_batch as one solar bin with nzen zenith angles (zen_u, zen_w), the surface reflectance rsfc (1) and
 * nrow levels (0..nz, TOA-first) -> up_tau(a, n) = d fup(level(a)) / d tau(n), up_w0, up_g ((nrow, nz) row after row, n
 * TOA-first), up_rsfc(a) = d fup(level(a)) / d rsfc, and dn_* (fdn), am_* (amean) likewise, summed over the zenith angles
 * with their weights and over the g-points with the weights wbin -- produced by ONE launch of the production kernels
 * (k_sol_opr_adjoint, k_sol_opr_sum_g) with unit stellar flux and unit factors, each (row, quantity) a bin of its own with
 * a unit cotangent.  nz >= 1. */
void clima_test_sol_opr_sens(const int *nz, const int *ng, const double *tau, const double *w0, const double *g,
                             const double *wbin, const int *nzen, const double *zen_u, const double *zen_w, const double *rsfc,
                             const int *nrow, const int *level,
                             double *up_tau, double *up_w0, double *up_g, double *up_rsfc,
                             double *dn_tau, double *dn_w0, double *dn_g, double *dn_rsfc,
                             double *am_tau, double *am_w0, double *am_g, double *am_rsfc, char *err);

/* test hook: the sums over the bins, fup_n(i) = sum_l fup_a(i,l) * (freq(l) - freq(l+1)) (clima_radtran_radiate.f90:184-192),
 * by the PRODUCTION integration kernels on arrays given directly, without a handle.  ir_dims / sol_dims = {bins of the
 * channel, first owned bin (0-based), owned bins}; ir_freq / sol_freq (bins + 1); the per-bin arrays (nz+1, bins, ncol)
 * column-major, ground-first as the kernels hold them; on the device the columns lie spec_stride (>= bins * (nz+1))
 * doubles apart.
 *   form 0: the launcher of every radiate call (k_integrate_one, or k_integrate_partial + k_integrate_final above 5440
 *           owned bins in a channel: one column); 1: that two-launch pair at any bin count (one column).
 *           flux_n (nz+1, 4, ncol) is read and written (flux_stride >= 4 * (nz+1) apart on the device): the rows ir up, ir
 *           down, solar up, solar down; with do_solar = 0 the solar rows stay as given, or become flux_part's where
 *           flux_part (nz+1, 4; optional, one column; read and written) is given (do_solar = 0: one column).  col0 and out
 *           are not used.
 *   form 2: the batch pair (k_integrate_partial_b, k_integrate_final_b) on ir_fup_a / ir_fdn_a; the solar arguments and
 *           flux_stride are not used, flux_n (nz+1, 4) is read for f_total, out (nz+1, col0 + ncol, 3) = fup_n, fdn_n,
 *           f_total is read and written: the columns from col0 on are the results. */
void clima_test_integrate(const int *form, const int *nz, const int *ncol, const int *spec_stride, const int *flux_stride,
                          const int *ir_dims, const double *ir_freq, const int *sol_dims, const double *sol_freq,
                          const double *ir_fup_a, const double *ir_fdn_a, const double *sol_fup_a, const double *sol_fdn_a,
                          const int *do_solar, double *flux_n, double *flux_part, const int *col0, double *out, char *err);

/* The far accumulation of the response form has two kernels: 0 (default) the matrix-core one (v_mfma_f64_16x16x4_f64),
 * 1 the vector one it replaced.  Process-wide; tests hold the two against each other. */
void clima_test_green_far_form_set(const int *vector_form);

/* OpticalPropertiesResult (clima_radtran_types.f90:242-247), for parity checks:
 * tau,w0 (nz,ngauss,nw) and g,tau_band (nz,nw), column-major, TOA-first.  Refused ("opr_get needs opacities: ...")
 * where the handle's own block holds none: a fresh handle, after a batch that ran one launch per chunk. */
void radtran_opr_get(void *ptr, double *tau, double *w0, double *g, double *tau_band, char *err);

/* ------------------------------------------------------------------------------------
 * Getters / setters with the reference's names and signatures
 * (clima/fortran/Radtran.f90:3-299).
 * ---------------------------------------------------------------------------------- */
void radtran_set_bolometric_flux_wrapper(void *ptr, const double *flux);             /* :3  */
void radtran_bolometric_flux_wrapper(void *ptr, double *flux);                       /* :12 */
void radtran_skin_temperature_wrapper(void *ptr, const double *bond_albedo, double *T_skin); /* :21 */
void radtran_equilibrium_temperature_wrapper(void *ptr, const double *bond_albedo, double *T_eq); /* :31 */
void radtran_zenith_u_get_size(void *ptr, int *dim1);                                /* :124 */
void radtran_zenith_u_get(void *ptr, const int *dim1, double *arr);                  /* :133 */
void radtran_zenith_u_set(void *ptr, const int *dim1, const double *arr);            /* :143 */
void radtran_zenith_weights_get(void *ptr, const int *dim1, double *arr);            /* field :53 */
void radtran_zenith_weights_set(void *ptr, const int *dim1, const double *arr);
void radtran_surface_albedo_get_size(void *ptr, int *dim1);                          /* :153 */
void radtran_surface_albedo_get(void *ptr, const int *dim1, double *arr);            /* :162 */
void radtran_surface_albedo_set(void *ptr, const int *dim1, const double *arr);      /* :172 */
void radtran_surface_emissivity_get_size(void *ptr, int *dim1);                      /* :182 */
void radtran_surface_emissivity_get(void *ptr, const int *dim1, double *arr);        /* :191 */
void radtran_surface_emissivity_set(void *ptr, const int *dim1, const double *arr);  /* :201 */
void radtran_has_hard_surface_get(void *ptr, bool *val);                             /* :211, logical(c_bool) */
void radtran_has_hard_surface_set(void *ptr, const bool *val);                       /* :220, logical(c_bool) */
void radtran_photon_scale_factor_get(void *ptr, double *val);                        /* :229 */
void radtran_photon_scale_factor_set(void *ptr, const double *val);                  /* :238 */
void radtran_ir_tau_min_get(void *ptr, double *val);                                 /* :247 */
void radtran_ir_tau_min_set(void *ptr, const double *val);                           /* :256 */
void radtran_diurnal_fac_get(void *ptr, double *val);                                /* field :51 */
void radtran_diurnal_fac_set(void *ptr, const double *val);
void radtran_ir_get(void *ptr, void **ptr1);                                         /* :265 */
void radtran_sol_get(void *ptr, void **ptr1);                                        /* :274 */
void radtran_wrk_ir_get(void *ptr, void **ptr1);                                     /* :283 */
void radtran_wrk_sol_get(void *ptr, void **ptr1);                                    /* :292 */
void radtran_f_total_get_size(void *ptr, int *dim1);                                 /* field :72 */
void radtran_f_total_get(void *ptr, const int *dim1, double *arr);
void radtran_photons_sol_get_size(void *ptr, int *dim1);                             /* field :65 */
void radtran_photons_sol_get(void *ptr, const int *dim1, double *arr);

/* ClimaRadtranWrk (clima/fortran/ClimaRadtranWrk.f90:7-123); ptr from radtran_wrk_*_get.
 * Getters copy device results out on first use after a radiate (lazy D2H). */
void climaradtranwrk_fup_a_get_size(void *ptr, int *dim1, int *dim2);
void climaradtranwrk_fup_a_get(void *ptr, const int *dim1, const int *dim2, double *arr);
void climaradtranwrk_fdn_a_get_size(void *ptr, int *dim1, int *dim2);
void climaradtranwrk_fdn_a_get(void *ptr, const int *dim1, const int *dim2, double *arr);
void climaradtranwrk_fup_n_get_size(void *ptr, int *dim1);
void climaradtranwrk_fup_n_get(void *ptr, const int *dim1, double *arr);
void climaradtranwrk_fdn_n_get_size(void *ptr, int *dim1);
void climaradtranwrk_fdn_n_get(void *ptr, const int *dim1, double *arr);
void climaradtranwrk_amean_get_size(void *ptr, int *dim1, int *dim2);
void climaradtranwrk_amean_get(void *ptr, const int *dim1, const int *dim2, double *arr);
void climaradtranwrk_tau_band_get_size(void *ptr, int *dim1, int *dim2);
void climaradtranwrk_tau_band_get(void *ptr, const int *dim1, const int *dim2, double *arr);

/* RTChannel (clima/fortran/RTChannel.f90:3-38); ptr from radtran_ir_get / radtran_sol_get */
void rtchannel_wavl_get_size(void *ptr, int *dim1);
void rtchannel_wavl_get(void *ptr, const int *dim1, double *arr);
void rtchannel_freq_get_size(void *ptr, int *dim1);
void rtchannel_freq_get(void *ptr, const int *dim1, double *arr);

#ifdef __cplusplus
}
#endif
#endif
