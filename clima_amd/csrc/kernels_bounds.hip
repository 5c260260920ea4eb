// kernels_bounds.hip -- the kernels of the column batches with per-column bounds (radtran_toa_fluxes_batch_bounds): the BND
// instances of k_fused, k_twostream_w, k_twostream_h and k_twostream, their launchers launch_fused_bounds,
// launch_twostream_w_bounds and launch_twostream_bounds, and k_pack_bounds.  They are kernels.hip's templates, compiled
// here into a code object of their own: kernels.hip's own code object holds what it held before there were bounds, and a
// process that runs no bounds batch loads and looks up what it did (kernels.hip says what each compilation holds).
#define CLIMA_BOUNDS_TU 1
#include "kernels.hip"
