// The mixed-mode instantiations of k_fit_group (fit_group_impl.h) for 4 sources: up to 13 variables.
#include "fit_group_impl.h"
#include "kernels.h"

namespace mpsfr {

void launch_fit_group_k4(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                         const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit) {
    launch_fit_group_mode<float, 4>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
}

}  // namespace mpsfr
