// The f64 instantiations of k_fit_group (fit_group_impl.h): fp64 throughout, the stamp, its weights and the model
// stamp as doubles in LDS (60 KB).
#include "fit_group_impl.h"
#include "kernels.h"

namespace mpsfr {

void launch_fit_group_f64(hipStream_t s, int nstamp, int nsrc, const double* d_stamps, const double* d_var, int npsf,
                          const double* d_psf, const int32_t* d_index, const double* d_shift, int flags,
                          double* d_fit) {
    switch (nsrc) {                // (the C entry point has refused any other size)
    case 2:
        launch_fit_group_mode<double, 2>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    case 3:
        launch_fit_group_mode<double, 3>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    case 4:
        launch_fit_group_mode<double, 4>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    default:
        break;
    }
}

}  // namespace mpsfr
