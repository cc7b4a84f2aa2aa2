// The simultaneous PSF-model fit of blended stars (k_fit_group, fit_group_impl.h): the entry
// point of the launchers and the instantiations of the mixed mode (float iterations + fp64 polish) for 2 and 3
// sources.  Those for 4 sources are in fit_group_k4.hip and the f64 ones in fit_group_f64.hip, so that the three
// shares of the 36 variants compile side by side.
#include "fit_group_impl.h"
#include "kernels.h"

namespace mpsfr {

void launch_fit_group_k4(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                         const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit);
void launch_fit_group_f64(hipStream_t s, int nstamp, int nsrc, const double* d_stamps, const double* d_var, int npsf,
                          const double* d_psf, const int32_t* d_index, const double* d_shift, int flags,
                          double* d_fit);

void launch_fit_group(hipStream_t s, int nstamp, int nsrc, const double* d_stamps, const double* d_var, int npsf,
                      const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit,
                      bool f64) {
    if (nstamp <= 0) return;
    if (f64) {
        launch_fit_group_f64(s, nstamp, nsrc, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        return;
    }
    switch (nsrc) {                // (the C entry point has refused any other size)
    case 2:
        launch_fit_group_mode<float, 2>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    case 3:
        launch_fit_group_mode<float, 3>(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    case 4:
        launch_fit_group_k4(s, nstamp, d_stamps, d_var, npsf, d_psf, d_index, d_shift, flags, d_fit);
        break;
    default:
        break;
    }
}

}  // namespace mpsfr
