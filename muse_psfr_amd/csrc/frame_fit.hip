// Crowded-field PSF photometry (mpsfr_fit_frame_psf, include/mpsfr.h): the fluxes of all stars of
// a frame, and one constant, as one weighted linear least-squares problem, solved by Jacobi-preconditioned conjugate
// gradients on the normal equations without ever forming them.  A x is the renderer's tile walk (render.hip) over lists
// built once per solve; what is new here:
//   k_ff_star<false>  one workgroup per star: judges it (FrameStar's rule and footprint, which are the renderer's; the
//                     valid pixels of its own disc, sum w P~^2 over them) and takes sum P of its model
//   k_ff_domain       one workgroup per frame tile: W = w [pixel in Omega], Omega the valid pixels in the disc of an
//                     accepted star, from the tile's star list
//   k_ff_star<true>   the projection, one workgroup per accepted star: g_k = sum W P~_k (V + c) over its footprint and,
//                     in the first pass, N_kk = sum W P~_k^2 -- the model stamp with the rows and columns its taps
//                     reach staged once in LDS, every thread a fixed set of footprint pixels, a fixed tree
//   k_ff_reduce       sum W (V + c), sum W, sum W (V + c)^2 and |Omega| over chunks of the frame, one partial per chunk
//   k_ff_step<phase>  one workgroup: the conjugate-gradient step over the unknowns, the stop test and the done word; the
//                     first residual; the rows of the result
// The kernels and the driver are in frame_fit_impl.h, which has them for the layers of a cube too (cube_fit.hip).
// Every sum has a fixed order (no floating-point atomics), all arithmetic is fp64, and nothing waits for the host: the
// scalars live in the work buffer, and once the done word is set the queued kernels of the later iterations return.
#include "frame_fit_impl.h"

namespace mpsfr {

size_t frame_fit_workspace_bytes(int ny, int nx, int nstar) { return workspace_bytes<FrameFitWork>(ny, nx, nstar); }

void launch_fit_frame(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, StarList stars,
                      const double* d_scale0, double radius, bool background, int max_iter, double tol,
                      double* d_star_out, double* d_head_out, double* d_resid_out, void* d_ws) {
    fit_layers<false>(s, ny, nx, 1, d_image, d_var, stars, d_scale0, radius, background, max_iter, tol, d_star_out,
                      d_head_out, d_resid_out, d_ws);
}

}  // namespace mpsfr
