// Crowded-field photometry of cubes (mpsfr_fit_cube_psf, include/mpsfr.h): the solve of
// frame_fit_impl.h for a batch of layers side by side -- its kernels in their LAYERS form, the layer one more grid
// dimension, one done word per layer, the tile lists built and sorted once from the geometry.  Layer by layer the bits
// are those of mpsfr_fit_frame_psf: the code that fixes them is the same.
#include "frame_fit_impl.h"

namespace mpsfr {

size_t cube_fit_workspace_bytes(int ny, int nx, int nstar, int layers) {
    return workspace_bytes<FrameFitWork>(ny, nx, nstar, layers);
}

void launch_fit_cube(hipStream_t s, int ny, int nx, int layers, const double* d_cube, const double* d_var,
                     StarList stars, const double* d_scale0, double radius, bool background, int max_iter, double tol,
                     double* d_star_out, double* d_head_out, double* d_resid_out, void* d_ws) {
    fit_layers<true>(s, ny, nx, layers, d_cube, d_var, stars, d_scale0, radius, background, max_iter, tol, d_star_out,
                     d_head_out, d_resid_out, d_ws);
}

}  // namespace mpsfr
