/* libmpsfr -- C ABI of the MI355X-native PSF-reconstruction hot path of muse-psfr.
 *
 * The reference (musevlt/muse-psfr) has no FFI: its boundary for this path is two Python
 * functions.  This header is what a ctypes binding of those functions binds to; every entry
 * point cites the reference interface it replaces (file:line in /root/reference/muse_psfr/).
 *
 * Conventions: plain pointers and sizes only; all arrays C-contiguous; every function returns 0
 * on success or a negative error code (MPSFR_E_*), with a thread-local message available from
 * mpsfr_last_error(); nothing is allocated across the ABI; no exceptions cross it.  A context
 * owns one GPU (one process per GPU, one context per process is the intended use), its HIP
 * streams and all device workspaces; it is not re-entrant.
 *
 * Asynchronous calls (on_device = 1) are pipelined inside the context: consecutive calls run on
 * alternating internal streams ("lanes") with their own workspaces, so the transforms of one
 * call overlap the convolutions and fits of the one before.  What a caller may rely on:
 *   - mpsfr_stream() is ordered after every call made so far (wait on it, or mpsfr_sync, before
 *     reading results);
 *   - two calls that write the same output buffer run in call order;
 *   - calls with distinct output buffers may run concurrently and finish in any order;
 *   - to make the NEXT call wait for the caller's own GPU work, register an event with
 *     mpsfr_wait_event (work queued on mpsfr_stream() does not hold back later calls).
 * Option "pipeline_calls" = 0 restores strictly serial calls.
 */
#ifndef MPSFR_H
#define MPSFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpsfr_ctx mpsfr_ctx;

#define MPSFR_OK            0
#define MPSFR_E_INVALID    -1   /* bad argument (message says which) */
#define MPSFR_E_HIP        -2   /* a HIP runtime call failed */
#define MPSFR_E_GRID       -3   /* wavelength too short for the grid: npixc(lambda) > dim.  The
                                   reference raises ValueError from interpn here
                                   (psfrec.py:663-664, 672-683) */
#define MPSFR_E_NOMEM      -4

/* precision modes */
#define MPSFR_PREC_MIXED    0   /* fp64 PSD -> structure function, fp32 per-wavelength stage,
                                   fp64 Moffat fit */
#define MPSFR_PREC_F64      1   /* fp64 everywhere (reference arithmetic type) */

/* number of doubles per fitted stamp in fit_out */
#define MPSFR_NFIT         16
/* fit_out[k]: 0 peak  1 p0 (row centre, px)  2 q0 (col centre, px)  3 alpha (px)  4 n (beta)
 *             5 fwhm (px) = 2 alpha sqrt(2^(1/n) - 1)   6 chi2   7 iterations
 *             8 err_peak  9 err_p0  10 err_q0  11 err_alpha  12 err_n  13 err_fwhm (px)
 *             14 status (0 converged, 1 iteration cap, 2 singular; + MPSFR_FIT_ILL_CONDITIONED: see below)
 *             15 flux = peak pi alpha^2/(n-1)
 * Status bit MPSFR_FIT_ILL_CONDITIONED (4): the least-squares minimum was found, but the stamp does not pin
 * (fwhm, n) to the parity tolerance: n^2 sqrt((J^T J)^-1[eta, eta]) * peak >= 100, i.e. iid pixel noise of 1e-6 of
 * the peak moves n by 1e-4 or more (the covariance is the one err_n comes from).  That is the case where the stamp
 * is narrower than the PSF core (the 128^2 / 256^2 grids with the rescaled pixel scale, seeing > 2 arcsec at 512^2);
 * on the 512^2 ... 1280^2 grids with the SPARTA range of inputs the number stays below 30.
 * Rule of the circular fit for stamps without a Moffat in them (any data is accepted; nothing here is an error of the call): a row whose
 * status & 3 is 0 holds finite numbers, lies inside the search domain (fwhm > 1e-3 px, n >= 1/90) and is the
 * least-squares minimum.  Otherwise the row says so: 2 (singular) for an all-zero stamp, for a stamp with a NaN or
 * an infinite pixel (the other fields are then the start values or NaN), for a brightest pixel outside the
 * amplitude range of mpsfr_fit_stamps, and where the normal matrix cannot be factored; 1 (not converged) at the
 * iteration cap and where the iteration ended with n < 1/90, against the bound n = 0.01 of the domain, as on a constant or an
 * all-negative stamp, which have no maximum to fit.  A single hot pixel is a Moffat of vanishing width: it converges
 * to fwhm = 1e-3 px with the ill-conditioned bit set.
 */
#define MPSFR_FIT_ILL_CONDITIONED 4

/* Side of the AO-corrected zone grid (psfrec.py:103, 138: Dimpup * 2). */
#define MPSFR_DIM_AO       80

/* Create a context on HIP device `device_id` for an N x N spatial-frequency grid.
 * dim      : N, the `dim` argument of simul_psd_wfm (psfrec.py:37; compute_psf hard-codes 1280,
 *            psfrec.py:954-955).  Supported: 128, 256, 512, 1024, 1280.
 * dimpsf   : side of the output stamps (psfrec.py:658); only 40 is supported.
 * pixscale : arcsec per output pixel (psfrec.py:659, :899, :868).
 * Builds the wavelength- and row-independent telescope OTF (psfrec.py:784-790) once. */
int mpsfr_create(mpsfr_ctx** out, int device_id, int dim, int dimpsf, double pixscale,
                 int precision);
void mpsfr_destroy(mpsfr_ctx* ctx);
const char* mpsfr_last_error(void);

/* Tunables: "chunk_tasks" (tasks per pipeline pass, 0 = automatic: one pass up to 512 tasks /
 * 65536 stamps / 4 GiB of workspace, balanced passes beyond; a synchronous call -- host outputs --
 * of 8192 stamps or more: one pass per lane); "fast_exp" (mixed mode only,
 * default 1: hardware exp2 for the OTF); "fft_conv" (mixed mode only, default 1: the two 41x41
 * convolutions through 64-point FFTs instead of the direct form); "cu_partition" (default 0; 1: every lane's stream is created with a CU mask and owns
 * 1/lanes of the compute units -- measured slower, profiles/r05_experiments.md); "streams" (0 = automatic = 2,
 * or 1..4 pipeline lanes: consecutive chunks -- of one call and of consecutive asynchronous
 * calls -- go to successive HIP streams with their own workspaces so that one chunk's tail
 * overlaps the next one's body; results are independent of it except for the summation order of
 * psf_sum_out in multi-chunk calls); "pipeline_calls" (default 1: asynchronous calls rotate over
 * the lanes; 0: every call starts on the first lane); "prune_eps" (mixed mode only, default 1e-9:
 * the parts of the OTF half plane -- trailing lines, and 16 x 32 blocks inside the lines kept --
 * whose elements together weigh less than eps of OTF[0][0] (<= eps of the PSF peak, the sum of the OTF, whose
 * elements are all >= 0) are neither generated nor summed; 0 = everything); "tier_eps" (mixed mode, matrix-core
 * stage only, default 4e-6: the two precision tiers of that stage -- blocks whose largest element is below
 * 2^-29 of OTF[0][0] are dropped, blocks below 2^-18 run without the low fp16 half of the OTF -- are applied,
 * per task and wavelength, only as far as the OTF mass each of them leaves out stays below tier_eps / 2 of a
 * lower bound of the PSF peak (the OTF summed exactly over its first four lines; two on grids above 512^2); where it would not, the
 * thresholds of that (task, wavelength) are lowered until it does; the kernel for several directions has the floor
 * tier only and takes one floor per task, from the OTF of the task's shortest wavelength and the number of blocks.
 * 0 = no tiers; inf = tiers without a budget).
 * WHAT THE TWO TOGETHER GUARANTEE, for every input: with eps = prune_eps + tier_eps no pixel of a stamp before
 * the convolutions (psf_muse, psfrec.py:644-686) moves by more than eps of that stamp's peak -- up to the
 * stamp's normalisation to unit sum (psfrec.py:685), which in the worst case (all 1600 pixels moved the same
 * way) rescales the stamp by 1600 eps peak / sum; the Moffat fwhm, n and centre do not depend on the
 * normalisation, and the two convolutions (non-negative kernels of unit sum) do not increase a difference.
 * What the approximations really do on the workloads measured (tests/test_gpu_parity.py::
 * test_precision_tiers_of_the_matrix_core_stage): <= 3e-7 of the peak, |d beta| <= 2e-6, and the budget
 * is not reached (it is a guarantee for inputs nobody measured, e.g. an OTF whose coherent plateau sits just
 * below the floor); "otf_mfma" (mixed mode only,
 * default 1: the per-wavelength stage as split-fp16 contractions on the matrix cores; 0: LDS
 * FFTs on the vector pipe); "profile" (0/1: bracket every kernel launch
 * with HIP events on the stream it is launched on -- the event packets cost ~8 % of a step);
 * "profile_only" (-1 = all kernels, else the kernel id of mpsfr_profile_name to time alone);
 * "prune_eps_f64" (f64 mode only, default 1e-13, at most 1e-6: the same bound for the line pruning
 * of the reference-precision mode; 0 = everything).
 * "stage_a" (default 1 = automatic: from 512^2 on (at 256^2 with several directions) the structure function of a task is the sum of a
 * per-pixel polynomial in 1/L0^2 -- the fitting term, from tables built once per context -- and a pruned
 * transform of the 80 x 80 corrected zone (stage_a2.hip); below, and for any call with L0 < 7 m, the
 * full-size fp64 transforms of the PSD (stage_a.hip); 0 = always the full-size transforms, 2 = the
 * series form on every grid; the two forms agree to the rounding of the stored structure function).
 * Round 6, where a call's work is queued (results do not depend on any of these, bit for bit):
 * "persist_reserve" / "persist_reserve_mf" / "persist_reserve_a" (default -1 = automatic; 0..128): the two persistent
 * kernels (the matrix-core per-wavelength kernel / the column kernel of stage A's series form) launch ncu - R
 * workgroups instead of one per CU, so that R CUs -- R / 8 per XCD -- stay free for the latency-bound kernels of the
 * context's other lane while the big kernel runs; automatic: R = ncu / 8 when the call has chunks on several lanes
 * or the other lane still has work in flight, 0 for a call that runs alone (one lane loses 5 % to a reserve of 32,
 * two lanes gain 5 %: profiles/r06_experiments.md);
 * "head_fusion" (default 1: in the series form of stage A the spectra of a chunk's tip-tilt Moffat kernels are
 * computed by trailing workgroups of the patch's row kernel; 0: by a kernel of their own at the head of the call);
 * "support_skip" (default 1: the series form of stage A neither
 * evaluates nor stores the structure function on the pieces of a line where the telescope OTF is identically zero
 * -- a fifth of the half plane).  Those pieces of the buffer ("dphi0") hold zero after such a call: the buffer is
 * zeroed when it is allocated, and a series call clears it first when an earlier call on its lane wrote there (the
 * full-size form of a call with an L0 below 7 m or with "stage_a" 0, a series call with "support_skip" 0,
 * mpsfr_psf_from_psd) -- a result never depends on the calls before it.  mpsfr_debug_fetch("d0t_clears") counts
 * those clears.
 * "cold_stagger" (default 0 = off; 1 / 2: after the GPU has drained, the second lane's first chunk
 * waits once for the first lane's column transforms / per-wavelength preparation, so that the two
 * lanes do not start in step: +3 % in a sustained run of 100-row calls, -1 % on a burst of 20;
 * results do not depend on it).
 * Experiment switches of the matrix-core stage (results depend on them within the bound of "tier_eps"): "mf_kernel" (2 = thin-wave kernel with precision tiers
 * for one direction, 1 = the blocked kernel that several directions always use), "mf_permax"
 * (1..7 wavelengths per workgroup, default 6), "mf_floor" (default 1: blocks below the fp16
 * representation floor are skipped, within "tier_eps"), "mf_mid_log2" (default -18.01: blocks below 2^this of
 * OTF[0][0] run without the low half of the OTF, within "tier_eps"), "mf_clock" (phase time stamps; builds with
 * -DMPSFR_MF_CLOCK=1 only), "prune_fixed" (a fixed number of lines for the FFT form). */
int mpsfr_set_option(mpsfr_ctx* ctx, const char* key, double value);

/* Batched replacement of  Parallel(n_jobs)(delayed(compute_psf)(*args) ...)  (psfrec.py:1082-1083)
 * i.e. of compute_psf (psfrec.py:933-978) = simul_psd_wfm (:36-151) -> psf_muse (:644-686) ->
 * convolve_final_psf (:874-930) -> fit_psf_cube (:861-871), for ntask (seeing, GL, L0) triples.
 *
 * seeing, gl, l0 : [ntask] arcsec @500 nm, ground-layer fraction, outer scale [m]; seeing > 0, L0 > 0, 0 <= GL <= 1.
 *                  GL = 1 (no turbulence above the ground layer) makes the width of the residual tip-tilt kernel 0:
 *                  the reference's Moffat2DKernel(0, 2) is NaN there; the library returns the limit GL -> 1, the
 *                  identity kernel (in every entry point that takes GL, mpsfr_convolve_stamps included)
 * three_lgs      : [ntask] 0/1, three_lgs_mode of simul_psd_wfm (psfrec.py:86-91)
 * h              : layer altitudes [m] (psfrec.py:60); exactly two layers (psfrec.py:66 fixes two
 *                  wind directions)
 * wind_speed     : m/s; the reference uses np.full_like(h, 12.5) = 12 for integer h, 12.5 for
 *                  float h (psfrec.py:61) -- the caller decides
 * npsflin        : linear number of evaluation directions (psfrec.py:154-158), 1..5
 * lbda_nm        : [nl] wavelengths in nm
 * mask_rec/res   : [80*80] 0/1 cut-off masks of psfrec.py:257 (>=) and :435 (>) indexed
 *                  [i_fx][j_fy] like the reference's arrays, or NULL for the exact rule
 *                  |k| >= 24 / |k| > 24 on the integer frequency grid.  (In the reference these
 *                  masks depend on last-bit libm rounding; see DESIGN.md "cut-off masks".)
 *                  NOTE: NULL is NOT what the Python API passes by default.  muse_psfr_amd.compute_psf /
 *                  compute_psf_from_sparta default to cutoff_masks='host' -- the masks as the caller's NumPy
 *                  evaluates psfrec.py:257/:435, i.e. what the reference itself would compute on that
 *                  machine -- which differs from the exact rule on 44-52 of the 160 boundary pixels and
 *                  moves beta by up to 3e-3 (30x the parity tolerance).  A C caller that wants the results
 *                  of the Python default (or of a given reference installation) passes that installation's
 *                  masks; cutoff_masks='exact' in Python is this NULL.
 * psf_out        : [ntask][nl][dimpsf][dimpsf] final stamps (after both convolutions), or NULL
 * psf_sum_out    : [nl][dimpsf][dimpsf] sum over the ntask stamps (the caller divides by the
 *                  global task count to get PSF_MEAN, psfrec.py:1104), or NULL
 * fit_out        : [ntask][nl][MPSFR_NFIT] Moffat fit of every stamp, or NULL
 * on_device      : 0 = the three outputs are host pointers, the call returns with the results;
 *                  1 = device pointers on this context's device (results complete after mpsfr_sync);
 *                  2 = host pointers, asynchronous: the call returns once its work is queued (like
 *                  on_device = 1 it takes its turn on the pipeline lanes, so consecutive calls
 *                  overlap), the results travel to a pinned staging set of the library and reach the
 *                  caller's arrays in mpsfr_wait(ctx, mpsfr_last_ticket(ctx)) -- or in mpsfr_sync, or
 *                  when the fourth asynchronous call after this one is made (the ring of staging
 *                  sets has four); the arrays must stay allocated until then
 * All outputs are float64.  The call is asynchronous when on_device != 0. */
int mpsfr_reconstruct(mpsfr_ctx* ctx, int ntask, const double* seeing, const double* gl,
                      const double* l0, const uint8_t* three_lgs, const double h[2],
                      double wind_speed, int npsflin, int nl, const double* lbda_nm,
                      const uint8_t* mask_rec, const uint8_t* mask_res, double* psf_out,
                      double* psf_sum_out, double* fit_out, int on_device);

/* Field-resolved PSFs: one stamp and one Moffat fit per (row, field position, wavelength), at positions the caller
 * chooses.  The reference documents npsflin as the points where the PSF is reconstructed, then averages them
 * (psf_muse, psfrec.py:667-674); this keeps them apart.  Stamp (t, p, l) is what compute_psf would return for row t
 * if its PSD were the single direction p: psf_muse on that direction's PSD, convolve_final_psf with row t's
 * tip-tilt kernel, then the fit.  Nothing is averaged over positions.
 *
 * npos, pos_arcsec : [npos][2] (x, y) in arcsec, 1 <= npos <= 25, in the convention of direction_perf (x is
 *                    dirperf[0]); every coordinate finite with |x|, |y| <= 60 (twice the WFM half-field).
 *                    direction_perf(npsflin) passed here gives exactly the directions of npsflin.  Anything else
 *                    returns MPSFR_E_INVALID and touches nothing.
 * psf_out          : [ntask][npos][nl][dimpsf][dimpsf] final stamps, or NULL
 * psf_sum_out      : [npos][nl][dimpsf][dimpsf] sum over the ntask rows, or NULL
 * fit_out          : [ntask][npos][nl][MPSFR_NFIT], fields and status bits as for mpsfr_reconstruct, or NULL
 * Every other argument, on_device 0 / 1 / 2 included (lanes, tickets, mpsfr_wait, mpsfr_sync, mpsfr_abandon,
 * mpsfr_stream_wait, mpsfr_wait_event), means what it means for mpsfr_reconstruct.  The eps = prune_eps + tier_eps
 * guarantee of mpsfr_set_option holds PER STAMP: each (row, position) stamp is held to it on its own.
 * One position at (0, 0) is mpsfr_reconstruct with npsflin = 1, bit for bit; every position is computed
 * independently of the others in the call (psf_out and fit_out equal a call with that position alone, bit for bit).
 * After a field call, mpsfr_debug_fetch's per-task shapes ("pre", "vkeep", "mf_work") count (row, position) pairs:
 * [chunk tasks][npos]...; "dphi0" and "ao_tables" have npos directions. */
int mpsfr_reconstruct_field(mpsfr_ctx* ctx, int ntask, const double* seeing, const double* gl,
                            const double* l0, const uint8_t* three_lgs, const double h[2],
                            double wind_speed, int npos, const double* pos_arcsec,
                            int nl, const double* lbda_nm, const uint8_t* mask_rec,
                            const uint8_t* mask_res, double* psf_out, double* psf_sum_out,
                            double* fit_out, int on_device);

/* Multi-layer Cn2 profiles with per-layer wind.  The calls above model the reference's fixed atmosphere: two layers
 * at h[2], one wind speed, the directions (0.628163, -0.326497) rad (simul_psd_wfm, psfrec.py:61, 66).  The model
 * itself (dsp4muse, psfrec.py:531-613) takes any number of layers, and the residual PSD of the corrected zone is
 * LINEAR in their weights:  PSD_AO = VK sum_k cn2_k T_k + noise,  where T_k depends only on layer k's altitude and
 * wind, the LGS geometry and the direction.  So the library builds one table T_k per layer, once per profile, and
 * every row mixes them with its own weights on the 80 x 80 zone; nothing else of the pipeline changes.
 *
 * nlayer            1 .. MPSFR_MAX_LAYERS
 * h, wind_speed,    [nlayer] altitudes [m] in [0, 50000], wind speeds [m/s] in [0, 100], wind directions [rad]
 *   wind_dir        (the reference's Cn2 heights, vent and arg_v); all finite
 * cn2               [ntask][nlayer] weights, finite and >= 0, each row with a positive sum; each row is normalised
 *                   to sum 1 (psfrec.py:57-58)
 * gl                [ntask] only sets the tip-tilt kernel of convolve_final_psf (psfrec.py:881-883)
 * npos = 0          the npsflin (1..5) directions, averaged: outputs as for mpsfr_reconstruct
 * npos >= 1         field positions pos_arcsec [npos][2] (rules of mpsfr_reconstruct_field), npsflin must be 0:
 *                   outputs as for mpsfr_reconstruct_field
 * Every other argument, on_device 0 / 1 / 2 included, means what it means for mpsfr_reconstruct.  A bad profile,
 * weight or npsflin / npos combination returns MPSFR_E_INVALID before anything is queued and touches nothing.
 * The profile h = (100, 10000), wind_speed = (ws, ws), wind_dir = (0.628163, -0.326497), cn2 = [gl, 1 - gl] per row
 * is mpsfr_reconstruct / mpsfr_reconstruct_field with h = (100, 10000) and wind_speed = ws, bit for bit.
 * A layer whose weight is 0 in every row is left out (the result is that of the profile without it, bit for bit).
 * The AO tables are cached on the whole profile (layers, altitudes, winds), the directions and the masks.  After a
 * profile call mpsfr_debug_fetch("ao_tables") is [2 geometries][ndir][max(nlayer, 2) + 1][80][80]: the layer
 * tables, then the noise (a single layer has a second table of zeros).
 *
 * mpsfr_simul_psd_profile is mpsfr_simul_psd for a profile: psd_out [ndir][dim][dim] in the units and layout of
 * mpsfr_simul_psd, ndir = npsflin^2 (npos = 0) or npos (the PSD at each position, npsflin = 0).  cn2 [nlayer]. */
#define MPSFR_MAX_LAYERS 8
int mpsfr_reconstruct_profile(mpsfr_ctx* ctx, int ntask, const double* seeing, const double* gl,
                              const double* l0, const uint8_t* three_lgs,
                              int nlayer, const double* h, const double* wind_speed, const double* wind_dir,
                              const double* cn2, int npsflin, int npos, const double* pos_arcsec,
                              int nl, const double* lbda_nm, const uint8_t* mask_rec, const uint8_t* mask_res,
                              double* psf_out, double* psf_sum_out, double* fit_out, int on_device);
int mpsfr_simul_psd_profile(mpsfr_ctx* ctx, double seeing, double l0, int three_lgs,
                            int nlayer, const double* h, const double* wind_speed, const double* wind_dir,
                            const double* cn2, int npsflin, int npos, const double* pos_arcsec,
                            const uint8_t* mask_rec, const uint8_t* mask_res, double* psd_out);

/* Band-integrated PSFs.  The PSF of a broadband image -- white light, a synthetic filter, a narrow band summed over a
 * line -- is the spectrum-weighted mean of the monochromatic PSFs over the band,
 *     PSF_band = int T(lambda) f(lambda) PSF_lambda dlambda / int T(lambda) f(lambda) dlambda,
 * with T the throughput and f the source's f_lambda: not the PSF at the central wavelength.  The caller gives the
 * quadrature weights of each band on the lbda_nm grid (e.g. band_weights in psfrec.py); the library reduces the
 * per-wavelength stamps of every (row, position) on the GPU and fits only the band stamps.  The per-wavelength stamps
 * never leave the device and no per-wavelength fit runs.
 *
 * nband, weights    : 1 <= nband <= MPSFR_MAX_BANDS bands, weights [nband][nl], finite and >= 0, each band with a
 *                     positive sum.  Each band is normalised to sum 1 here: w_bl / sum_l w_bl = w^_bl (a power-of-two
 *                     scale of a band's weights changes nothing, bit for bit).
 * npos = 0          : the npsflin (1..5) directions, averaged:
 *                       band_out [ntask][nband][dimpsf][dimpsf], band_sum_out [nband][dimpsf][dimpsf] (sum over the
 *                       rows), band_fit_out [ntask][nband][MPSFR_NFIT]
 * npos >= 1         : field positions pos_arcsec [npos][2] (rules of mpsfr_reconstruct_field), npsflin must be 0:
 *                       each output gains an [npos] axis after the row axis, as in mpsfr_reconstruct_field
 * Band stamp (t, b) is  sum_l w^_bl x  the stamp mpsfr_reconstruct / mpsfr_reconstruct_field returns for (t, l),
 * summed in fp64 in wavelength order (the mixed mode reduces its float stamps).  A band that holds one wavelength at
 * weight 1 is that stamp exactly.  band_fit_out is the Moffat fit of the band stamp, with the fields and status bits
 * of MPSFR_NFIT.  The eps = prune_eps + tier_eps guarantee of mpsfr_set_option holds per band stamp: a convex
 * combination of stamps that each meet it.  Every other argument, on_device 0 / 1 / 2 included (tickets, mpsfr_wait,
 * mpsfr_sync, mpsfr_abandon, the staging ring), means what it means for mpsfr_reconstruct.  A bad nband, weight or
 * npsflin / npos combination returns MPSFR_E_INVALID before anything is queued and touches nothing.
 * Cn2 profiles (mpsfr_reconstruct_profile) with bands are not supported yet: a follow-up. */
#define MPSFR_MAX_BANDS 16
int mpsfr_reconstruct_band(mpsfr_ctx* ctx, int ntask, const double* seeing, const double* gl,
                           const double* l0, const uint8_t* three_lgs, const double h[2], double wind_speed,
                           int npsflin, int npos, const double* pos_arcsec,
                           int nl, const double* lbda_nm, int nband, const double* weights,
                           const uint8_t* mask_rec, const uint8_t* mask_res,
                           double* band_out, double* band_sum_out, double* band_fit_out, int on_device);

/* The same over several devices: the reference's  Parallel(n_jobs=...)  fans the rows out over
 * worker processes (psfrec.py:1082-1083); here the rows go in contiguous, balanced shards (the
 * first ntask % nctx contexts take one row more) to `nctx` contexts -- normally one per device,
 * created by the caller with the same dim, dimpsf, pixscale and precision -- one host thread per
 * context.  Host buffers only, synchronous.  Per-row outputs are those of the single-context
 * call; psf_sum_out adds the shards' sums in context order.  ntask < nctx: the first context
 * takes everything. */
int mpsfr_reconstruct_multi(mpsfr_ctx* const* ctxs, int nctx, int ntask, const double* seeing,
                            const double* gl, const double* l0, const uint8_t* three_lgs,
                            const double h[2], double wind_speed, int npsflin, int nl,
                            const double* lbda_nm, const uint8_t* mask_rec,
                            const uint8_t* mask_res, double* psf_out, double* psf_sum_out,
                            double* fit_out);

/* The same without waiting for the GPUs: every context takes its shard as an asynchronous host-output call
 * (on_device = 2 of mpsfr_reconstruct: no host thread, the call returns once the shards are queued), and
 * mpsfr_wait_multi(ctxs, nctx) -- same contexts, same order -- blocks until all of them have finished, hands
 * the per-row outputs to the caller's arrays and adds the shards' stamp sums in context order into the
 * psf_sum_out of the call.  One such call may be pending per ctxs[0]; the output arrays must stay allocated
 * until mpsfr_wait_multi returns (or mpsfr_abandon on every context gives them up).  Several tables -- or the
 * parts of one -- can so be kept in flight on several devices, like on_device = 2 does on one.
 * A shard that fails (the error names its context) ABANDONS every pending asynchronous call of EVERY context of
 * the call -- the shards already queued and any single on_device = 2 call still in flight on them: their arrays
 * are never written, mpsfr_wait on their tickets fails.  The refusals made before anything is queued (NULL
 * context, a multi-context call already pending on ctxs[0], contexts of different shape) touch nothing. */
int mpsfr_reconstruct_multi_async(mpsfr_ctx* const* ctxs, int nctx, int ntask, const double* seeing,
                            const double* gl, const double* l0, const uint8_t* three_lgs,
                            const double h[2], double wind_speed, int npsflin, int nl,
                            const double* lbda_nm, const uint8_t* mask_rec,
                            const uint8_t* mask_res, double* psf_out, double* psf_sum_out,
                            double* fit_out);
int mpsfr_wait_multi(mpsfr_ctx* const* ctxs, int nctx);

/* Replacement of fit_psf_cube (psfrec.py:861-871) on caller-provided stamps, e.g. the mean PSF
 * (psfrec.py:1105).  stamps: [nstamp][dimpsf][dimpsf] float64; fit_out: [nstamp][MPSFR_NFIT].
 * Amplitude range: the brightest pixel of a stamp must lie in [2^-40, 2^40] (9.1e-13 ... 1.1e12) in modulus; a stamp
 * outside it is refused with status 2 (a caller with stamps in physical flux units scales them by a power of two,
 * which is exact).  The iterations run in fp32 in both precision modes and their sums scale with the square of the
 * peak I: the gradient terms of the wing pixels (I^2 2^-34 at the last steps) leave the normal range of fp32 below
 * I = 2^-46 and the fit then stops short of the minimum; from I = 2^50 on the normal matrix overflows.  Inside the range:
 *   [2^-20, 2^40]  a factor 2^k changes no bit of (fwhm, n, alpha, p0, q0, the other err_* columns, status,
 *                  iterations), and peak, flux, err_peak scale by 2^k and chi2 by 4^k exactly;
 *   [2^-40, 2^-20) the parameters and the status are right to the tolerances of the precision mode, but not bit for
 *                  bit: the squared residuals of a nearly exact fit (I^2 2^-54 and less) are subnormal in fp32
 *                  there, so chi2 and the err_* columns, which carry chi2 / dof, are not exact multiples.
 * The circular fits inside mpsfr_reconstruct and its siblings follow the same rule (their stamps have sum 1: peaks of
 * 1e-4 ... 1).  The elliptical fit (mpsfr_fit_stamps_elliptical and the elliptical columns) is another kernel with the
 * same range: a brightest pixel outside [2^-40, 2^40] in modulus is refused with status 2 in both precision modes;
 * inside it the status, the parameters and chi2, flux and the err_* columns (scaled by the powers of the factor) are
 * right to the tolerances of the precision mode.  Bit identity under a factor 2^k is not promised there.
 * on_device = 1: both pointers are device pointers and the call is queued on the context stream, after every call
 * queued so far on this context: stamps written by a device-output mpsfr_reconstruct* are complete when it reads them. */
int mpsfr_fit_stamps(mpsfr_ctx* ctx, int nstamp, const double* stamps, double* fit_out,
                     int on_device);

/* What a call writes.  This holds for the fifteen stamp, frame and cube entry points below (mpsfr_fit_stamps_elliptical,
 * _observed, _psf, mpsfr_fit_groups_psf, mpsfr_fit_spectra_psf, mpsfr_stamp_metrics, mpsfr_cut_stamps,
 * mpsfr_render_stars, mpsfr_find_stars, mpsfr_group_stars, mpsfr_fit_frame_psf, _free, mpsfr_fit_cube_psf, _free,
 * mpsfr_frame_background), in the host and in the device form alike:
 *   - a call that returns MPSFR_OK writes EVERY element of every output array it is given, at the size stated for the
 *     array: a row that holds no result -- a stamp or star with status 1 or 2, a star left out of one layer, a layer with
 *     nothing to fit, the rows of mpsfr_find_stars from count_out[0] up to max_stars, the rows of mpsfr_group_stars
 *     from the number of groups up to max_groups and the doubles of shift_out that belong to no member -- is written
 *     with the zeros, NaNs or fillers stated for it, never left as the caller's buffer held it;
 *   - it writes nothing behind that size: the rows beyond max_stars or max_groups of a frame with more peaks or groups
 *     do not exist for the call;
 *   - an optional output passed as NULL is not written, and changes no other output;
 *   - a refused call (MPSFR_E_INVALID) writes nothing.
 * No output depends on what the context ran before: the work memory of these calls is reused from
 * call to call and never cleared, and every word a call reads from it the same call has written. */

/* Elliptical Moffat fit of caller-provided stamps (mpdaf's moffat_fit(circular=False), which the reference does not
 * use): I (1 + Q)^-n with Q = (g / alpha^2) [(1 - e1) x^2 - 2 e2 x y + (1 + e1) y^2], g = 1 / sqrt(1 - e1^2 - e2^2),
 * x = q - q0, y = p - p0; alpha is the geometric mean of the semi-axes.  With e = sqrt(e1^2 + e2^2):
 * alpha_major = alpha ((1 + e)/(1 - e))^(1/4), alpha_minor = alpha ((1 - e)/(1 + e))^(1/4), the major axis at
 * rot = atan2(e2, e1) / 2, FWHM_axis = 2 alpha_axis sqrt(2^(1/n) - 1).  At e = 0 the model is mpsfr_fit_stamps's.
 * Arguments and on_device as mpsfr_fit_stamps: with on_device = 1 both pointers are device pointers and the call is
 * queued on the context stream (e.g. after a device-output mpsfr_reconstruct_field / mpsfr_reconstruct_profile).
 * stamps: [nstamp][dimpsf][dimpsf] float64; fit_out: [nstamp][MPSFR_NFIT_ELL].  Errors: the reduced-chi2 covariance
 * (dof = npix - 7), propagated to first order.  A stamp whose elongation is not determined (e -> 0) has a finite rot
 * and a large err_rot (at most 180); that is not a failure.  Timed under the fit's profiling id.
 * Rule for stamps without such a Moffat in them (any data is accepted on_device; nothing here is an error of the
 * call), the circular fit's: a row whose status & 3 is 0 holds finite numbers only, lies inside the search domain
 * (fwhm > 1e-3 px, n >= 1/90, |e| <= 0.94, i.e. b/a >= 0.176) and is the least-squares minimum.  Otherwise the row
 * says so: 2 (singular) for an all-zero stamp, for a stamp with a NaN or an infinite pixel, for a brightest pixel
 * outside the amplitude range [2^-40, 2^40] of mpsfr_fit_stamps (the other fields are then the start values or NaN),
 * and where the normal matrix cannot be factored; 1 (not converged) at the iteration cap, where the iteration ended
 * with n < 1/90 against the bound n = 0.01 of the domain (a constant or an all-negative stamp), and where it ended
 * with |e| > 0.94 against the bound |e| = 0.95: a stamp more elongated than b/a = 0.16 has its minimum outside the
 * domain, and the row is the point of the boundary the steps were cut at, not a minimum.  A single hot pixel is a
 * Moffat of vanishing width: away from the edge it converges with the ill-conditioned bit set. */
#define MPSFR_NFIT_ELL 24
/* fit_out[k]: 0 peak  1 p0  2 q0  3 alpha_major (px)  4 alpha_minor (px)  5 n  6 rot (deg, [0,180), from +q towards +p)
 *             7 fwhm_major (px)  8 fwhm_minor (px)  9 chi2  10 iterations  11 err_peak  12 err_p0  13 err_q0
 *             14 err_fwhm_major  15 err_fwhm_minor  16 err_rot (deg)  17 err_n
 *             18 status (codes and MPSFR_FIT_ILL_CONDITIONED bit as fit_out[14] of MPSFR_NFIT, same rule on n, and the
 *                rule on |e| above; the number behind the bit is taken from the 7-variable normal matrix)
 *             19 flux = peak pi alpha_major alpha_minor / (n - 1)  20 err_flux  21..23 zero (reserved) */
int mpsfr_fit_stamps_elliptical(mpsfr_ctx* ctx, int nstamp, const double* stamps, double* fit_out, int on_device);

/* Weighted Moffat fit of observed stars (mpdaf's moffat_fit(weight=True, fit_back=..., circular=...)): the minimum of
 *     sum over the used pixels of (model - data)^2 / var,   model = Moffat [+ b]
 * in the variables I, p0, q0, w, [e1, e2,] eta = 1/n, [b] of mpsfr_fit_stamps_elliptical (circular without
 * MPSFR_FIT_ELLIPTICAL), with a constant background b under MPSFR_FIT_BACKGROUND.
 * stamps: [nstamp][dimpsf][dimpsf] float64; var: the same shape, or NULL for unit weights.  A pixel is USED iff its
 * value is finite and, when var is given, its variance is finite and > 0; every other pixel is left out of every sum
 * and its stored value never matters (NaN data, or var <= 0 / NaN / inf, is the mask).  A +-inf value under a valid
 * variance makes the row status 2.
 * fit_out: [nstamp][MPSFR_NFIT_ELL] in the elliptical layout, with 21 background, 22 err_background (both 0 without
 * MPSFR_FIT_BACKGROUND) and 23 the number of used pixels; without MPSFR_FIT_ELLIPTICAL alpha_major = alpha_minor,
 * fwhm_major = fwhm_minor, rot = err_rot = 0.  Errors: sqrt(diag((J^T W J)^-1) chi2 / dof), dof = n_used - npar with
 * npar = 5 ... 8, propagated to first order; chi2 (field 9) is the weighted sum.  A constant factor on var changes
 * no parameter and no error.
 * Status (field 18): 0, 1, 2 as for mpsfr_fit_stamps_elliptical; 2 also when n_used < npar + 1, when no used pixel
 * exceeds the start background (the mean of the used pixels of the outer ring), and when the brightest used pixel
 * lies outside [2^-40, 2^40] in modulus (the stamp is normalised by a power of two internally), and when a used
 * pixel exceeds 2^60 times the brightest one in modulus (a deep negative outlier that was not masked).  The
 * MPSFR_FIT_ILL_CONDITIONED bit is not set by this entry point: its threshold is defined for unit weights, and the
 * formal errors carry the information here.  A row whose status & 3 is 0 holds finite numbers only.
 * A stamp's row depends on that stamp only, bit for bit.  on_device as mpsfr_fit_stamps_elliptical (stamps, var and
 * fit_out are device pointers, the call is queued on the context stream); timed under the fit's profiling id.
 * MPSFR_E_INVALID, with fit_out untouched: nstamp < 1, unknown flag bits, NULL stamps or fit_out. */
#define MPSFR_FIT_BACKGROUND 1   /* fit a constant background b: model = Moffat + b */
#define MPSFR_FIT_ELLIPTICAL 2   /* the (e1, e2) model of mpsfr_fit_stamps_elliptical; else circular */
int mpsfr_fit_stamps_observed(mpsfr_ctx* ctx, int nstamp, const double* stamps, const double* var, int flags,
                              double* fit_out, int on_device);

/* PSF-model fit of observed stars: the model stamp itself, resampled, is fitted to the star.  For star stamp d with
 * optional variance var, and model stamp P ([dimpsf][dimpsf], any real values), the minimum over the used pixels of
 *     sum (m - d)^2 / var,   m(p, q) = F P~(p - dp, q - dq) + b,   P~(y, x) = sum_kl c(y - k) c(x - l) P[k][l]
 * with c the Keys cubic-convolution kernel (a = -1/2): c(t) = 1.5|t|^3 - 2.5|t|^2 + 1 for |t| <= 1,
 * -0.5|t|^3 + 2.5|t|^2 - 4|t| + 2 for 1 < |t| < 2, 0 beyond; P counts as zero outside its pixels (a model whose
 * wings reach the edge of its stamp is cut there: the background of such a fit is biased).  The result is the weighted
 * chi2 of the model against the data together with the star's flux, position and background: PSF-fitting photometry.
 * Variables: (F, dp, dq, [b]); under MPSFR_FIT_FIXED_SHIFT (F, [b]) at the given shift, which is a linear problem
 * (iterations = 1); b only under MPSFR_FIT_BACKGROUND.  Domain: |dp|, |dq| <= MPSFR_FIT_PSF_MAX_SHIFT pixels.
 * stamps, var: as mpsfr_fit_stamps_observed (the same rule for the used pixels; var NULL: unit weights).
 * psf: [npsf][dimpsf][dimpsf]; psf_index: [nstamp] values in 0..npsf-1, the model stamp of every star, or NULL, which
 * requires npsf == nstamp and pairs them one to one.  shift: [nstamp][2] (dp, dq) start values -- the fixed values
 * under MPSFR_FIT_FIXED_SHIFT, which requires it -- or NULL: the start is then the brightest used pixel of the star
 * minus the brightest pixel of the model stamp (each the first maximum in row-major order), brought into the domain.
 * F and b start from the closed-form weighted linear solve at that shift.
 * fit_out: [nstamp][MPSFR_NFIT_PSF]:
 *   0 F  1 dp  2 dq  3 back  4 chi2 (the weighted sum)  5 iterations  6 err_F  7 err_dp  8 err_dq  9 err_back
 *   10 status  11 n_used  12 flux = F sum(P)  13 err_flux = err_F |sum(P)|  14, 15 zero (reserved)
 * Fields of variables that are not fitted are 0; a fixed (dp, dq) is echoed.  Errors: sqrt(diag((J^T W J)^-1) chi2 /
 * dof), dof = n_used - npar, npar = 1 ... 4, the convention of mpsfr_fit_stamps_observed: a caller whose variances are
 * the true ones divides the errors by sqrt(chi2 / dof).
 * Status: 0 a minimum; 1 the iteration cap, or an iteration that ended against the bound of the shift (the values are
 * the last iterate); 2 not fitted (every other field but n_used is 0) or no covariance: an infinite pixel under a
 * valid variance, n_used < npar + 1, a model stamp that is all zero or not finite, the brightest used pixel of the star
 * or the brightest pixel of the model stamp outside [2^-40, 2^40] in modulus (both are normalised by powers of two
 * internally), a used pixel beyond 2^60 times the brightest one in modulus, a singular normal matrix.  The
 * MPSFR_FIT_ILL_CONDITIONED bit is never set.  A row whose status & 3 is 0 holds finite numbers only.
 * A star's row depends on that star and its model stamp only, bit for bit.  A constant factor on var changes no
 * parameter and no error; a factor 2^k on the data with 4^k on var scales F, back, flux and their errors by 2^k.
 * on_device as mpsfr_fit_stamps_observed: with 1, stamps, var, psf, psf_index, shift and fit_out are all device
 * pointers and the call is queued on the context stream (e.g. behind a device-output mpsfr_reconstruct_field, whose
 * stamps are then the model); timed under the fit's profiling id.
 * MPSFR_E_INVALID before anything is queued, with fit_out untouched: nstamp < 1 or npsf < 1; NULL stamps, psf or
 * fit_out; unknown flag bits or MPSFR_FIT_ELLIPTICAL; psf_index NULL with npsf != nstamp; MPSFR_FIT_FIXED_SHIFT
 * without shift; and, for host pointers, an index out of range or a shift that is not finite or outside the domain --
 * in the device form these two make that row status 2 instead. */
#define MPSFR_NFIT_PSF 16
#define MPSFR_FIT_FIXED_SHIFT 4      /* with MPSFR_FIT_BACKGROUND (1); MPSFR_FIT_ELLIPTICAL is refused here */
#define MPSFR_FIT_PSF_MAX_SHIFT 8.0  /* pixels */
int mpsfr_fit_stamps_psf(mpsfr_ctx* ctx, int nstamp, const double* stamps, const double* var, int npsf,
                         const double* psf, const int32_t* psf_index, const double* shift, int flags,
                         double* fit_out, int on_device);

/* PSF-model fit of blended stars: all sources of a group (2 to MPSFR_MAX_GROUP stars that share the pixels of one
 * stamp) are fitted at once with one model stamp -- DAOPHOT's NSTAR for the reconstructed PSF.  Per stamp d with optional
 * variance var, over the used pixels, the minimum of
 *     sum (m - d)^2 / var,   m(p, q) = sum_{k < nsrc} F_k P~(p - dp_k, q - dq_k) + b
 * with P~ the Keys resampling of the stamp's model P exactly as mpsfr_fit_stamps_psf defines it (zero outside its
 * pixels).  All sources of a stamp share the model stamp psf[psf_index[stamp]] (one to one when psf_index is NULL).  The
 * rule for the used pixels, the weights and the power-of-two normalisations are those of mpsfr_fit_stamps_psf.
 * nsrc: 2 .. MPSFR_MAX_GROUP, the same for every stamp of the call (groups of several sizes: one call per size; one
 * source is mpsfr_fit_stamps_psf and nsrc = 1 is refused).  shift: [nstamp][nsrc][2], always required: (dp_k, dq_k), the
 * displacement of each source from the model stamp's own position, in pixels.  Three modes:
 *   free    (neither shift flag)       variables F_k, dp_k, dq_k, [b]; npar = 3 nsrc + [1] <= 13; shift: start values
 *   common  (MPSFR_FIT_COMMON_SHIFT)   variables F_k, Dp, Dq, [b]; npar = nsrc + 2 + [1]; dp_k = shift_k,p + Dp (and q):
 *                                      the relative positions are the caller's (a catalogue); D starts at 0
 *   fixed   (MPSFR_FIT_FIXED_SHIFT)    variables F_k, [b]: linear, solved in closed form (iterations = 1)
 * b only under MPSFR_FIT_BACKGROUND.  Domain: every source keeps |dp_k|, |dq_k| <= MPSFR_FIT_PSF_MAX_SHIFT throughout
 * (in common mode after D is added): a step that takes any source outside is refused, and a fit that ends resting on
 * the bound has status 1.  A neighbour farther than 8 pixels from the stamp centre cannot be a member of the group.
 * The F_k and b start from the closed-form weighted linear solve at the given positions; the iteration is that of
 * mpsfr_fit_stamps_psf, the step size measured relative to max_k |F_k| for every F_k and b and in pixels for positions.
 * fit_out: [nstamp][MPSFR_NFIT_GROUP]:
 *   0 back  1 err_back  2 chi2 (the weighted sum)  3 iterations  4 status  5 n_used  6 nsrc  7 zero
 *   8 + 8k, source k:  0 F  1 dp  2 dq  3 err_F  4 err_dp  5 err_dq  6 flux = F sum(P)  7 err_flux = err_F |sum(P)|
 *   40 .. 45: the correlation coefficients of (F_i, F_j) from the covariance, for (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
 *   -- how blended two fluxes are; pairs that do not exist are 0.  46, 47 zero.
 * Sources >= nsrc are zeros; fixed positions are echoed with error 0; in common mode every source's err_dp / err_dq is
 * the error of Dp / Dq.  Errors: sqrt(diag((J^T W J)^-1) chi2 / dof), dof = n_used - npar.
 * Status as mpsfr_fit_stamps_psf (0 / 1 / 2; MPSFR_FIT_ILL_CONDITIONED is never set).  Status 2 also covers
 * n_used < npar + 1, a singular start solve (two sources at the same position) and, in the device form, an index out
 * of range or a given position that is not finite or outside the domain.  A status-2 row is zeros except status,
 * n_used and nsrc.  A row whose status & 3 is 0 holds finite numbers only.
 * A stamp's row depends on that stamp, its model and its positions only, bit for bit: not on the batch or on the
 * stamp's place in it.  A constant factor on var changes no parameter and no error.  2^k on the data with 4^k on var
 * scales every F, back, flux and their errors by 2^k exactly and changes no other bit; 2^k on the model scales every F
 * (and err_F) by 2^-k exactly.  Values of unused pixels never matter.  Permuting the sources of a group permutes the
 * result to rounding only, not bit for bit: the order of the sums changes.
 * on_device: 0 synchronous on host pointers; 1: stamps, var, psf, psf_index, shift and fit_out are all device pointers
 * and the call is queued on the context stream behind earlier calls (e.g. a device-output mpsfr_reconstruct_field,
 * whose stamps are then the model); timed under the fit's profiling id.
 * MPSFR_E_INVALID before anything is queued, with fit_out untouched: nstamp < 1, npsf < 1 or nsrc outside 2 .. 4; NULL
 * stamps, psf, shift or fit_out; both shift flags, MPSFR_FIT_ELLIPTICAL or an unknown bit; psf_index NULL with
 * npsf != nstamp; and, for host pointers, an index out of range or a position that is not finite or outside the
 * domain. */
#define MPSFR_MAX_GROUP 4            /* sources per stamp */
#define MPSFR_NFIT_GROUP 48          /* doubles per fitted group */
#define MPSFR_FIT_COMMON_SHIFT 8     /* beside MPSFR_FIT_BACKGROUND (1), MPSFR_FIT_FIXED_SHIFT (4) */
int mpsfr_fit_groups_psf(mpsfr_ctx* ctx, int nstamp, int nsrc, const double* stamps, const double* var, int npsf,
                         const double* psf, const int32_t* psf_index, const double* shift, int flags,
                         double* fit_out, int on_device);

/* PSF-model fit of star cubes: nl images of one star, fitted at once with one position and a flux per layer -- the
 * spectrum of a star from the per-wavelength PSFs.  Per star, over the used pixels of all fitted layers, the minimum of
 *     sum_l sum_pq (m_l - d_l)^2 / var_l,   m_l(p, q) = F_l P~_l(p - dp - sp x_l, q - dq - sq x_l) + b_l
 * with P~_l the Keys resampling of the layer's model stamp exactly as mpsfr_fit_stamps_psf defines it.  Variables: F_l
 * of every layer, b_l of every layer under MPSFR_FIT_BACKGROUND, and theta = (dp, dq), or (dp, dq, sp, sq) under
 * MPSFR_FIT_DRIFT: a position that moves linearly with x_l (a chromatic drift).  Domain: |dp + sp x_l| and
 * |dq + sq x_l| <= MPSFR_FIT_PSF_MAX_SHIFT for every fitted layer; a step that leaves it is refused.
 * cubes, var: [nstar][nl][dimpsf][dimpsf] (var NULL: unit weights); the rule for the used pixels and the weights are
 * those of mpsfr_fit_stamps_psf, per layer.  psf: [npsf][nl][dimpsf][dimpsf] -- the device output of
 * mpsfr_reconstruct_field ([ntask npos][nl]...) is exactly this; psf_index: [nstar] values in 0..npsf-1, or NULL, which
 * requires npsf == nstar.  shift: [nstar][2] start values of (dp, dq), or NULL.  x: [nl], ALWAYS a host pointer,
 * required under MPSFR_FIT_DRIFT and ignored otherwise: finite values in [-1, 1] of which at least two differ.
 * A layer is left out (layer status 2, its other fields zero except n_used) when it has fewer than nlin + 1 used pixels
 * (nlin = 1, or 2 with the background), holds an infinite pixel under a valid variance, or its model stamp is all zero,
 * not finite, or has its largest |P| outside [2^-40, 2^40].  The other layers are fitted without it: a masked sky-line
 * layer is the ordinary case.
 * The fit is a variable projection: at a given theta the (F_l, b_l) of a layer are its closed-form weighted linear
 * solve, and the Levenberg-Marquardt iteration of mpsfr_fit_stamps_psf descends in theta alone (step size in pixels) on
 * the reduced normal equations; its minimum is that of the joint problem over all variables.  Start: `shift` if given,
 * else the first maximum of sum_l d_l / var_l (over the used pixels of the fitted layers) minus the first maximum of
 * sum_l P_l, brought into the domain; sp = sq = 0.  This default only serves stars whose collapsed image stands above
 * the noise: once the peak signal-to-noise per layer is below about 3.5 / sqrt(nl) it lands on a noise pixel.  Faint
 * stars are started from a catalogue position.
 * fit_out: [nstar][MPSFR_NFIT_SPEC + MPSFR_NFIT_SPEC_LAYER nl]:
 *   head: 0 dp  1 dq  2 sp  3 sq  4 .. 7 their errors  8 chi2 (the weighted sum)  9 iterations  10 status
 *         11 N_used (used pixels of the fitted layers)  12 L (fitted layers)  13 dof  14, 15 zero
 *   layer l at 16 + 10 l: 0 F  1 back  2 err_F  3 err_back  4 flux = F sum(P_l)  5 err_flux = err_F |sum(P_l)|
 *         6 chi2_l  7 n_used_l  8 status_l (0 or 2)  9 zero
 * Errors: those of the joint problem, sqrt(diag((J^T W J)^-1) chi2 / dof), dof = N_used - (npos + nlin L), npos = 2 or
 * 4: cov(theta) = S^-1 chi2 / dof with S the reduced normal matrix, and the covariance of (F_l, b_l) carries the
 * uncertainty of the shared position.
 * Star status: 0 a minimum; 1 the iteration cap, or the fit ended resting on the bound of the domain; 2 not fitted:
 * the row is zeros except status, N_used, L and the per-layer n_used and status.  Status 2 covers: no fitted layer;
 * dof < 1; drift with fewer than two distinct x among the fitted layers; the brightest used pixel of the fitted layers
 * outside [2^-40, 2^40] in modulus or a used pixel beyond 2^60 times it (the amplitude rules of
 * mpsfr_fit_stamps_psf); a layer whose linear solve is singular at the start; and, in the device form, an index out of
 * range or a start that is not finite or outside the domain.  A row whose status & 3 is 0 holds finite numbers only.
 * A star's row depends on that star, its models, x and the flags only, bit for bit: not on the batch or the star's
 * place in it.  A constant factor on var changes no parameter and no error.  2^k on the data with 4^k on var scales
 * every F, back, flux and their errors by 2^k exactly; 2^k on one layer's model scales that layer's F and err_F by
 * 2^-k exactly.  Values of unused pixels and of left-out layers never matter.
 * Both precision modes of a context run this fit in fp64 throughout: it has no float path, and a mixed context gives
 * the rows of an f64 one.
 * on_device: 0 synchronous on host pointers; 1: cubes, var, psf, psf_index, shift and fit_out are device pointers (x
 * stays a host pointer; it is copied before the call returns) and the call is queued on the context stream; timed under
 * the fit's profiling id.
 * MPSFR_E_INVALID before anything is queued, with fit_out untouched: nstar < 1, npsf < 1 or nl outside
 * 1 .. MPSFR_MAX_SPEC_LAYERS; NULL cubes, psf or fit_out; unknown flag bits, MPSFR_FIT_ELLIPTICAL,
 * MPSFR_FIT_FIXED_SHIFT or MPSFR_FIT_COMMON_SHIFT; MPSFR_FIT_DRIFT with nl == 1, or with x NULL, not finite, outside
 * [-1, 1] or all equal; psf_index NULL with npsf != nstar; and, for host pointers, an index out of range or a start
 * that is not finite or outside the domain. */
#define MPSFR_FIT_DRIFT 16           /* beside MPSFR_FIT_BACKGROUND (1); ELLIPTICAL, FIXED_SHIFT, COMMON_SHIFT are refused here */
#define MPSFR_MAX_SPEC_LAYERS 4096
#define MPSFR_NFIT_SPEC 16           /* head of a star's row */
#define MPSFR_NFIT_SPEC_LAYER 10     /* per layer */
int mpsfr_fit_spectra_psf(mpsfr_ctx* ctx, int nstar, int nl, const double* cubes, const double* var, int npsf,
                          const double* psf, const int32_t* psf_index, const double* shift, const double* x,
                          int flags, double* fit_out, int on_device);

/* PSF energy metrics of caller-provided stamps: encircled and ensquared energy with exact pixel overlap, and the radii
 * that hold given fractions of the flux -- the non-parametric description of a core + halo PSF, beside the Moffat fits.
 * Pixel (p, q) is the unit square centred on (p, q), in the pixel coordinates of the fits (p0, q0).  Per stamp:
 *   flux     the sum of the stamp;  peak, peak_p, peak_q: the brightest pixel (the first in row-major order on a tie);
 *   centre   (cp, cq): centers[stamp] = (p, q) if `centers` is given, else the flux-weighted first moment of the stamp;
 *   EE_k     = sum_pq A(p, q; cp, cq, r_k) I_pq / flux, A the exact area of pixel (p, q) inside the circle of radius
 *            r_k about the centre (analytic circle-square overlap); a circle reaching beyond the stamp counts what is on
 *            the stamp;
 *   SQE_k    the same for the axis-aligned box of side s_k centred on the centre (overlap length in p times in q);
 *   R_k      a radius with |EE(R_k) - f_k| <= 1e-12 where the status is 0, found on the exact EE(r) between 0 and the
 *            distance to the farthest pixel corner (unique where the stamp is non-negative).
 * Arithmetic is fp64 in both precision modes: the call measures the stamp it is given.  A stamp's row depends on that
 * stamp and the parameters only (bit for bit), not on the batch.
 * stamps: [nstamp][dimpsf][dimpsf] float64; centers: [nstamp][2] or NULL; radii_px / boxes_px / fractions: nrad / nbox /
 * nfrac values, each count 0..MPSFR_MAX_METRIC_RADII, always host pointers;
 * out: [nstamp][MPSFR_NMET_HEAD + nrad + nbox + nfrac]:
 *   0 flux  1 peak  2 peak_p  3 peak_q  4 cp  5 cq  6 status  7 zero (reserved), then the nrad EE values, the nbox
 *   ensquared energies and the nfrac radii (pixels).
 * status: 0; 1: an EE radius did not reach 1e-12 (the value is the last iterate, finite and inside the search interval):
 * the fp64 sums of EE(r) cancel too much for the iteration to settle, on a stamp of mixed signs once sum |I| / flux
 * reaches ~1e4 (seen at 1e4, not at 1e2; not seen on a non-negative stamp);
 * 2: the stamp has a non-finite pixel or flux <= 0 (an all-zero stamp included), or the centre is not finite, or |cp|
 * or |cq| exceeds MPSFR_METRIC_CENTER_MAX pixels (the overlap area of a pixel is good to ~eps r^2, and a radius is
 * searched up to the centre's distance: farther out the 1e-12 of R_k could not be kept) -- every energy field is then
 * NaN (the centroid too); the other stamps of the call are not affected.
 * on_device as mpsfr_fit_stamps_elliptical: with 1, stamps, centers and out are device pointers and the call is queued
 * on the context stream (e.g. behind a device-output reconstruct).  Refused with MPSFR_E_INVALID before anything is
 * queued (out is not touched): a count outside 0..16 or all three zero, a radius or box side that is not finite and > 0
 * or exceeds 2 dimpsf pixels, a fraction outside (0, 1), nstamp < 1.  Timed under the fit's profiling id. */
#define MPSFR_MAX_METRIC_RADII 16      /* also the cap on boxes and on fractions */
#define MPSFR_NMET_HEAD 8
#define MPSFR_METRIC_CENTER_MAX 100.0  /* |cp|, |cq| of a centre, pixels */
int mpsfr_stamp_metrics(mpsfr_ctx* ctx, int nstamp, const double* stamps, const double* centers, int nrad,
                        const double* radii_px, int nbox, const double* boxes_px, int nfrac, const double* fractions,
                        double* out, int on_device);

/* Frame-level PSF photometry: stamps out of a frame, and the fitted models back into it -- frame -> cut_stamps -> the
 * PSF-model fits -> render_stars -> residual frame, every step on device buffers of one context if the caller wants.
 *
 * A frame is [ny][nx] float64, 1 <= ny, nx <= MPSFR_MAX_IMAGE_SIDE and ny nx <= 2^26.  origin[k] = (row, column) is the
 * frame pixel on which pixel [0][0] of star k's stamp lies: stamp pixel (p, q) is frame pixel (origin_p + p, origin_q + q).
 * Any int32 origin with |origin| <= 2^30 is legal, on or off the frame.  `shift` is the (dp, dq) of mpsfr_fit_stamps_psf
 * (|dp|, |dq| <= MPSFR_FIT_PSF_MAX_SHIFT) and `scale` its F: a frame cut with `origin`, fitted and rendered with the same
 * `origin` and the fit's (F, dp, dq) reproduces the fit's model (without b) on those pixels.
 *
 * mpsfr_cut_stamps: stamps_out[k][p][q] = image[origin_p + p][origin_q + q], bit for bit, where that pixel is on the
 * frame, NaN elsewhere; var_out likewise from var, 0 elsewhere (var and var_out: both NULL or both given).  NaN data and
 * var <= 0 are the pixel mask of the observed fits, so a star at the frame's edge is fitted on the pixels it has and a
 * stamp wholly off the frame makes the fits answer status 2.
 *
 * mpsfr_render_stars: for every frame pixel (Y, X), the stars taken in increasing index k,
 *   acc_0 = image_in[Y][X] (0 if image_in is NULL),  acc_k = acc_{k-1} +- t_k,  image_out[Y][X] = acc_nstar,
 *   t_k = scale_k P~_k(Y - origin_p,k - dp_k, X - origin_q,k - dq_k),
 * with - under MPSFR_RENDER_SUBTRACT (which requires image_in), else +.  P~ is the cubic-convolution resampling of
 * mpsfr_fit_stamps_psf of the model stamp psf[psf_index[k]] (psf[k] if psf_index is NULL, then npsf == nstar), zero
 * outside the model's pixels.  A star's term is applied only on its footprint, the (dimpsf + 20)^2 window around its
 * stamp (frame rows origin_p - 10 .. origin_p + dimpsf + 9); pixels no footprint reaches are copied unchanged, so a NaN
 * of one model stays inside that star's footprint.  Inside it values follow IEEE rules (a NaN pixel of image_in stays
 * NaN); the call does not inspect the model.  The product scale_k P~ is rounded before it is added.
 * The order of the sum is part of the contract: a pixel's value depends on image_in there and on the stars whose
 * footprint reaches it, in index order -- not on the tile grid, the batch or where the scene sits in the frame --, so
 * one call over the stars 0 .. n-1 equals, bit for bit, two calls over 0 .. m-1 and m .. n-1, the second reading the
 * first's output.  image_out may be image_in (in place); no other overlap is allowed.
 * Arithmetic is fp64 in both precision modes: the call measures the data it is given.
 * star_out (or NULL): [nstar][MPSFR_NRENDER]: 0 status, 1 the number of frame pixels inside the footprint, 2, 3 zero.
 * status 0: rendered (scale = 0 included); 1: the footprint misses the frame, nothing added; 2: skipped, nothing added
 * (count 0) -- in the device form a psf_index out of range, a shift that is not finite or outside the domain, a scale
 * that is not finite, an |origin| above 2^30; for host pointers these make the call return MPSFR_E_INVALID instead.
 * A tile's list of up to MPSFR_RENDER_SORT_CHUNK stars is sorted in LDS, a longer one in memory; the result is the same.
 *
 * on_device as mpsfr_fit_stamps_psf: 0 synchronous on host pointers; 1: every array is a device pointer and the call is
 * queued on the context stream behind the lanes.  MPSFR_E_INVALID, outputs untouched: ny or nx outside 1 ..
 * MPSFR_MAX_IMAGE_SIDE or ny nx > 2^26; nstar < 1 or npsf < 1; a NULL image, origin, psf, scale, stamps_out or
 * image_out; var and var_out not both NULL or both given; unknown flag bits; SUBTRACT without image_in; psf_index NULL
 * with npsf != nstar.  Both calls are timed under the fit's profiling id. */
#define MPSFR_RENDER_SUBTRACT 1
#define MPSFR_NRENDER 4            /* doubles per star in star_out */
#define MPSFR_MAX_IMAGE_SIDE 16384 /* and ny * nx <= 2^26 */
#define MPSFR_RENDER_SORT_CHUNK 256
int mpsfr_cut_stamps(mpsfr_ctx* ctx, int ny, int nx, const double* image, const double* var, int nstar,
                     const int32_t* origin, double* stamps_out, double* var_out, int on_device);
int mpsfr_render_stars(mpsfr_ctx* ctx, int ny, int nx, const double* image_in, int nstar, int npsf, const double* psf,
                       const int32_t* psf_index, const int32_t* origin, const double* shift, const double* scale,
                       int flags, double* image_out, double* star_out, int on_device);

/* The star finder: matched-filter detection on a frame -- the source of the positions the frame calls above take, and
 * the FIND of the loop find -> cut -> fit -> subtract -> find on the residual.
 *
 * image [ny][nx] and var (NULL or the same shape) are a frame as above.  psf is ONE model stamp [dimpsf][dimpsf]; the
 * filter K is its (2 half + 1)^2 core centred on stamp pixel (dimpsf/2, dimpsf/2), used as given, without any
 * normalisation, so that an amplitude is the `scale` F of mpsfr_fit_stamps_psf.  Arithmetic is fp64 in both precision
 * modes: a mixed context gives the bits of an f64 one.
 *
 * The pixel mask is that of the observed fits: a datum that is NaN or not finite, var <= 0 or not finite, a pixel off
 * the frame.  w = 1/var on a valid pixel (1 without var) and 0 on a masked one, whose datum counts as 0.
 * The map: for the frame pixel (Y, X), over its window in row-major tap order (rows outer, columns inner; the order is
 * part of the contract),
 *   S0 = sum w,  S1 = sum w K,  S2 = sum w K^2,  S3 = sum w D,  S4 = sum w K D,
 *   den = S2 - S1^2 / S0,   H = (S4 - S1 S3 / S0) / den,   b = (S3 - H S1) / S0:
 * H is the least-squares amplitude of the model on the window beside a free constant background b.  The statistic T is
 * H sqrt(den) with var (the significance H / sigma_H) and H without.  T is defined where the centre pixel is valid, more
 * than half of the window's pixels are valid and den > 0, and NaN elsewhere: a star at the frame's edge is found on the
 * pixels it has.  map_out (or NULL) receives T [ny][nx].
 * Peaks: pixel i = Y nx + X is a peak when T(i) >= threshold and every other pixel j with a finite T in the
 * (2 sep + 1)^2 square around it has T(j) < T(i), or T(j) == T(i) and j > i (on a plateau the first pixel wins).
 * Rows: the peaks in increasing pixel index.  count_out[0] is their number in the frame; if it exceeds max_stars the
 * first max_stars are written.  Rows and their order depend on the frame alone, not on the tile grid, the scheduling or
 * where the scene sits in the frame.  star_out [max_stars][MPSFR_NFIND]:
 *   0 Y + dy   1 X + dx   2 T at the peak pixel   3 H   4 b   5 sharpness   6 valid pixels in the window   7 flags
 * dy = clamp(0.5 (T- - T+) / (T- - 2 T0 + T+), +-0.5), the parabola through T along the row axis, dx along the column
 * axis; the offset is 0 and flag bit 0 (rows) or 1 (columns) is set when a neighbour is not finite or off the frame or
 * the curvature is not negative.  sharpness = (D0 - mD) / (H (K0 - mK)) with mD, mK the unweighted means of D and K over
 * the other valid pixels of the window: 1 for the model itself on any constant background, far above 1 for a hot pixel,
 * below 1 for something extended; NaN and flag bit 2 when there is no other valid pixel or the denominator is 0.
 * origin_out (or NULL) [max_stars][2]: (Y - dimpsf/2, X - dimpsf/2), the origin mpsfr_cut_stamps and mpsfr_render_stars
 * take; with it (dy, dx) is a legal start shift.
 * Rows from count_out[0] up to max_stars are NaN in all columns and have the origin (-2^30, -2^30): legal and off the
 * frame, so that cut_stamps makes an all-NaN stamp of it, the fits answer status 2 and render_stars skips it -- find ->
 * cut -> fit -> subtract run at the fixed size max_stars on device buffers without a host synchronisation between them.
 *
 * on_device as mpsfr_render_stars.  MPSFR_E_INVALID, outputs untouched, nothing queued: ny or nx out of range; a NULL
 * image, psf, star_out or count_out; half outside 1 .. MPSFR_FIND_MAX_HALF or above dimpsf/2; sep outside 1 ..
 * MPSFR_FIND_MAX_SEP; max_stars outside 1 .. 2^24; a threshold that is not finite; on host pointers a core with a value
 * that is not finite or with all values equal (in the device form such a core gives a map without peaks and
 * count_out[0] = 0).  Timed under the fit's profiling id. */
#define MPSFR_NFIND          8    /* doubles per star in star_out */
#define MPSFR_FIND_MAX_HALF  8
#define MPSFR_FIND_MAX_SEP   16
int mpsfr_find_stars(mpsfr_ctx* ctx, int ny, int nx, const double* image, const double* var, const double* psf,
                     int half, int sep, double threshold, int max_stars, double* star_out, int32_t* origin_out,
                     int32_t* count_out, double* map_out, int on_device);

/* Friends-of-friends groups of found stars (DAOPHOT's GROUP): the connected components of the relation "closer than
 * crit", as the tables mpsfr_cut_stamps, mpsfr_fit_stamps_psf and mpsfr_fit_groups_psf take as they are -- the step
 * between mpsfr_find_stars and the fits in a crowded frame.
 *
 * pos [nstar][stride] doubles, stride >= 2: columns 0 and 1 are (y, x) in frame pixels; the star_out of mpsfr_find_stars
 * is passed as it is with stride = MPSFR_NFIND.  A row with NaN in either coordinate is a filler (the finder's filler
 * rows are such rows): it belongs to no group and gets the label -1.  Any other row outside [-1, ny] x [-1, nx],
 * +-infinity included, makes the call return MPSFR_E_INVALID on host pointers; in the device form it is treated as a
 * filler with the label -2.
 * The link rule: stars i and j are linked when d2 <= c2, with dy = y_i - y_j, dx = x_i - x_j, d2 = dy dy + dx dx (each
 * product rounded, then the sum: no fused multiply-add) and c2 = crit crit rounded.  The relation is symmetric bit for
 * bit, and two stars at one position are linked.  A group is a connected component: a chain of any length is one group.
 * label_out [nstar]: the smallest star index of the star's group.
 * Groups come in five classes: 1, 2, 3, 4 members, then oversize (more than MPSFR_MAX_GROUP).  Rows are ordered by class
 * first and by label within a class.  count_out [6]: the number of groups, then the number in each class -- of the frame,
 * so they may exceed max_groups; then the first max_groups rows are written.  offset_k, the first row of class k, is the
 * sum of the class counts before it.
 * group_out [max_groups][MPSFR_NGROUP] int32:  0 members n   1 flags   2 label   3 zero   4..7 the member indices in
 * ascending order, -1 beyond n; of an oversize group the four smallest.
 * origin_out [max_groups][2] int32, for n <= 4: per axis, c = 0.5 (lo + hi) over the members' coordinates and
 * origin = (int)floor(c + 0.5) - dimpsf/2: the stamp is centred on the group's bounding box.
 * shift_out: member k of a group has, per axis, shift = pos_k - (double)(origin + dimpsf/2), one subtraction.  The buffer
 * is [max_groups][8] doubles, and the shifts of class k lie in it AT THE PITCH OF THEIR CLASS: row r of the class (row
 * offset_k + r of the tables), member m, axis a is shift_out[8 offset_k + 2 k r + 2 m + a].  So shift_out + 8 offset_k is
 * the [count_k][k][2] array mpsfr_fit_groups_psf takes with nsrc = k, and for k = 1 the [count_1][2] array
 * mpsfr_fit_stamps_psf takes, beside origin_out + 2 offset_k for mpsfr_cut_stamps -- no repacking.  Every other double
 * of the buffer is 0.  A row beyond max_groups is not written in this buffer either.
 * MPSFR_GROUP_WIDE is set when a member's |shift| exceeds MPSFR_FIT_PSF_MAX_SHIFT on an axis; the row is still written
 * (the fits refuse such a start).  An oversize group has MPSFR_GROUP_OVERSIZE, the origin (-2^30, -2^30) and no shifts:
 * the caller regroups its stars -- label_out says which they are -- with a smaller crit, as DAOPHOT does.
 * Rows from the number of groups up to max_groups are fillers: n = 0, flags 0, label 0, members -1, origin
 * (-2^30, -2^30), which mpsfr_cut_stamps turns into an all-NaN stamp.
 * Every output depends on the positions and crit alone -- not on the launch geometry, the cell grid, earlier calls or
 * the order in which workgroups run -- and is an integer or a single rounding.
 *
 * origin_out and shift_out: both or neither.  on_device as mpsfr_render_stars; in the device form reading count_out
 * back is the one host synchronisation of find -> group -> cut -> fit.  MPSFR_E_INVALID, outputs untouched, nothing
 * queued: ny or nx out of range; nstar outside 1 .. 2^24; stride < 2; crit not finite, <= 0 or above
 * MPSFR_GROUP_MAX_CRIT; max_groups < 1; a NULL pos, label_out, group_out or count_out; exactly one of origin_out and
 * shift_out; on host pointers a position out of range.  Timed under the fit's profiling id. */
#define MPSFR_GROUP_MAX_CRIT 16.0   /* pixels: 2 MPSFR_FIT_PSF_MAX_SHIFT, beyond it two stars cannot share a stamp */
#define MPSFR_NGROUP 8              /* int32 per group row */
#define MPSFR_GROUP_OVERSIZE 1      /* flag: more than MPSFR_MAX_GROUP members */
#define MPSFR_GROUP_WIDE 2          /* flag: a member's |shift| exceeds MPSFR_FIT_PSF_MAX_SHIFT */
int mpsfr_group_stars(mpsfr_ctx* ctx, int ny, int nx, int nstar, const double* pos, int stride, double crit,
                      int max_groups, int32_t* label_out, int32_t* group_out, int32_t* origin_out,
                      double* shift_out, int32_t* count_out, int on_device);

/* Crowded-field PSF photometry: the fluxes of ALL stars of a frame in one solve -- positions known (the finder's or a
 * catalogue's), PSF known, no limit on how many stars touch each other.  The step after mpsfr_group_stars for the
 * groups it flags MPSFR_GROUP_OVERSIZE or MPSFR_GROUP_WIDE.
 *
 * image, var, psf, psf_index, origin, shift: as for mpsfr_render_stars and mpsfr_cut_stamps.  Star k is F_k P~_k, P~_k the
 * cubic-convolution resampling of psf[psf_index[k]] placed by origin[k] and shifted by shift[k], zero outside its
 * footprint (the (dimpsf + 20)^2 window); its centre is c_k = (double)(origin_k + dimpsf/2) + shift_k per axis.
 * Arithmetic is fp64 in both precision modes.
 * A pixel is valid when its datum is finite and var is finite and > 0 (var NULL: unit weights); w = 1 / var.
 * The fit domain Omega: the valid pixels (Y, X) with dy dy + dx dx <= radius radius for an accepted star, dy = Y - c_y,
 * dx = X - c_x (each product rounded, then the sum: no fused multiply-add; radius radius rounded).  radius in [1, 20].
 * A star is accepted when index, shift and origin pass mpsfr_render_stars' per-star rule, its footprint meets the
 * frame, its own disc holds a valid pixel and sum w P~_k^2 over the valid pixels of its own disc is positive and finite
 * (so N_kk > 0: Omega only adds terms that are not negative).  Any other star is left out of the solve and of
 * resid_out: its row is status 2 (1: its footprint misses the frame) and zero otherwise.
 * Minimised over the F_k of the accepted stars and, with MPSFR_FIT_BACKGROUND, one constant b (a background that varies
 * over the frame is taken out beforehand with mpsfr_frame_background, whose applied_out is an image for this call):
 *     sum over Omega of w (D - b - sum_k F_k P~_k)^2;
 * a pixel of Omega sees every star whose footprint reaches it.  Solver: conjugate gradients on the normal equations
 * N u = A^T W D with the diagonal of N as preconditioner M, matrix-free; start F = scale0 (NULL: 0; a value that is not
 * finite counts as 0 in the device form), b = 0; stop when r.M^-1 r <= tol^2 (r0.M^-1 r0), when r0 = 0, or after
 * max_iter (1 .. 1000) steps; tol in (0, 1).  The loop is queued whole, without a host synchronisation: once the stop
 * test has passed the kernels of the remaining iterations return at once.
 *
 * star_out [nstar][MPSFR_NFRAMEFIT]:  0 F   1 err_F   2 flux = F sum P   3 err_flux = err_F |sum P|   4 overlap
 *     5 valid pixels in the star's own disc   6 N_kk = sum over Omega of w P~_k^2   7 status (0 fitted)
 *   err_F = sqrt((chi2 / dof) / N_kk), dof = |Omega| - unknowns: the CONDITIONAL error, every other star held fixed.
 *   overlap = sum_{l != k} N_kl / N_kk says when that is optimistic (0: the star is alone).  Marginal errors, the
 *   diagonal of N^-1, are not computed; groups of up to four stars get them from mpsfr_fit_groups_psf.
 * head_out [8]:  0 b   1 err_b = sqrt((chi2 / dof) / sum w)   2 chi2 of the result, from the residual frame itself
 *     3 |Omega|   4 iterations done   5 the last sqrt(r.M^-1 r / r0.M^-1 r0)   6 accepted stars
 *     7 status: 0 converged, 1 max_iter reached (the values are the last iterate), 2 nothing fitted -- no accepted star,
 *     or |Omega| < unknowns + 1; the star rows are then status 2 or 1 and resid_out is a copy of image.
 * resid_out [ny][nx] or NULL: image - sum_k F_k P~_k (b is not subtracted), made by the renderer: bit for bit what
 *   mpsfr_render_stars(MPSFR_RENDER_SUBTRACT) gives with the fitted scales over the accepted stars in index order.
 *
 * The same call gives the same bits, a mixed context those of an f64 one; no sum depends on scheduling.  A power of two
 * on var, or 2^k on the data (and scale0) with 4^k on var, scales F, b, the fluxes, the errors, chi2 and N_kk by exact
 * powers of two and changes no other bit.  Two accepted stars at one position are no error: N is singular, their sum
 * is determined, their split is not, and the call may end with status 1.
 * Work memory, in one buffer of the context: render's lists, two frames of doubles, and
 * 7 nstar + 4 ceil(ny nx / 4096) + 9 doubles and 2 nstar + 5 int32.
 * on_device as mpsfr_render_stars.  MPSFR_E_INVALID, outputs untouched, nothing queued: ny or nx out of range; nstar
 * outside 1 .. 2^20; npsf < 1; a NULL image, psf, origin, star_out or head_out; psf_index NULL with npsf != nstar;
 * radius, tol or max_iter out of range or not finite; flag bits other than MPSFR_FIT_BACKGROUND; on host pointers what
 * mpsfr_render_stars refuses (an index, shift or origin out of range, a scale0 that is not finite).  Timed under the
 * fit's profiling id. */
#define MPSFR_NFRAMEFIT 8                 /* doubles per star in star_out, and in head_out */
#define MPSFR_FRAME_FIT_MAX_RADIUS 20.0   /* pixels */
#define MPSFR_FRAME_FIT_MAX_ITER 1000
int mpsfr_fit_frame_psf(mpsfr_ctx* ctx, int ny, int nx, const double* image, const double* var, int nstar, int npsf,
                        const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                        const double* scale0, double radius, int flags, int max_iter, double tol, double* star_out,
                        double* head_out, double* resid_out, int on_device);

/* Crowded-field PSF photometry with free positions: mpsfr_fit_frame_psf with the shifts of the stars as unknowns beside
 * their fluxes -- the fluxes AND positions of all stars of a frame refined at once by Gauss-Newton, no limit on how
 * many stars touch each other (DAOPHOT's ALLSTAR step).
 *
 * image .. tol: as for mpsfr_fit_frame_psf.  The given shift is the start s0.  The valid pixels, the accepted stars and
 * Omega (the discs of `radius` around the START centres) are decided once, from s0, by mpsfr_fit_frame_psf's rules, and
 * stay for the whole call: Omega does not follow the stars.  Minimised over the F_k of the accepted stars, the shifts
 * s_k of the free stars and, with MPSFR_FIT_BACKGROUND, one constant b:
 *     sum over Omega of w (D - b - sum_k F_k P~_k(s_k))^2,      P~_k(s) placed by origin[k], which never moves.
 * 1. Opening solve: F and b at s0 from scale0, positions held.
 * 2. Up to max_outer Gauss-Newton steps.  A star is FREE in a step when it is accepted, its F from the solve before is
 *    finite and > 0, F > min_snr err_F, and its derivative columns have a positive finite norm; any other star is HELD
 *    in that step.  err_F = sqrt((chi2 / dof) / N_kk) is the conditional error of the solve before, taken where the step
 *    starts: chi2 of the residual of that F and b at the current shifts, N_kk at them, dof = |Omega| - accepted - [b].
 *    No star is free when |Omega| < 3 accepted + [b] + 1.  A free star has three columns at the current shifts, P~_k,
 *    dP~_k/ds_y and dP~_k/ds_x, the exact derivatives of the cubic-convolution taps; a held star has P~_k alone.  The
 *    linear least-squares problem in (F_k, a_k, c_k, b) over Omega is solved by Jacobi-preconditioned conjugate gradients
 *    on the normal equations, matrix-free, from the F and b before and a = c = 0.  Then delta_k = (a_k, c_k) / F_k with
 *    the new F_k (0 if that is not finite or not positive, or if the quotient is not finite); each axis is clipped to
 *    +- max_step, then so that |s_k - s0_k| <= max_move and |s_k| <= 8.  The loop ends when the largest unclipped
 *    |delta| over the free stars is <= pos_tol, or when no star is free.
 * 3. Closing solve: F and b at the final shifts, positions held, from the F and b before.  Columns 0-7, the head's
 *    first eight and resid_out belong to the returned shifts.
 * Every solve stops when r.M^-1 r <= tol^2 (g.M^-1 g), g = A^T W D over its live unknowns and M = diag(N) -- relative to
 * the right-hand side, so that a solve started at its solution ends at once --, when g = 0, or after max_iter steps.
 * Everything is queued whole, without a host synchronisation; behind a done word the queued kernels return at once.
 *
 * star_out [nstar][MPSFR_NFRAMEFREE]:  0-7 as mpsfr_fit_frame_psf, of the closing solve, with
 *     dof = |Omega| - accepted - 2 (stars ever free) - [b]
 *     8, 9 the final shift y, x   10, 11 their errors   12, 13 final minus start   14 flags   15 outer steps in which
 *     the star was free.
 *   The position errors are conditional on the other stars, as err_F is: the star's own 3 x 3 block of N (F, a, c) at
 *   its last free step, inverted, times chi2 / dof of the closing solve, over F^2 of the closing solve; 0 for a star
 *   that was never free.  Flags: MPSFR_FRAME_FREE_HELD held in the last outer step that ran; of the star's last free
 *   step, MPSFR_FRAME_FREE_BOUND resting on max_move or on the +-8 bound and MPSFR_FRAME_FREE_CLIPPED clipped by
 *   max_step.  A left-out star keeps its input shift in 8, 9, its status in 7, and zeros elsewhere.
 * shift_out [nstar][2], required: the final shifts, at the pitch mpsfr_render_stars and mpsfr_fit_frame_psf read.
 * head_out [MPSFR_NFRAMEFREE_HEAD]:  0-7 as mpsfr_fit_frame_psf, of the closing solve (5: the last
 *     sqrt(r.M^-1 r / g.M^-1 g))   8 outer steps done   9 the last largest |delta| over the free stars   10 free stars in
 *     the last step   11 inner iterations summed over all solves.
 *     7 status: 0 the position test AND the closing solve's stop test have passed (max_outer = 0, or no star free:
 *     the position test counts as passed); 1 anything else that was fitted; 2 nothing fitted.
 * resid_out [ny][nx] or NULL: bit for bit mpsfr_render_stars(MPSFR_RENDER_SUBTRACT) with shift_out and column 0 over
 *   the accepted stars.
 * max_outer in 0 .. 16 (0: the opening solve alone, reported as the closing one); pos_tol finite and > 0; max_step in
 * (0, 1]; max_move in (0, 4]; min_snr finite and >= 0.
 *
 * The same call gives the same bits, a mixed context those of an f64 one, host and device pointers the same; no
 * floating-point atomics, every sum in a fixed order.  mpsfr_fit_frame_psf's two power-of-two laws hold: they scale F,
 * b, the fluxes, their errors, chi2 and N_kk by exact powers of two, and every position, position error, flag and count
 * keeps its bits.
 * Work memory, in one buffer of the context: render's lists, two frames of doubles, and
 * 36 nstar + 8 ceil(ny nx / 4096) + 11 doubles and 6 nstar + 12 int32.
 * on_device as mpsfr_render_stars.  MPSFR_E_INVALID, outputs untouched, nothing queued: whatever mpsfr_fit_frame_psf
 * refuses; a NULL shift_out; max_outer, pos_tol, max_step, max_move or min_snr out of range or not finite.  The cube
 * form (one position from all layers, the layers side by side) is mpsfr_fit_cube_psf_free below.  Timed under the fit's
 * profiling id. */
#define MPSFR_NFRAMEFREE 16               /* doubles per star in star_out */
#define MPSFR_NFRAMEFREE_HEAD 12          /* doubles in head_out */
#define MPSFR_FRAME_FREE_MAX_OUTER 16
#define MPSFR_FRAME_FREE_MAX_STEP 1.0     /* pixels */
#define MPSFR_FRAME_FREE_MAX_MOVE 4.0     /* pixels */
#define MPSFR_FRAME_FREE_HELD 1           /* flag: held in the last outer step */
#define MPSFR_FRAME_FREE_BOUND 2          /* flag: resting on max_move or on the +-8 bound */
#define MPSFR_FRAME_FREE_CLIPPED 4        /* flag: the last step was clipped by max_step */
int mpsfr_fit_frame_psf_free(mpsfr_ctx* ctx, int ny, int nx, const double* image, const double* var, int nstar, int npsf,
                             const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                             const double* scale0, double radius, int flags, int max_iter, double tol, int max_outer,
                             double pos_tol, double max_step, double max_move, double min_snr, double* star_out,
                             double* shift_out, double* head_out, double* resid_out, int on_device);

/* Crowded-field photometry of a cube: the spectra of ALL stars, one solve of mpsfr_fit_frame_psf per wavelength layer,
 * the layers of a batch side by side in the same kernels -- positions shared by the layers, the PSF of each layer its own.
 *
 * cube [nl][ny][nx]; var of the same shape, or NULL.  psf [npsf][nl][40][40], the layout of mpsfr_fit_spectra_psf: star k
 * of layer l is psf[psf_index[k]][l].  origin, shift, psf_index: per star, for all layers, as for mpsfr_fit_frame_psf.
 * layer_shift [nl][2] or NULL: one offset per layer common to all stars (differential refraction).  The shift of star
 * k in layer l is shift[k] + layer_shift[l] per axis, one rounded addition (a NULL shift counts as 0); NULL: shift[k]
 * itself.  The footprint is placed by origin alone and does not move with the layer; the centre, the taps of the
 * resampling and the discs do.  scale0 [nl][nstar] or NULL.
 * star_out [nl][nstar][MPSFR_NFRAMEFIT], head_out [nl][8], resid_out [nl][ny][nx] or NULL: columns, statuses, acceptance
 * rule (per layer), Omega, stop rule (per layer), errors and on_device exactly as for mpsfr_fit_frame_psf.
 *
 * THE CONTRACT: layer l of the three outputs is bit for bit what mpsfr_fit_frame_psf returns on cube[l], var[l], the
 * contiguous copy of psf[:, l], shift + layer_shift[l], scale0[l] and the same radius, flags, max_iter and tol --
 * whatever layer_batch is, in both precision modes, on host and on device pointers.  In the device form a star whose
 * summed shift leaves the +-8 pixels in some layer is status 2 in that layer only.
 *
 * nl in 1 .. MPSFR_CUBE_FIT_MAX_LAYERS.  layer_batch >= 0: the layers solved side by side; values above nl count as nl;
 * 0: as many as MPSFR_CUBE_FIT_WORK_BYTES of per-layer work memory hold (at least one).  All max_iter iterations of a
 * batch are queued without a host synchronisation; every layer has its own done word, and once it is set the
 * workgroups of that layer return at once while the other layers of the batch go on.
 * Work memory, in one buffer of the context: render's lists once (built from the origins and indices alone, sorted once),
 * and per layer of a batch two frames of doubles, 7 nstar + 4 ceil(ny nx / 4096) + 9 doubles and 2 nstar + 5 int32.  The
 * host form stages the layers batch by batch: besides the per-star inputs and layer_shift, per layer of a batch one
 * frame for each of cube, var and resid_out that is given, npsf model stamps, and 9 nstar + 8 doubles (scale0, rows,
 * head); it waits for each batch before it refills the stage.
 * MPSFR_E_INVALID, outputs untouched, nothing queued: whatever mpsfr_fit_frame_psf refuses (cube in the place of image);
 * nl out of range; layer_batch < 0; on host pointers a layer_shift that is not finite or that takes the summed shift of
 * any star beyond 8 pixels, and a scale0 that is not finite.  Timed under the fit's profiling id. */
#define MPSFR_CUBE_FIT_MAX_LAYERS 4096
#define MPSFR_CUBE_FIT_WORK_BYTES ((size_t)256 << 20)   /* budget of per-layer work memory behind layer_batch = 0 */
int mpsfr_fit_cube_psf(mpsfr_ctx* ctx, int nl, int ny, int nx, const double* cube, const double* var, int nstar, int npsf,
                       const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                       const double* layer_shift, const double* scale0, double radius, int flags, int max_iter,
                       double tol, int layer_batch, double* star_out, double* head_out, double* resid_out,
                       int on_device);

/* Crowded-field photometry of a cube with free positions: ONE position per star from all layers jointly, each layer
 * with its own PSF and its own refraction offset -- mpsfr_fit_frame_psf_free's Gauss-Newton loop on the layers of
 * mpsfr_fit_cube_psf, all layers side by side in the same kernels.
 *
 * Inputs.  cube, var, psf, psf_index, origin, layer_shift, scale0, radius, flags, max_iter, tol: as for
 * mpsfr_fit_cube_psf.  shift: the start s0.  max_outer, pos_tol, max_step, max_move, min_snr: as for
 * mpsfr_fit_frame_psf_free, with the same ranges.  There is no layer_batch: all layers are solved together.
 *
 * Objective.  The shift of star k in layer l is s_k + layer_shift[l] per axis, one rounded addition, as for
 * mpsfr_fit_cube_psf.  Per layer, once, from s0, by mpsfr_fit_cube_psf's own judging: the valid pixels, accept[l][k]
 * and Omega_l (the discs around the START centres of layer l); they stay for the whole call.  A layer with fewer than
 * one accepted star, or with |Omega_l| < acc_l + [b] + 1, is DEAD: nothing of it is fitted, its head status is 2, and
 * the other layers are blind to it.  Minimised over the F_kl of the accepted stars, one s_k per free star and, with
 * MPSFR_FIT_BACKGROUND, one b_l per layer:
 *     sum_l sum over Omega_l of w_l (D_l - b_l - sum_k F_kl P~_kl(s_k + t_l))^2,          t_l = layer_shift[l].
 * 1. Opening solve: all F_kl, b_l at s0 from scale0, positions held.
 * 2. Up to max_outer joint Gauss-Newton steps.  Layer l CARRIES star k in a step when the star is accepted in l, F_kl
 *    from the solve before is finite and > 0, F_kl > min_snr err_F,kl with err_F,kl = sqrt(s2_l / N_kk,l) and
 *    s2_l = chi2_l / (|Omega_l| - acc_l - [b]), both at the current shifts from the opening pass of the step (as
 *    mpsfr_fit_frame_psf_free takes them per frame), and both derivative norms B_AA,kl, B_CC,kl are positive and
 *    finite.  Star k is FREE when at least one live layer carries it.  No star is free when
 *    sum over the live layers of |Omega_l| < sum over the live layers of (acc_l + [b]) + 2 A + 1, A the number of
 *    stars accepted in some live layer.  The linear problem has the unknowns (F_kl, b_l, delta_k); the column of
 *    delta_k,y is sum over the layers that carry k of F0_kl dP~_kl/ds_y, F0 the flux before the step, the exact
 *    derivatives of the cubic-convolution taps; the same for x.  It is solved by Jacobi-preconditioned conjugate
 *    gradients on the normal equations, matrix-free, from the F and b before and delta = 0, over ONE vector of
 *    nl (nstar + 1) + 2 nstar places (layer after layer its F and b, then delta_y, then delta_x) with a live mask.  The
 *    preconditioner of delta_k,y is sum_l F0_kl^2 B_AA,kl, summed in layer order.  Then delta_k is the solved value
 *    (0 if it is not finite); each axis is clipped to +- max_step, then to |s - s0| <= max_move, then so that
 *    |s_k + layer_shift[l]| <= 8 after rounding in EVERY layer of the call (the bound depends on layer_shift alone).
 *    The loop ends when the largest unclipped |delta| over the free stars is <= pos_tol, or when no star is free.
 * 3. Closing solve at the final shifts, positions held, from the F and b before.
 * Every solve stops when r.M^-1 r <= tol^2 (g.M^-1 g), g = A^T W D over all live unknowns of all layers and M = diag(N):
 * mpsfr_fit_frame_psf_free's rule on the joint vector, one done word per solve for all layers; a solve started at its
 * solution ends at once.  Everything is queued whole, without a host synchronisation.
 *
 * star_out [nl][nstar][MPSFR_NFRAMEFIT], head_out [nl][8]: mpsfr_fit_cube_psf's columns of the closing solve, with
 *     dof_l = |Omega_l| - acc_l - [b];  head 4 the closing solve's iteration count (the same in every layer), 5 the
 *     layer's own sqrt(r_l.M^-1 r_l / g_l.M^-1 g_l), 7: 2 for a dead layer, else the call's status.
 * pos_out [nstar][MPSFR_NCUBEFREE_POS]:  0, 1 the final shift   2, 3 its errors   4, 5 final minus start   6 flags
 *     (MPSFR_FRAME_FREE_HELD: free in no layer in the last outer step that ran; _BOUND, _CLIPPED of the last free step)
 *     7 outer steps in which the star was free.  A star accepted in no live layer keeps its input shift and zeros.
 *   The position errors are conditional on the other stars, as err_F is.  S_k = the sum over the layers that carried k
 *   in its last free step of (F_kl^2 / s2_l) times the 2 x 2 Schur complement of (a, c) over F in that layer's 3 x 3
 *   block of N of that step, F_kl and s2_l those of the closing solve, in layer order; the errors are the roots of the
 *   diagonal of S_k^-1, and 0 for a star that was never free or where that is not positive and finite.
 * shift_out [nstar][2], required: the final shifts, at the pitch mpsfr_fit_cube_psf and mpsfr_render_stars read.
 * call_out [MPSFR_NCUBEFREE_CALL]:  0 sum of chi2_l   1 sum of dof_l - 2 (stars ever free)   2 outer steps done
 *     3 the last largest |delta|   4 free stars in the last step   5 inner iterations summed over all solves
 *     6 status: 0 the position test AND the closing solve's stop test have passed, 1 anything else that was fitted,
 *     2 every layer dead   7 the last joint sqrt(r.M^-1 r / g.M^-1 g).
 * resid_out [nl][ny][nx] or NULL: layer l is bit for bit mpsfr_render_stars(MPSFR_RENDER_SUBTRACT) with
 *   shift_out + layer_shift[l] and column 0 of layer l over its accepted stars.
 *
 * The same call gives the same bits, a mixed context those of an f64 one, host and device pointers the same; no
 * floating-point atomics, every sum in a fixed order: star-index order in the walks, mpsfr_fit_frame_psf's tree in the
 * projections, layer order wherever layers are summed (the places of one layer are summed by one wave, lane j taking
 * the places j, j + 64, ..., then the wave's ladder; a joint scalar product is the sum over the layers plus the sum
 * over the delta places).  mpsfr_fit_frame_psf's two power-of-two laws hold on the whole cube: they scale the fluxes,
 * errors, chi2 and N_kk exactly, and every position, position error, flag and count keeps its bits.  At nl = 1 the
 * call agrees with mpsfr_fit_frame_psf_free within the bounds of the two solves, not in bits: there the unknowns are
 * a = F delta, here delta itself.
 * Work memory, in one buffer of the context, all layers resident: render's lists once; per layer two frames of
 * doubles, 25 nstar + 8 ceil(ny nx / 4096) + 17 doubles and 4 nstar + 5 int32; once 14 nstar + 10 doubles and
 * 5 nstar + 11 int32.  A call that needs more than MPSFR_CUBE_FREE_WORK_BYTES is refused (a budget, not a measured
 * value): positions come from a few dozen layers or bins, the spectra of a whole cube from mpsfr_fit_cube_psf at
 * shift_out.  The host form stages everything once and copies back.
 * MPSFR_E_INVALID, outputs untouched, nothing queued: whatever mpsfr_fit_cube_psf and mpsfr_fit_frame_psf_free refuse;
 * a NULL pos_out, shift_out or call_out; work memory above the budget.  MPSFR_E_NOMEM if the work memory cannot be
 * had.  Timed under the fit's profiling id. */
#define MPSFR_NCUBEFREE_POS 8             /* doubles per star in pos_out */
#define MPSFR_NCUBEFREE_CALL 8            /* doubles in call_out */
#define MPSFR_CUBE_FREE_WORK_BYTES ((size_t)4 << 30)    /* budget of work memory of one call */
int mpsfr_fit_cube_psf_free(mpsfr_ctx* ctx, int nl, int ny, int nx, const double* cube, const double* var, int nstar,
                            int npsf, const double* psf, const int32_t* psf_index, const int32_t* origin,
                            const double* shift, const double* layer_shift, const double* scale0, double radius,
                            int flags, int max_iter, double tol, int max_outer, double pos_tol, double max_step,
                            double max_move, double min_snr, double* star_out, double* head_out, double* pos_out,
                            double* shift_out, double* call_out, double* resid_out, int on_device);

/* The background map of a frame or cube: a robust mesh of clipped medians, a smooth full-resolution map of it and an rms
 * map (what SExtractor and photutils' Background2D build on the CPU), and optionally a second frame minus the map in the
 * same call, so that fit -> residual -> background of the residual -> subtract -> refit runs on device buffers without a
 * host synchronisation.
 *
 * image [nl][ny][nx], var the same shape or NULL, apply_to [nl][ny][nx] or NULL; a frame is nl = 1.  The frame rules of
 * mpsfr_render_stars apply, with nl ny nx <= 2^26 in total.  Arithmetic is fp64 in both precision modes: a mixed context
 * gives the bits of an f64 one.  A pixel is valid when its datum is finite and var, if given, is finite and > 0; var is
 * a mask only, the estimator is unweighted.  A valid zero counts as +0 (x + 0.0 at intake): no order statistic depends
 * on the sign of a zero.
 * Mesh: cells of side box (MPSFR_BACKGROUND_MIN_BOX .. MPSFR_BACKGROUND_MAX_BOX) from pixel (0, 0), my = ceil(ny / box),
 * mx = ceil(nx / box); edge cells are partial, npix is the number of a cell's pixels on the frame.
 * Cell estimate: med(v) of n values in ascending order is v[(n-1)/2] for odd n and 0.5 v[n/2-1] + 0.5 v[n/2] for even
 * n.  S_0 = the valid pixels of the cell, n_valid = |S_0|; the cell is valid iff n_valid >= 1 and (double)n_valid >=
 * min_frac (double)npix (one rounded product).  For pass p = 0, 1, ...: m = med(S_p); d_i = |x_i - m| (one rounded
 * subtraction); MAD = med(d); if p == max_clip the loop stops with MPSFR_BACK_CLIP_CAP, if MAD == 0 with MPSFR_BACK_FLAT
 * (both when both hold); else t = kc MAD with kc = kappa 1.4826 rounded once on the host, S_(p+1) = {i in S_p : d_i <=
 * t}, and the loop stops if nothing was rejected.  kappa >= 1 keeps S non-empty.  raw level = m, raw rms = 1.4826 MAD
 * (one rounded product), n_used = |S_last|, passes = p.  Every quantity is an order statistic, an integer or a single
 * rounding: the raw columns have no rounding freedom.
 * Filter and fill: filter in {1, 3, 5}, h = (filter - 1) / 2.  For cell (i, j), W_r is the set of VALID cells in rows
 * i-r .. i+r and columns j-r .. j+r inside the mesh; r starts at h and grows by 1 while W_r is empty and r < max(my,
 * mx).  level = med of the raw levels over W_r, rms = med of the raw rms over W_r, taken separately.  A cell that is
 * itself invalid has MPSFR_BACK_FILLED.  A layer without any valid cell has head status 2, level and rms NaN in every
 * cell and NaN maps.
 * mesh_out [nl][my][mx][MPSFR_NBACK]:
 *   0 level   1 rms   2 raw level   3 raw rms (both NaN for an invalid cell)   4 n_used (0 for an invalid cell)
 *   5 n_valid   6 passes   7 flags
 * head_out [nl][MPSFR_NBACK_HEAD]: 0 status (0 fine, 1 some cells filled, 2 no valid cell)  1 valid cells  2 filled cells
 *   3 zero
 * map_out (or NULL) [nl][ny][nx]: the cubic-convolution interpolation of the level plane with the Keys polynomials of
 * mpsfr_fit_stamps_psf.  Node i of an axis sits at pixel (i + 0.5) box - 0.5.  For pixel Y: u = ((double)Y + 0.5) /
 * (double)box - 0.5, i0 = floor(u), t = u - i0; the taps i0-1 .. i0+2 carry the Keys weights c(t+1), c(t), c(t-1),
 * c(t-2).  Beyond the mesh the plane continues linearly: E[-j] = M[0] + j (M[0] - M[1]) and E[m-1+j] = M[m-1] +
 * j (M[m-1] - M[m-2]) for j = 1, 2 (every tap is M[0] on an axis of one cell), columns first, then rows.  The sum is
 * separable: columns inner, rows outer, both ascending.  A plane on the nodes is reproduced over the whole frame up to
 * rounding; replicated edge nodes would flatten gradients in the outer half cell.
 * rms_out (or NULL): the same interpolation of the rms plane, values below 0 replaced by 0.  applied_out = apply_to -
 * map, one rounded subtraction (a NaN of apply_to stays NaN); apply_to and applied_out are given together or both NULL,
 * they may be the same buffer, and applied_out may not be image.
 *
 * Layer l of every output equals the call on layer l alone, bit for bit.  The same call repeated, host and device
 * pointers, mixed and f64 contexts, optional outputs given or NULL (the other outputs do not change) give the same bits.
 * A permutation of the pixels inside a cell changes no bit of columns 2 - 7 of that cell.  Negating the data negates the
 * levels exactly and keeps every other column; a factor 2^k on the data scales levels and rms exactly, away from
 * subnormals.  No floating-point atomics are used.
 *
 * on_device as mpsfr_render_stars: queued on the context stream behind the lanes, no host synchronisation.
 * MPSFR_E_INVALID, outputs untouched, nothing queued: nl < 1 or the size out of range; box outside 8 .. 64; filter not 1,
 * 3 or 5; kappa not finite or outside [1, 100]; max_clip outside 0 .. MPSFR_BACKGROUND_MAX_CLIP; min_frac not finite or
 * outside (0, 1]; a NULL image, mesh_out or head_out; exactly one of apply_to and applied_out; applied_out == image.
 * Timed under the fit's profiling id. */
#define MPSFR_NBACK 8                  /* doubles per mesh cell */
#define MPSFR_NBACK_HEAD 4             /* doubles per layer in head_out */
#define MPSFR_BACKGROUND_MIN_BOX 8
#define MPSFR_BACKGROUND_MAX_BOX 64
#define MPSFR_BACKGROUND_MAX_CLIP 16
#define MPSFR_BACK_FILLED 1            /* cell invalid: level and rms come from neighbours */
#define MPSFR_BACK_CLIP_CAP 2          /* the clipping ended at max_clip */
#define MPSFR_BACK_FLAT 4              /* MAD == 0 at the last pass */
int mpsfr_frame_background(mpsfr_ctx* ctx, int nl, int ny, int nx, const double* image, const double* var,
                           int box, int filter, double kappa, int max_clip, double min_frac,
                           const double* apply_to, double* mesh_out, double* head_out, double* map_out,
                           double* rms_out, double* applied_out, int on_device);

/* The stages of the path as the reference exports them (muse_psfr/__init__.py:16: `from .psfrec import *`),
 * for a caller that holds its own PSD or its own stamps.  Host buffers, synchronous, float64; the same
 * kernels as mpsfr_reconstruct entered or left at another stage.
 *
 * mpsfr_simul_psd      simul_psd_wfm (psfrec.py:36-151) for one (seeing, GL, L0): psd_out [npsflin^2][dim][dim],
 *                      centred (DC at [dim/2][dim/2]) and in the reference's units (times (0.5 1000 / 2 pi)^2,
 *                      psfrec.py:151).  Arguments as for mpsfr_reconstruct.
 * mpsfr_psf_from_psd   psf_muse (psfrec.py:644-686): psd [ndir][dim][dim] as above -- ANY real image, not only
 *                      the model's: every row is transformed -- to psf_out [nl][dimpsf][dimpsf], the stamps
 *                      BEFORE the convolutions (mean over the ndir directions, normalised to sum 1).  A PSD with
 *                      a NaN or an infinity is refused (MPSFR_E_INVALID) before anything is queued; a finite PSD
 *                      so large that its transform overflows gives non-finite stamps, and leaves no trace in the
 *                      calls after it.  (mpsfr_psd_to_psf below does NOT look at its PSDs: a PSD with a NaN is
 *                      accepted, return code 0, and every pixel of every plane of that PSD comes back NaN -- the
 *                      NaN goes through both passes of the structure function's transform; the other PSDs of the
 *                      same call are computed as ever, and nothing of it is left in the calls after it.)
 * mpsfr_convolve_stamps  convolve_final_psf (psfrec.py:874-930): psf_in [ntask][nl][dimpsf][dimpsf] convolved
 *                      with each task's tip-tilt Moffat kernel and the instrument's, into psf_out. */
int mpsfr_simul_psd(mpsfr_ctx* ctx, double seeing, double gl, double l0, int three_lgs, const double h[2],
                    double wind_speed, int npsflin, const uint8_t* mask_rec, const uint8_t* mask_res,
                    double* psd_out);
int mpsfr_psf_from_psd(mpsfr_ctx* ctx, int ndir, const double* psd, int nl, const double* lbda_nm,
                       double* psf_out);
int mpsfr_convolve_stamps(mpsfr_ctx* ctx, int ntask, const double* seeing, const double* gl, const double* l0,
                          int nl, const double* lbda_nm, const double* psf_in, double* psf_out);

/* psd_to_psf (psfrec.py:689-807): the full dimnum x dimnum PSF of any PSD, any pupil and an optional static
 * phase, for FoV == FoVnum and samp <= dim / npup (the reference's other branches are not supported).
 *   psd           [npsd][dim][dim] float64, centred (DC at [dim/2][dim/2]), nm^2 m^2 at the PSF wavelength;
 *                 dim is the context's grid.  Not checked for NaN: see mpsfr_psf_from_psd above
 *   pup           [npup][npup] float64, any real values (apodised, spiders, gaps); sum(pup) != 0
 *   phase_static  [npup][npup] or NULL.  The field is pup exp(2 pi i phase_static / lbda_m) as psfrec.py:785-786
 *                 computes it: phase_static is in METRES (the reference's docstring says nm; its code divides
 *                 by the wavelength in metres, and this follows the code)
 *   D             pupil diameter [m]; L = D dim / npup (psfrec.py:710-711)
 *   lbda_m        [nl] wavelengths in metres, as the reference's `lbda`
 *   dimnum        output side: 128, 256, 512, 1024 or 1280, <= dim and >= npup (psfrec.py:731:
 *                 int(fix(dim samp / sampnum / 2)) 2)
 *   psf_out       [npsd][nl][dimnum][dimnum] float64, centred, each plane normalised to sum 1
 *   on_device     0: host buffer; 1: device pointer on the context's device.  The call is synchronous either way.
 * Everything is computed in fp64 whatever the context's precision.  The call uses a stream and workspaces of its
 * own (bounded: the wavelengths go in chunks), so asynchronous mpsfr_reconstruct calls in flight are unaffected.
 * Every plane is computed independently: a batched call equals the same planes called one at a time, bit for bit. */
int mpsfr_psd_to_psf(mpsfr_ctx* ctx, int npsd, const double* psd, int npup, const double* pup,
                     const double* phase_static, double D, int nl, const double* lbda_m, int dimnum,
                     double* psf_out, int on_device);

/* FIT_ROWS assembly on the host (pure C, no GPU): the columns fit_psf_cube keeps from the fit object
 * (psfrec.py:866-870) -- center[2], flux, fwhm[2] (arcsec), n, peak, err_center[2], err_flux, err_fwhm[2] (arcsec),
 * err_n, err_peak: 14 doubles -- of `n` fit rows ([n][MPSFR_NFIT], as mpsfr_reconstruct writes them) into
 * out[r * stride + 0..13].  `stride` (in doubles, >= 14) lets the caller write straight into the records of a
 * table that carries further columns (compute_psf_from_sparta's FIT_ROWS: lbda in front, SEEING, GL, L0, row_idx,
 * lgs_idx behind, psfrec.py:1086-1101).  err_flux: the relative errors of peak, alpha^2 and (n - 1) in quadrature. */
int mpsfr_fit_rows(const double* fit, long n, double pixscale, double* out, long stride);

/* Block until every call made so far has finished (and hand over the results of every
 * asynchronous host-output call). */
int mpsfr_sync(mpsfr_ctx* ctx);

/* Asynchronous host outputs (on_device = 2).  mpsfr_last_ticket: the ticket (0, 1, 2, ...) of the most
 * recent such call of the context, -1 before the first.  mpsfr_wait: block until the call with that
 * ticket has finished and copy its results (and those of every earlier ticket not yet handed over)
 * into the arrays it was given.  This is how the rows of a table larger than one call are kept in
 * flight (the reference: Parallel(...)(delayed(compute_psf) ...), psfrec.py:1082-1083, results
 * collected at :1086-1113). */
long mpsfr_last_ticket(mpsfr_ctx* ctx);
int mpsfr_wait(mpsfr_ctx* ctx, long ticket);

/* Give up every asynchronous host-output call that has not been handed over yet: wait for the GPU to
 * drain, then forget the callers' arrays WITHOUT writing to them.  The error path of a caller whose output
 * arrays are about to go away (an exception between the call and its mpsfr_wait): after this, no later
 * mpsfr_wait / mpsfr_sync / mpsfr_reconstruct of the context touches those arrays.  The abandoned tickets
 * count as completed; the context stays usable. */
int mpsfr_abandon(mpsfr_ctx* ctx);

/* The context's hipStream_t (as void*): it is ordered after every asynchronous (on_device = 1)
 * call made so far, so a caller can queue its own GPU work behind the results without a host
 * sync, e.g. torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(...)). */
void* mpsfr_stream(mpsfr_ctx* ctx);

/* Make `caller_stream` (a hipStream_t of the caller, as void*) wait, on the GPU, for every asynchronous call made so far
 * on this context: the cheap form of "wait on mpsfr_stream()" -- the call's work stays on its lane and one event at the
 * lane's end is all that is queued (asking for mpsfr_stream() makes every later call join its lanes into a further
 * queue).  E.g. before a collective that reads the call's device outputs:
 *   mpsfr_stream_wait(ctx, (void*)torch.cuda.current_stream().cuda_stream). */
int mpsfr_stream_wait(mpsfr_ctx* ctx, void* caller_stream);

/* Make the next mpsfr_reconstruct wait (on the GPU, no host sync) for `hip_event`, a recorded
 * hipEvent_t of the caller, e.g. the end of a collective that still reads the buffers the call
 * will overwrite.  One-shot: consumed by the next call. */
int mpsfr_wait_event(mpsfr_ctx* ctx, void* hip_event);

/* Host wall time spent inside mpsfr_reconstruct since the last mpsfr_profile_reset, and the
 * number of calls: what queueing a call costs the host thread.  Time spent blocked because the
 * host ran four calls ahead of the GPU (the ring of parameter blobs) is not counted. */
int mpsfr_host_time(mpsfr_ctx* ctx, double* seconds, long* calls);

/* Copy an intermediate of the most recent mpsfr_reconstruct pipeline pass (last chunk) to the
 * host as float64 (parity tests, tests/test_gpu_parity.py).  `what`:
 *   "ao_tables"  [2 geometries][ndir][3 (T0,T1,noise)][80][80]   (psfrec.py:531-613); after a profile call
 *                [2][ndir][max(nlayer, 2) + 1 (layer tables, noise)][80][80] (mpsfr_reconstruct_profile)
 *   "tel"        [dim/2+1][dim]  telescope OTF, transposed half plane (psfrec.py:784-790)
 *   "dphi0"      [chunk tasks][ndir][dim/2+1][dim] structure function / lambda-factor,
 *                transposed half plane (psfrec.py:717-722)
 *   "dlin"       [chunk tasks][ndir][dim/2+1][dim/32] line minima of the series form of stage A (option
 *                "prune_eps" > 0): the minimum of max("dphi0", 0) over each block of 32 columns of a line, as
 *                float (f64 mode: rounded down); >= 3e38 where the whole block lies outside the support of the
 *                telescope OTF (option "support_skip")
 *   "pre"        [chunk tasks][nl][dimpsf][dimpsf] stamps before the convolutions (psfrec.py:685)
 *   "vkeep"      [chunk tasks][(nl+1)/2] lines of the half plane transformed per wavelength pair
 *                (option "prune_eps")
 *   "mf_work"    [7] (the first 3 / 5 if capacity < 5 / 7) matrix-core stage, last chunk: tile steps executed,
 *                m-tiles with a second pass, tile steps without pruning, tile steps with all three
 *                products, tile steps without the low half of the OTF, blocks kept by at least one
 *                wavelength summed over the tasks, blocks inside the support of the telescope OTF x tasks
 * The work plan of the per-wavelength stage in the last chunk, as its kernels read it (tests/test_gpu_mf_plan.py;
 * tc = chunk tasks x stamp groups per task, nks = dim/32, nmt = ceil((dim/2+1)/16), nsw = ceil(nmt/8); a mask word
 * holds bit ks of its m-tile or sweep -- at most 40 bits, which a double carries exactly).  Each name fails with a
 * message when the last call did not produce that buffer; none launches anything or changes a buffer:
 *   "mf_par"     [9 + nl] the host's thresholds thr_eps, thr_floor, thr_mid, tier_half, thr_blk, thr_sum, c2min (floats),
 *                then per, ngr (wavelengths per group, groups) and c = -1/2 (2 pi / lambda)^2 of every wavelength
 *   "mf_own"     [tc][nl][nmt][2] thin-wave kernel: the full blocks (word 0) and mid blocks (word 1) of a wavelength
 *   "mf_uni"     [tc][ngr][nmt] the blocks a wavelength group stages
 *   "mf_ksum"    [tc][nl][nsw] the k-steps with work per sweep of eight m-tiles, of a wavelength
 *   "mf_kuni"    [tc][ngr][nsw] the same of a wavelength group
 *   "mf_gsw"     [tc][ngr] bit sw: the sweep has work
 *   "mf_sched"   [64] the lengths of the work lists, by work class
 *   "mf_items"   [sum of "mf_sched"][5] the filled part of every list: class, task, group, sweep, sweeps of the (task, group)
 *   "tlb"        [nmt][nks] log2 of the largest telescope OTF element of a block (-inf outside the support)
 *   "dminb"      [tc][nmt][nks] block minima of max("dphi0", 0) over the directions, as the matrix-core kernels prune on
 *                them (not when the thin-wave kernel took the line minima "dlin" instead)
 *   "dblk"       [chunk tasks][ndir][nmt][nks] the block minima per direction (same condition)
 *   "dline"      [chunk tasks][ndir][dim/2+1] the line minima per direction (same condition)
 *   "thrf"       [tc] log2 floor per task of the kernel for several directions (finite "tier_eps" > 0)
 *   "order"      [tc] dispatch order of the tasks (blocked matrix-core kernel, "prune_eps" > 0)
 *   "d0t_clears" [1] times a call cleared a lane's "dphi0" buffer because of what an earlier call left there
 *                (option "support_skip"), since the context was created
 * Returns the number of doubles written (<= capacity) or a negative error. */
long mpsfr_debug_fetch(mpsfr_ctx* ctx, const char* what, double* out, size_t capacity);

/* Per-kernel timing with HIP events recorded on the context's stream (option "profile" = 1). */
int mpsfr_profile_count(void);
const char* mpsfr_profile_name(int kernel_id);
int mpsfr_profile_get(mpsfr_ctx* ctx, int kernel_id, double* total_ms, long* launches);
int mpsfr_profile_reset(mpsfr_ctx* ctx);

/* Number of HIP devices visible to the process (0 if there is none or the runtime fails): what the
 * drop-in Python layer fans a large SPARTA table out over, one context and one host thread per
 * device -- the reference's joblib fan-out over worker processes (psfrec.py:1082-1083). */
int mpsfr_device_count(void);

/* Library/ABI version (major*100 + minor). */
int mpsfr_version(void);

/* Hash of the sources, headers and compiler flags this binary was built from (written by
 * muse_psfr_amd/_build.py; "unstamped" for a hand build).  bench.py records it. */
const char* mpsfr_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* MPSFR_H */
