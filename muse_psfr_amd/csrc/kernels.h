// Launchers for the HIP kernels of the PSF-reconstruction hot path (implemented in stage_a.hip,
// per_lambda.hip and stamps.hip; the fits of caller-provided stamps in fit_ell.hip, fit_obs.hip, fit_psf.hip,
// fit_group*.hip and fit_spec.hip: the last three fit a resampled model stamp -- flux scale, sub-pixel shift,
// background -- to an observed star, a blended group or a star cube; the frame calls in render.hip, find.hip,
// group.hip, frame_fit.hip and cube_fit.hip, which share frame_common.h).
// Host code (mpsfr_api.cpp) sees only these plain functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpsfr {

constexpr int NS = 40;       // dimpsf, psfrec.py:658
constexpr int NSH = NS / 2 + 1;  // samples 0..20 of a line; sample 40-i is the conjugate of i
constexpr int KS = 41;       // Moffat kernel side, psfrec.py:911-916
constexpr int NAO = 80;      // AO-corrected zone, psfrec.py:103, 138
constexpr int kNH = NAO / 2 + 1;   // values per line of the patch row transforms: the Hermitian half su = 0 .. 40 (stage_a2.hip)
constexpr int NFIT = 16;
constexpr int NFIT_ELL = 24;     // elliptical fit (fit_ell.hip)
constexpr int NFIT_PSF = 16;     // PSF-model fit (fit_psf.hip)
constexpr int NFIT_GROUP = 48;   // PSF-model fit of a blended group (fit_group.hip)
constexpr int METRIC_MAX = 16;   // MPSFR_MAX_METRIC_RADII: radii, boxes, fractions of one metrics call (metrics.hip)
constexpr int METRIC_HEAD = 8;   // MPSFR_NMET_HEAD
constexpr int KHAT = 33 * 64;  // complex entries of one kernel spectrum (k_khat)
constexpr int MAXLGS = 4;

// per-task scalars of the PSD model
struct TaskPar {
    double r0m53;     // r0^(-5/3), r0 at 0.5 um (psfrec.py:108, 183-187)
    double inv_l0sq;  // (1/L0)^2
    double cn2_0;     // normalised Cn2 of the ground layer (psfrec.py:57-58)
    double cn2_1;
    int geom;         // 0 = 4 LGS, 1 = 3 LGS (psfrec.py:86-91)
    int basis;        // 0: a task.  k + 1: "basis task" k of the series form of stage A (stage_a2.hip):
                      // PSD = r0m53 cfit (f^2 + inv_l0sq)^(-11/6 - k) [f >= fc], no corrected zone
};

// per-wavelength scalars
struct LamPar {
    double c;         // -0.5 * (2 pi / lambda_nm)^2   (psfrec.py:717, 793)
    int npixc;        // psfrec.py:663-664
    int pad;
};

struct AoGeom {
    double h[2];            // layer altitudes [m]
    double wind[2][2];      // wind[xy][layer] m/s  (psfrec.py:594)
    int nlgs[2];            // per geometry
    double poslgs[2][2][MAXLGS];  // [geom][xy][lgs] arcmin (psfrec.py:536)
    int ndir;
    double dir[2][25];      // [xy][dir] arcmin
};

// A Cn2 profile (mpsfr_reconstruct_profile): the layers that take the place of AoGeom::h / wind.  The tables of
// the AO zone are linear in the layer weights, PSD_AO = VK sum_l w_l T_l + noise, so a profile call builds one
// table per layer ([geom][dir][ntab + 1][80][80], ntab = max(n, 2): a single layer gets a second, zero table and
// weight, so that the mixing sum always starts as the legacy two-layer one) and every row mixes them with its own
// weights ([ntask][ntab], normalised to sum 1).
constexpr int MAXLAYER = 8;
struct AoLayers {
    int n;                         // layers, 1..MAXLAYER
    int ntab;                      // max(n, 2)
    double h[MAXLAYER];            // altitudes [m]
    double wind[2][MAXLAYER];      // wind[xy][layer] m/s
};
inline int ao_ntab(int nlayer) { return nlayer < 2 ? 2 : nlayer; }
// the per-row weights a profile call hands to the kernels of stage A: d_w [task][ntab] (relative to the tasks the
// launch sees); w = nullptr: a legacy call (TaskPar::cn2_0 / cn2_1, two layer tables)
struct LayerMix {
    const double* w = nullptr;
    int ntab = 2;
};

// work lists of the thin-wave matrix-core kernel: one per work class (a lane of the consumer's wave keeps the
// bounds of one list), then the queue head
constexpr int kMfLists = 64;
constexpr int kMfSchedInts = kMfLists + 1;

enum KernelId {
    K_AO_TABLES = 0,
    K_TEL_OTF,
    K_PSD_ROWFFT,
    K_COLFFT_DPHI,
    K_GTABLE,
    K_MOFFAT_KERNELS,
    K_OTF_ROWFFT,
    K_COLPASS,
    K_CONV,
    K_FIT,
    K_STAMP_SUM,
    K_VKEEP,        // FFT path: K_DMIN + K_VKEEP
    K_OTF_MFMA,     // matrix-core per-wavelength stage (K_OTF_MFMA2 + K_MF_FINISH, or K_OTF_MFMA1)
    K_MF_PREP,      // its preparation: K_DMIN + K_MF_PREP (or K_DMIN + K_VKEEP + K_TASK_ORDER)
    K_PATCH,        // series form of stage A (stage_a2.hip): K_PATCH_GEN + K_PATCH_ROWS
    K_DPHI_SERIES,  //   and K_DPHI_SERIES
    K_COUNT
};

void launch_ao_tables(hipStream_t s, const AoGeom& g, const uint8_t* d_mask_rec,
                      const uint8_t* d_mask_res, double* d_tab);
// profile tables [2][ndir][ly.ntab + 1][80][80] (layers beyond ly.n are zero)
void launch_ao_tables_profile(hipStream_t s, const AoGeom& g, const AoLayers& ly, const uint8_t* d_mask_rec,
                              const uint8_t* d_mask_res, double* d_tab);
void launch_tel_otf(hipStream_t s, int N, const uint64_t* d_rows, int words, double pupsum,
                    void* d_tel, bool f64out);
// d_dcpart: [ntd][psd_rowfft_groups(N)] the workgroups' shares of the PSD sum (bg[0,0], psfrec.py:721),
// added by launch_colfft_dphi; f64: the f64 mode (two Newton steps in x^(-11/6) instead of one)
int psd_rowfft_groups(int N);
void launch_psd_rowfft(hipStream_t s, int N, int ntd, int ndir, const TaskPar* d_tp,
                       const double* d_aotab, double cfit, void* d_C, const void* d_tw64,
                       double* d_dcpart, bool f64, const LayerMix& mix = LayerMix());
// d_zero: kMfSchedInts ints the kernel sets to zero (the work-list counters of launch_mf_prep), or nullptr
void launch_colfft_dphi(hipStream_t s, int N, int ntd, const void* d_C, const double* d_dcpart,
                        double scale2, void* d_D0t, bool f64out, const void* d_tw64,
                        int* d_zero = nullptr);
// Pruning of the per-wavelength stage (stage_a.hip, "Line pruning"): minima of D per line
// ([ntd][N/2+1]) and per block of 16 lines x 32 columns ([ntd][nmt][N/32]), then the lines to keep
// per (task, wavelength pair) and the block minima over the directions
// (f64: D / the telescope OTF are double; the minima are rounded down, the maxima up)
void launch_dmin(hipStream_t s, int N, int ntd, const void* d_D0t, float* d_dline, float* d_dblk,
                 bool f64 = false);
// Stage-level entry points (stage_a.hip): the PSD of one task as an image [ndir][N][N] (centred, in the
// reference's units: `unit` = (lambda_ref 1000 / 2 pi)^2), and the structure function of an arbitrary
// PSD image: d_Cm [ndir][N][N/2+1] complex workspace, scale = 2 / L^2 for a PSD in the reference's units.
void launch_psd_image(hipStream_t s, int N, int ndir, const TaskPar& p, const double* d_aotab, double cfit,
                      double unit, double* d_psd, const LayerMix& mix = LayerMix());
void launch_dphi_from_psd(hipStream_t s, int N, int ndir, const double* d_psd, void* d_Cm, double scale,
                          void* d_D0t, bool f64out, const void* d_tw64);
// psd_to_psf (psd_to_psf.hip), fp64, M = dimnum (a planned length), d_twm: exp(-2 pi i m / M).
// launch_p2p_otf: nz telescope OTFs of the pupil d_pup [P][P] (times exp(2 pi i d_phase / lambda_m[z]) when
// d_phase is not NULL) into d_otft [nz][M/2+1][M] (scaled by `scale`); d_T1 [nz][P][M] and d_Q [nz][M][M/2+1]
// complex workspaces.  launch_p2p_psf: nz planes d_psf [nz][M][M] (centred, sum 1) from the structure function
// d_D0t [N/2+1][N] (launch_dphi_from_psd), the OTFs (plane z at d_otft + z otf_stride) and d_cl[z] =
// -(2 pi / lambda_nm)^2 / 2; d_G [nz][M/2+1][M/2+1] complex workspace.
bool p2p_supported(int M);
void launch_p2p_otf(hipStream_t s, int M, int P, int nz, const double* d_pup, const double* d_phase,
                    const double* d_lbda_m, double scale, void* d_T1, void* d_Q, double* d_otft, const void* d_twm);
void launch_p2p_psf(hipStream_t s, int M, int N, int nz, const double* d_D0t, const double* d_otft, size_t otf_stride,
                    const double* d_cl, void* d_G, double* d_psf, const void* d_twm);
// Series form of stage A (stage_a2.hip).  d_coef: [N/2+1][N][series_terms] structure functions of the
// terms of the expansion of the fitting PSD in 1/L0^2 about series_eps0() (launch_series_coef from the
// fp64 planes [terms][N/2+1][N] that launch_colfft_dphi produced for the basis tasks);
// launch_patch: d_P [ntd][80][80], d_T [ntd][N/2+1][41] complex (kNH: the Hermitian half of a line), d_sp [ntd];
// launch_dphi_series: D0t as launch_colfft_dphi writes it.  Valid for 1/L0^2 <= series_eps_max().
// d_twk: the per-lane twiddle table of launch_series_twiddles (series_twiddle_bytes), which takes the
// place of d_tw64 in launch_patch / launch_dphi_series
size_t series_twiddle_bytes(int N);
void launch_series_twiddles(hipStream_t s, int N, const void* d_tw64, void* d_twk);
int series_terms(bool f64);
double series_eps0();
inline double series_eps_max() { return 1.0 / 49.0; }
void launch_series_coef(hipStream_t s, int N, const double* d_planes, void* d_coef, bool f64);
// The spectra of `n` tip-tilt Moffat kernels (launch_khat: gam, alp -> out; f64: complex double) that ride as extra
// workgroups of K_PATCH_ROWS in launch_patch; n = 0: none
struct PatchKhat {
    int n = 0;
    const double* gam = nullptr;
    const double* alp = nullptr;
    void* out = nullptr;
    bool f64 = false;
};
void launch_patch(hipStream_t s, int N, int ntd, int ndir, const TaskPar* d_tp, const double* d_aotab,
                  double cfit, const void* d_twk, double* d_P, void* d_T, double* d_sp, bool f64,
                  const PatchKhat& kh = PatchKhat(), const LayerMix& mix = LayerMix());
void launch_dphi_series(hipStream_t s, int N, int ntd, int ndir, const TaskPar* d_tp, const void* d_T,
                        const double* d_sp, const void* d_coef, const void* d_twk, double scale2,
                        void* d_D0t, float* d_dlin, bool f64out, int* d_zero, int ncu,
                        const unsigned* d_support = nullptr);
// d_support [N/2+1]: per line, the pieces of series_lanes(N) columns inside the support of the telescope OTF
// (launch_series_support from d_tel, once per context); launch_dphi_series neither evaluates nor stores the others
void launch_series_support(hipStream_t s, int N, const void* d_tel, bool f64, unsigned* d_support);
// d_dlin: [ntd][N/2+1][N/32] minima of max(D, 0) per line and block of 32 columns, written by
// launch_dphi_series when not nullptr; launch_dmin16 turns them into what launch_dmin computes from D
void launch_dmin16(hipStream_t s, int N, int ntd, const float* d_dlin, float* d_dline, float* d_dblk);
void launch_tel_linemax(hipStream_t s, int N, const void* d_tel, float* d_tlmax, bool f64 = false);
void launch_vkeep(hipStream_t s, int N, int ntask, int ndir, int nl, const LamPar* d_lp,
                  const float* d_dline, const float* d_dblk, const float* d_tlmax, float thr_sum,
                  int* d_vkeep, int fixed, float* d_dminb);
// d_order: [ntask] the tasks by descending work (dispatch order of launch_otf_mfma)
void launch_task_order(hipStream_t s, int ntask, int nl, const int* d_vkeep, int* d_order);
// Per-wavelength stage of the mixed-precision path on the matrix cores (otf_mfma.hip): operand
// tables per wavelength set, constant telescope tables, and the fused kernel D -> stamps.
size_t mf_etab_bytes(int N, int nl);
size_t mf_gtab_bytes(int N, int nl);
size_t mf_tl2_bytes(int N);
size_t mf_tlb_bytes(int N);
size_t mf_dminb_bytes(int N, int ntask);
int mf_block_count(int N);
void launch_mf_tables(hipStream_t s, int N, int nl, const LamPar* d_lp, const void* d_tw64,
                      void* d_E, void* d_G);
void launch_mf_tel(hipStream_t s, int N, const void* d_tel, float* d_tl2, float* d_tlb);
// d_vkeep / d_dminb: nullptr = no line / block pruning; thr: log2 of the block threshold;
// d_order: dispatch order of the tasks (or nullptr)
// K_PEAK_FLOOR: per-task floor of launch_otf_mfma's block rule under the tier budget (d_thrf [ntask])
void launch_peak_floor(hipStream_t s, int N, int ntask, int ndir, const void* d_D0t, const float* d_tl2, float c2min,
                       float tier_half, float floor_nominal, float* d_thrf);
void launch_otf_mfma(hipStream_t s, int N, int ntask, int ndir, int nl, const void* d_D0t,
                     const float* d_tl2, const LamPar* d_lp, const void* d_E, const void* d_G,
                     const int* d_vkeep, const float* d_dminb, const float* d_tlb, float thr,
                     void* d_pre, const int* d_order = nullptr, void* d_clk = nullptr, const float* d_thrf = nullptr);
// Second generation of the matrix-core stage (otf_mfma2.hip, one direction): block masks per
// (task, wavelength) in two precision tiers, then the thin-wave kernel.  permax: wavelengths per
// workgroup (7: 14 waves of 128 registers; 6: 12 waves of 168).
size_t mf2_own_bytes(int N, int ntask, int nl);
size_t mf2_uni_bytes(int N, int ntask, int nl);
size_t mf2_sched_bytes(int N, int ntask, int nl, int permax);
size_t mf2_part_bytes(int N, int ntask, int nl);
void mf2_groups(int nl, int permax, int* per, int* ngr);
// K_MF_PREP: block masks and the work lists of launch_otf_mfma2 from the block minima of launch_dmin
// (d_dminb = nullptr: no pruning); d_sched[0..16] must be zero (launch_colfft_dphi does that)
// thr: the eps rule; thr_floor / thr_mid: the precision tiers, applied per (task, wavelength) as far as the OTF
// mass each leaves out stays below tier_half of a lower bound of the PSF peak (d_D0t, d_tl2; tier_half <= 0: no budget)
void launch_mf_prep(hipStream_t s, int N, int ntask, int nl, int permax, const LamPar* d_lp,
                    const float* d_dminb, const float* d_tlb, float thr, float thr_floor, float thr_mid,
                    float tier_half, const void* d_D0t, const float* d_tl2, void* d_own,
                    void* d_uni, void* d_sched, const float* d_dlin = nullptr);
// (d_dlin: instead of d_dminb, the per-line block minima of launch_dphi_series -- the minimum over a
// block's 16 lines is then taken by the kernel itself and launch_dmin16 is not needed)
// K_OTF_MFMA2 (persistent, ncu workgroups) + K_MF_FINISH
void launch_otf_mfma2(hipStream_t s, int N, int ntask, int nl, int permax, int ncu, const void* d_D0t,
                      const float* d_tl2, const LamPar* d_lp, const void* d_E, const void* d_G,
                      const void* d_own, const void* d_uni, void* d_sched, void* d_part, void* d_pre,
                      void* d_clk = nullptr, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_gtable(hipStream_t s, int N, int nl, const LamPar* d_lp, const void* d_tw64,
                   int* d_samp_p, void* d_samp_a, void* d_G, bool f64);
void launch_moffat_kernels(hipStream_t s, int nker, const double* d_gamma, const double* d_alpha,
                           void* d_out, bool f64);
// d_xtab: extraction table of the radix-16 plans (launch_xtab), used when otf_uses_r16()
void launch_otf_rowfft(hipStream_t s, int N, int ntask, int ndir, int nl, const void* d_D0t,
                       const void* d_tel, const LamPar* d_lp, const int* d_samp_p,
                       const void* d_samp_a, const void* d_xtab, void* d_Tq, const void* d_tw64,
                       bool f64, bool fast_exp, const int* d_vkeep);
bool otf_uses_r16(int N, bool f64, int nl, int ndir);
size_t xtab_bytes(int nl);
void launch_xtab(hipStream_t s, int N, int nl, const int* d_samp_p, const void* d_samp_a,
                 const void* d_tw64, void* d_xtab);
// d_pre: stamps before the convolutions, float (mixed) or double (f64)
// d_vkeep: [ntask][(nl+1)/2] lines to read per (task, wavelength pair), or nullptr for all
void launch_colpass(hipStream_t s, int N, int ntask, int nl, const void* d_Tq, const void* d_G,
                    void* d_pre, bool f64, const int* d_vkeep);
// tdiv: stamp group g (blockIdx.y of the launch) takes the tip-tilt kernel g / tdiv -- 1 for one group per task; the
// field call (mpsfr_reconstruct_field) lays its chunks out as (task, position) groups and passes npos
void launch_conv(hipStream_t s, int ntask, int nl, const void* d_pre, const void* d_ktt,
                 const void* d_kmuse, double* d_fin, bool f64, int tdiv = 1);
void launch_khat(hipStream_t s, int nker, const double* d_gamma, const double* d_alpha,
                 void* d_khat, bool f64 = false);
// fin_f32 / stamps_f32: the final stamps are float (inside the pipeline) instead of double
// f64: double stamps in and out, fp64 transforms, khat tables of complex double
void launch_conv_fft(hipStream_t s, int ntask, int nl, const void* d_pre, const void* d_khat_tt,
                     const void* d_khat_muse, void* d_fin, bool fin_f32, bool f64 = false, int tdiv = 1);
// (sum_*: the deterministic sum of the stamps over the sum_ntask tasks of the chunk -- [sum_nl][40][40] into d_sum,
// added to it if sum_accumulate -- as the first workgroups of the same launch; d_sum = nullptr: none)
void launch_fit(hipStream_t s, int nstamp, const void* d_stamps, bool stamps_f32, double* d_fit,
                bool f64, int sum_ntask = 0, int sum_nl = 0, double* d_sum = nullptr, int sum_accumulate = 0);
void launch_stamp_sum(hipStream_t s, int ntask, int nl, const void* d_fin, bool fin_f32, double* d_sum,
                      int accumulate);
// elliptical Moffat fit (fit_ell.hip): [nstamp][40][40] double stamps -> [nstamp][NFIT_ELL]
void launch_fit_ell(hipStream_t s, int nstamp, const double* d_stamps, double* d_fit, bool f64);
// weighted Moffat fit of observed stars (fit_obs.hip): [nstamp][40][40] double stamps and variances (d_var = nullptr:
// unit weights) -> [nstamp][NFIT_ELL]; flags: MPSFR_FIT_BACKGROUND | MPSFR_FIT_ELLIPTICAL
void launch_fit_obs(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int flags, double* d_fit,
                    bool f64);
// PSF-model fit of observed stars (fit_psf.hip): star d_stamps[k] ([nstamp][40][40], d_var as launch_fit_obs) against
// the model stamp d_psf[d_index[k]] ([npsf][40][40]; d_index = nullptr: d_psf[k]) -> [nstamp][NFIT_PSF]; d_shift
// [nstamp][2]: the start values of (dp, dq), or nullptr; flags: MPSFR_FIT_BACKGROUND | MPSFR_FIT_FIXED_SHIFT
void launch_fit_psf(hipStream_t s, int nstamp, const double* d_stamps, const double* d_var, int npsf,
                    const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit,
                    bool f64);
// PSF-model fit of blended groups (fit_group.hip, fit_group_f64.hip): stamp d_stamps[k] holds nsrc (2 .. 4) sources of
// the model stamp d_psf[d_index[k]] at the positions d_shift[k] ([nstamp][nsrc][2], required) -> [nstamp][NFIT_GROUP];
// flags: MPSFR_FIT_BACKGROUND | one of MPSFR_FIT_FIXED_SHIFT, MPSFR_FIT_COMMON_SHIFT; grid(nstamp), block(64)
void launch_fit_group(hipStream_t s, int nstamp, int nsrc, const double* d_stamps, const double* d_var, int npsf,
                      const double* d_psf, const int32_t* d_index, const double* d_shift, int flags, double* d_fit,
                      bool f64);
// PSF-model fit of star cubes (fit_spec.hip): star d_cubes[k] ([nstar][nl][40][40], d_var likewise or nullptr) against
// the model cube d_psf[d_index[k]] ([npsf][nl][40][40]; d_index = nullptr: d_psf[k]) -> [nstar][16 + 10 nl]; d_shift
// [nstar][2]: the start of (dp, dq), or nullptr; d_x [nl] (device): the abscissa of the drift, or nullptr; flags:
// MPSFR_FIT_BACKGROUND | MPSFR_FIT_DRIFT; nl <= 4096; grid(nstar), block(256).  Both modes run in fp64.
void launch_fit_spec(hipStream_t s, int nstar, int nl, const double* d_cubes, const double* d_var, int npsf,
                     const double* d_psf, const int32_t* d_index, const double* d_shift, const double* d_x, int flags,
                     double* d_fit, bool f64);
// PSF energy metrics (metrics.hip): [nstamp][40][40] double stamps -> [nstamp][METRIC_HEAD + nrad + nbox + nfrac];
// d_centers [nstamp][2] (p, q) or nullptr (the centroid); radii / boxes / fractions: host arrays (they travel as kernel
// arguments), counts 0..METRIC_MAX
void launch_stamp_metrics(hipStream_t s, int nstamp, const double* d_stamps, const double* d_centers, int nrad,
                          const double* radii, int nbox, const double* boxes, int nfrac, const double* fractions,
                          double* d_out);
// Frame-level photometry (render.hip).  launch_cut_stamps: [nstar][40][40] stamps (and variances, d_var / d_var_out both
// nullptr or both set) out of the frame d_image [ny][nx] at d_origin [nstar][2]; NaN (0) off the frame.
// launch_render_stars: d_image_out = d_image_in (nullptr: zeros) +- sum_k d_scale[k] P~_k, the stars in index order at
// every pixel (mpsfr_render_stars, include/mpsfr.h); d_image_out may be d_image_in; d_star_out [nstar][4] or nullptr;
// d_ws: render_workspace_bytes(ny, nx, nstar) bytes of work lists, which the launch itself clears on the stream.
void launch_cut_stamps(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, int nstar,
                       const int32_t* d_origin, double* d_stamps, double* d_var_out);
// The stars of a frame call, by value to launchers and kernels (device pointers): star k is the model stamp
// psf[index[k]] (index nullptr: psf[k]) of psf [npsf][40][40], its pixel [0][0] on the frame pixel origin[2 k], [2 k + 1],
// resampled at shift[2 k], [2 k + 1] (nullptr: zeros).  The scales are an argument of their own: the frame fit walks one
// list with several vectors.  (Here and not in frame_common.h, because the host code fills it.)
// For the layers of a cube (cube_fit.hip) psf is [npsf][nl][40][40] and star k of layer `layer` is the model stamp
// psf[index[k]][layer] resampled at shift[k] + lshift[2 layer], [2 layer + 1] (one rounded addition; lshift nullptr:
// shift[k] itself); a frame call is the one layer of nl = 1.
struct StarList {
    int nstar, npsf;
    const double* psf;
    const int32_t *index, *origin;
    const double* shift;
    const double* lshift = nullptr;
    int nl = 1, layer = 0;
};
size_t render_workspace_bytes(int ny, int nx, int nstar);
void launch_render_stars(hipStream_t s, int ny, int nx, const double* d_image_in, StarList stars, const double* d_scale,
                         bool subtract, double* d_image_out, double* d_star_out, void* d_ws);
// The two halves of launch_render_stars, for a caller that walks the same lists many times (frame_fit.hip):
// launch_render_lists builds the per-tile star lists in d_ws (prepare, scan, fill; RenderLists of frame_common.h is
// where they lie) -- with d_accept [nstar] only of the stars it marks, which pass FrameStar's rule (d_scale may then be
// nullptr) --, launch_render_walk is the tile walk alone; with d_done it does nothing once *d_done is not 0.
void launch_render_lists(hipStream_t s, int ny, int nx, StarList stars, const double* d_scale, const int32_t* d_accept,
                         double* d_star_out, void* d_ws);
void launch_render_walk(hipStream_t s, int ny, int nx, const double* d_image_in, StarList stars, const double* d_scale,
                        bool subtract, double* d_image_out, void* d_ws, const int32_t* d_done);
// For the layers of a cube (cube_fit.hip, through frame_fit_impl.h): launch_render_lists with neither d_scale nor
// d_accept lists every star whose index and origin are in range and whose footprint meets the frame, whatever its shift;
// launch_render_sort sorts every tile's list by star index in place, once; launch_render_walk_layers is the tile walk
// of `layers` frames side by side over such lists -- frame, scales (at a pitch of scale_pitch doubles) and done word
// (at done_pitch int32) of layer b, star k of it summed only where d_accept[b nstar + k] is not 0, in index order.
void launch_render_sort(hipStream_t s, int ny, int nx, int nstar, void* d_ws);
void launch_render_walk_layers(hipStream_t s, int ny, int nx, int layers, const double* d_image_in, StarList stars,
                               const double* d_scale, int scale_pitch, const int32_t* d_accept, bool subtract,
                               double* d_image_out, void* d_ws, const int32_t* d_done, int done_pitch);
// d_offset[t] = sum of d_count[0 .. t - 1], d_offset[nt] = the total: the scan of the frame calls' counts (render.hip)
void launch_scan_counts(hipStream_t s, int nt, const int* d_count, int* d_offset);
// The star finder (find.hip; mpsfr_find_stars, include/mpsfr.h): the statistic T of every pixel of d_image [ny][nx]
// (d_var [ny][nx] or nullptr) with the (2 half + 1)^2 core of the model stamp d_psf [40][40], its peaks over (2 sep + 1)^2
// squares at or above `threshold` in pixel order into d_star_out [max_stars][8] and d_origin_out [max_stars][2] (or
// nullptr), their number into d_count_out [1], filler rows behind them; T into d_map_out [ny][nx] if it is given.
// d_ws: find_workspace_bytes(ny, nx, max_stars, d_map_out != nullptr) bytes; the launch writes every word of it before it reads it.
size_t find_workspace_bytes(int ny, int nx, int max_stars, bool with_map);
void launch_find_stars(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, const double* d_psf,
                       int half, int sep, double threshold, int max_stars, double* d_star_out, int32_t* d_origin_out,
                       int32_t* d_count_out, double* d_map_out, void* d_ws);
// The background map (background.hip; mpsfr_frame_background, include/mpsfr.h): the clipped median and MAD of every
// box x box cell of every layer of d_image [nl][ny][nx] (d_var of that shape or nullptr: a mask), kc = kappa 1.4826,
// filtered over filter x filter cells into d_mesh_out [nl][my][mx][8] and d_head_out [nl][4]; the level plane
// interpolated into d_map_out, the rms plane into d_rms_out, d_apply_to minus the map into d_applied_out (each
// [nl][ny][nx] or nullptr; d_applied_out may be d_apply_to).  No work memory: the later kernels read mesh_out and head_out.
void launch_frame_background(hipStream_t s, int nl, int ny, int nx, const double* d_image, const double* d_var, int box,
                             int filter, double kc, int max_clip, double min_frac, const double* d_apply_to,
                             double* d_mesh_out, double* d_head_out, double* d_map_out, double* d_rms_out,
                             double* d_applied_out);
// Friends-of-friends groups of stars (group.hip; mpsfr_group_stars, include/mpsfr.h): the connected components of
// "d2 <= crit^2" over the positions d_pos [nstar][stride] (columns 0 and 1: y, x) -- labels into d_label_out [nstar],
// rows in (class, label) order into d_group_out [max_groups][8] and d_origin_out [max_groups][2], shifts at the
// per-class pitch into d_shift_out [max_groups][8] (both or neither), the six counts into d_count_out.
// d_ws: group_workspace_bytes(ny, nx, nstar, max_groups) bytes; the launch writes every word of it before it reads it.
size_t group_workspace_bytes(int ny, int nx, int nstar, int max_groups);
void launch_group_stars(hipStream_t s, int ny, int nx, int nstar, const double* d_pos, int stride, double crit,
                        int max_groups, int32_t* d_label_out, int32_t* d_group_out, int32_t* d_origin_out,
                        double* d_shift_out, int32_t* d_count_out, void* d_ws);
// The four crowded-field fits below are one family.  frame_fit_impl.h holds the flux-only solve in its frame and layer
// forms and what every step kernel shares (the block reduction, the conjugate-gradient step, a star's row, a head);
// frame_free_impl.h the three-column walk and projection and what the two fits with free positions share (the scalar
// words, the carry rule, the first residual's places, the position update).
// Crowded-field photometry (frame_fit.hip; mpsfr_fit_frame_psf, include/mpsfr.h): the fluxes of all accepted stars and,
// with `background`, one constant by preconditioned conjugate gradients on the frame d_image / d_var (or nullptr), at
// most max_iter steps queued at once, into d_star_out [nstar][8], d_head_out [8] and d_resid_out [ny][nx] (or nullptr).
// d_ws: frame_fit_workspace_bytes(ny, nx, nstar) bytes -- the renderer's lists, two frames of doubles, 7 nstar +
// 4 ceil(ny nx / 4096) + 9 doubles, 2 nstar + 5 int32 (FrameFitWork, frame_fit_impl.h); the launch writes every word of it
// before it reads it.
size_t frame_fit_workspace_bytes(int ny, int nx, int nstar);
void launch_fit_frame(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, StarList stars,
                      const double* d_scale0, double radius, bool background, int max_iter, double tol,
                      double* d_star_out, double* d_head_out, double* d_resid_out, void* d_ws);
// Crowded-field photometry with free positions (frame_free.hip; mpsfr_fit_frame_psf_free, include/mpsfr.h): an opening
// solve of launch_fit_frame's problem at the shifts of `stars`, up to max_outer Gauss-Newton steps over the fluxes and
// the shifts of the free stars, a closing solve at the final shifts; Omega and the accepted stars are those of the
// start.  d_star_out [nstar][16], d_shift_out [nstar][2], d_head_out [12], d_resid_out [ny][nx] (or nullptr); everything
// is queued at once.  d_ws: frame_free_workspace_bytes(ny, nx, nstar) bytes -- the renderer's lists, two frames of
// doubles, 36 nstar + 8 ceil(ny nx / 4096) + 11 doubles, 6 nstar + 12 int32 (FrameFreeWork, frame_free.hip); the launch
// writes every word of it before it reads it.
size_t frame_free_workspace_bytes(int ny, int nx, int nstar);
void launch_fit_frame_free(hipStream_t s, int ny, int nx, const double* d_image, const double* d_var, StarList stars,
                           const double* d_scale0, double radius, bool background, int max_iter, double tol,
                           int max_outer, double pos_tol, double max_step, double max_move, double min_snr,
                           double* d_star_out, double* d_shift_out, double* d_head_out, double* d_resid_out,
                           void* d_ws);
// Crowded-field photometry of the layers of a cube (cube_fit.hip; mpsfr_fit_cube_psf, include/mpsfr.h): `layers` solves
// of launch_fit_frame side by side, bit for bit -- d_cube, d_var (or nullptr), d_resid_out (or nullptr)
// [layers][ny][nx], d_scale0 [layers][nstar] (or nullptr), d_star_out [layers][nstar][8], d_head_out [layers][8];
// layer b takes the models stars.psf[index][b] of [npsf][stars.nl][40][40] and the shifts stars.shift[k] +
// stars.lshift[2 b], [2 b + 1] (nullptr: stars.shift[k]).  d_ws: cube_fit_workspace_bytes(ny, nx, nstar, layers) bytes:
// the renderer's lists once, and `layers` times what launch_fit_frame has behind them.
size_t cube_fit_workspace_bytes(int ny, int nx, int nstar, int layers);
void launch_fit_cube(hipStream_t s, int ny, int nx, int layers, const double* d_cube, const double* d_var,
                     StarList stars, const double* d_scale0, double radius, bool background, int max_iter, double tol,
                     double* d_star_out, double* d_head_out, double* d_resid_out, void* d_ws);
// Crowded-field photometry of a cube with free positions (cube_free.hip; mpsfr_fit_cube_psf_free, include/mpsfr.h):
// launch_fit_frame_free's loop over all `layers` layers jointly, one shift per star -- the arrays of launch_fit_cube,
// d_star_out [layers][nstar][8], d_head_out [layers][8], d_pos_out [nstar][8], d_shift_out [nstar][2], d_call_out [8],
// d_resid_out [layers][ny][nx] (or nullptr); everything is queued at once.  d_ws: cube_free_workspace_bytes(ny, nx,
// nstar, layers) bytes -- the renderer's lists once; per layer two frames of doubles, 25 nstar + 8 ceil(ny nx / 4096) +
// 17 doubles and 4 nstar + 5 int32; once 14 nstar + 10 doubles and 5 nstar + 11 int32 (CubeFreeWork, cube_free.hip); the
// launch writes every word of it before it reads it.
size_t cube_free_workspace_bytes(int ny, int nx, int nstar, int layers);
void launch_fit_cube_free(hipStream_t s, int ny, int nx, int layers, const double* d_cube, const double* d_var,
                          StarList stars, const double* d_scale0, double radius, bool background, int max_iter,
                          double tol, int max_outer, double pos_tol, double max_step, double max_move, double min_snr,
                          double* d_star_out, double* d_head_out, double* d_pos_out, double* d_shift_out,
                          double* d_call_out, double* d_resid_out, void* d_ws);
// band-integrated stamps (band.hip): d_fin [ntb][nl][40][40] (float if fin_f32, else double) reduced over wavelength
// into d_out [ntb][nband][40][40] double with the weights d_w [nl][band_stride(nband)] (zero beyond nband)
constexpr int MAX_BANDS = 16;    // MPSFR_MAX_BANDS
int band_stride(int nband);      // the power of two >= nband the kernel is instantiated for
void launch_band_reduce(hipStream_t s, int ntb, int nl, int nband, const void* d_fin, bool fin_f32,
                        const double* d_w, double* d_out);
// the call's parameter blob from pinned host memory into device memory, as a kernel of the call's own queue
// (bytes: a multiple of 16); h_flag_pinned: a pinned host word that receives `seq` once the blob has been read
void launch_param_copy(hipStream_t s, void* d_dst, const void* h_src_pinned, size_t bytes,
                       unsigned long long* h_flag_pinned = nullptr, unsigned long long seq = 0);

}  // namespace mpsfr
