// Host side of libmpsfr: context, workspaces, the chunked pipeline and its part of the C ABI of
// include/mpsfr.h (the stamp, frame and cube calls are in stamp_calls.cpp).  Reference citations are to /root/reference/muse_psfr/psfrec.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "coeff_l0_table.h"
#include "host_ctx.h"

using namespace mpsfr;
using namespace mpsfr::host;

int mpsfr::host::resolve_profile(mpsfr_ctx* c) {
    if (c->pending.empty()) return MPSFR_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
        if (c->lane[k].stream) HIPCHK(hipStreamSynchronize(c->lane[k].stream));
    for (auto& p : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->prof_ms[p.id] += ms;
            c->prof_n[p.id] += 1;
        }
        c->pool.push_back(p.a);
        c->pool.push_back(p.b);
    }
    c->pending.clear();
    return MPSFR_OK;
}

namespace {

const char* kKernelNames[K_COUNT] = {
    "ao_tables", "tel_otf", "psd_rowfft", "colfft_dphi", "gtable",
    "moffat_kernels", "otf_rowfft", "colpass", "conv", "fit", "stamp_sum", "vkeep", "otf_mfma", "mf_prep",
    "patch", "dphi_series"};

// wait for an asynchronous host-output call and hand its results to the caller's arrays
int complete_ticket(mpsfr_ctx* c, mpsfr_ctx::Ticket& tk) {
    if (!tk.pending) return MPSFR_OK;
    HIPCHK(hipEventSynchronize(tk.done));
    const double* h = (const double*)tk.host;
    if (tk.u_psf) memcpy(tk.u_psf, h, tk.n_psf * sizeof(double));
    if (tk.u_sum) memcpy(tk.u_sum, h + tk.n_psf, tk.n_sum * sizeof(double));
    if (tk.u_fit) memcpy(tk.u_fit, h + tk.n_psf + tk.n_sum, tk.n_fit * sizeof(double));
    tk.pending = false;
    return MPSFR_OK;
}

// workgroups of a persistent kernel on a lane: one per CU the lane may use, less the reserve
template <class LaneT>
int persist_grid(const mpsfr_ctx* c, const LaneT& ln, int reserve, bool shared) {
    const int n = ln.ncu ? ln.ncu : c->ncu;
    if (reserve < 0) reserve = (shared && !ln.ncu) ? n / 8 : 0;         // (CU-masked lanes are partitioned already)
    return n - reserve >= n / 2 ? n - reserve : n / 2;
}

bool supported_dim(int n) { return n == 128 || n == 256 || n == 512 || n == 1024 || n == 1280; }

// np.interp(L0, arange(1, 201), coeff)  (psfrec.py:897)
double interp_coeff(double l0) {
    if (l0 <= 1.0) return kCoeffL0[0];
    if (l0 >= 200.0) return kCoeffL0[kCoeffL0N - 1];
    int j = (int)std::floor(l0) - 1;
    if (j > kCoeffL0N - 2) j = kCoeffL0N - 2;
    const double x0 = (double)(j + 1);
    const double slope = (kCoeffL0[j + 1] - kCoeffL0[j]) / 1.0;
    return slope * (l0 - x0) + kCoeffL0[j];
}

// Moffat alpha [px] of the residual tip-tilt kernel (psfrec.py:879-905)
double tiptilt_alpha(double seeing, double gl, double l0, double pixscale) {
    const double seeingHL = seeing * std::pow(1.0 - gl, 3.0 / 5.0);
    const double r0HL = 0.976 * 0.5 / seeingHL / 4.85;
    const double coeffHL = interp_coeff(l0);
    const double two_pi = 2.0 * M_PI;
    const double a = (0.5 * 1.0e-6 / two_pi);
    const double fwhm = std::sqrt(coeffHL * 0.97 * 6.88 * (a * a) * std::pow(8.0, -1.0 / 3.0) *
                                  std::pow(r0HL, -5.0 / 3.0)) /
                        (4.85 * 1.0e-6) * 2.35 / pixscale;
    // GL = 1: no turbulence above the ground layer, seeingHL = 0, r0HL = inf, and the width is 0 -- the identity
    // kernel, the limit GL -> 1 (the reference's Moffat2DKernel(0, 2) divides 0 by 0 at its centre and is NaN).  The
    // kernels evaluate (1 + r^2 / gamma^2)^-2 in fp64, so they need no branch if gamma stays positive: with
    // gamma = 1e-100, r^2 / gamma^2 >= 1e200 for r >= 1, its square overflows to +inf and the tap is exactly 0, and
    // the centre is (1 + 0 / 1e-200)^-2 = 1.  Any width below 1e-78 does (then (r / gamma)^4 > DBL_MAX); 1e-100 keeps
    // gamma^2 a normal number.  GL = 1 - 1e-12 gives gamma ~ 1e-8 px, taps of 1e-32: the floor is never felt below 1.
    // (The floor masks no invalid input: std::max(NaN, floor) is NaN, and the argument check refuses GL > 1.)
    constexpr double kTipTiltFloor = 1.0e-100;
    return std::max(fwhm / (2.0 * std::sqrt(std::pow(2.0, 1.0 / 2.0) - 1.0)), kTipTiltFloor);
}

double polyval6(const double* p, double x) {
    double y = 0.0;
    for (int i = 0; i < 6; ++i) y = y * x + p[i];
    return y;
}

// muse_intrinsic_psf (psfrec.py:1144-1171) -> Moffat (alpha px, beta) of the instrument kernel
void muse_kernel_params(double lbda_nm, double pixscale, double* alpha_px, double* beta) {
    static const double pol_beta[6] = {-0.83704697, 1.1337153, 0.0609222,
                                       -1.35581762, 1.15237178, 2.2106042};
    static const double pol_fwhm[6] = {0.60467385, -1.58905792, 1.75293264,
                                       -1.0368302, 0.21487023, 0.34851139};
    const double lb = (10.0 * lbda_nm - 4750.0) / (9350.0 - 4750.0);
    const double fwhm = polyval6(pol_fwhm, lb) / pixscale;
    const double b = polyval6(pol_beta, lb);
    *beta = b;
    *alpha_px = fwhm / (2.0 * std::sqrt(std::pow(2.0, 1.0 / b) - 1.0));
}

// npixc, psfrec.py:663-664 (np.round = round half to even = nearbyint in the default mode)
int npix_crop(double lbda_nm, int dimpsf, double pixscale) {
    const double x = ((((dimpsf * pixscale) * 2) * 8) * 4.85) * 1000;
    return (int)(std::nearbyint((x / lbda_nm) / 2.0) * 2.0);
}

double fit_constant() {
    return (std::tgamma(11.0 / 6.0) * std::tgamma(11.0 / 6.0) / (2.0 * std::pow(M_PI, 11.0 / 3.0))) *
           std::pow(24.0 * std::tgamma(6.0 / 5.0) / 5.0, 5.0 / 6.0);   // psfrec.py:622-623
}

double dphi_scale2() {
    const double k500 = 0.5 * 1000 / (2 * M_PI);                      // psfrec.py:151
    return 2.0 * (k500 * k500) / 256.0;       // 2 (.)/L^2, L = 16 m (psfrec.py:710, 718)
}

// Series form of stage A (stage_a2.hip): the structure functions of the terms
// binom(-11/6, k) cfit (f^2 + eps0)^(-11/6 - k) [f >= fc] of the fitting PSD, computed once with the
// full-size fp64 transforms of stage_a.hip ("basis tasks": r0m53 = the binomial coefficient,
// inv_l0sq = eps0), then interleaved per pixel in the precision of the context.
int build_series_tables(mpsfr_ctx* c) {
    const int N = c->N, H1 = N / 2 + 1, K = series_terms(c->f64);
    std::vector<TaskPar> tp(K);
    double binom = 1.0;
    for (int k = 0; k < K; ++k) {
        if (k > 0) binom *= (-11.0 / 6.0 - (k - 1)) / k;
        tp[k].r0m53 = binom;
        tp[k].inv_l0sq = series_eps0();
        tp[k].cn2_0 = 1.0;
        tp[k].cn2_1 = 0.0;
        tp[k].geom = 0;
        tp[k].basis = k + 1;
    }
    DevBuf dtp, C, s00, planes;
    int rc = MPSFR_OK;
    auto done = [&](int code) {
        release(dtp); release(C); release(s00); release(planes);
        return code;
    };
    if ((rc = ensure(c, dtp, K * sizeof(TaskPar)))) return done(rc);
    if ((rc = ensure(c, C, (size_t)K * (N / 2 + NAO / 2) * H1 * 2 * sizeof(double)))) return done(rc);
    if ((rc = ensure(c, s00, (size_t)K * psd_rowfft_groups(N) * sizeof(double)))) return done(rc);
    if ((rc = ensure(c, planes, (size_t)K * H1 * N * sizeof(double)))) return done(rc);
    if ((rc = ensure(c, c->scoef, (size_t)K * H1 * N * rsize(c)))) return done(rc);
    if (hipMemcpy(dtp.p, tp.data(), K * sizeof(TaskPar), hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(MPSFR_E_HIP, "hipMemcpy of the basis tasks failed"));
    launch_psd_rowfft(c->stream, N, K, 1, (const TaskPar*)dtp.p, nullptr, fit_constant(), C.p, c->tw64.p,
                      (double*)s00.p, true);
    launch_colfft_dphi(c->stream, N, K, C.p, (const double*)s00.p, dphi_scale2(), planes.p, true, c->tw64.p);
    launch_series_coef(c->stream, N, (const double*)planes.p, c->scoef.p, c->f64);
    if ((rc = ensure(c, c->stwk, series_twiddle_bytes(N)))) return done(rc);
    launch_series_twiddles(c->stream, N, c->tw64.p, c->stwk.p);
    if ((rc = ensure(c, c->ssup, (size_t)H1 * sizeof(unsigned)))) return done(rc);
    launch_series_support(c->stream, N, c->tel.p, c->f64, (unsigned*)c->ssup.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return done(fail(MPSFR_E_HIP, "building the series tables of stage A failed"));
    return done(MPSFR_OK);
}

int build_constant_tables(mpsfr_ctx* c) {
    const int N = c->N;
    // twiddles exp(-2 pi i m / N)
    std::vector<double> tw(2 * (size_t)N);
    for (int m = 0; m < N; ++m) {
        const long double ang = -2.0L * 3.141592653589793238462643383279502884L * m / N;
        tw[2 * m] = (double)cosl(ang);
        tw[2 * m + 1] = (double)sinl(ang);
    }
    int rc;
    if ((rc = ensure(c, c->tw64, tw.size() * sizeof(double)))) return rc;
    HIPCHK(hipMemcpy(c->tw64.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
    // pupil mask rows as bit masks: pupil_mask(dim/4, dim/2, oc=0.14), psfrec.py:190-203, 656
    const int H = N / 2, words = (H + 63) / 64, wpad = 2 * words + 1;
    std::vector<uint64_t> rows((size_t)H * wpad, 0);
    const double cen = (H - 1) / 2.0, radius = N / 4.0;
    long pupsum = 0;
    for (int x = 0; x < H; ++x)
        for (int y = 0; y < H; ++y) {
            const double rho = std::hypot(x - cen, y - cen) / radius;
            if (rho < 1.0 && rho >= 0.14) {
                rows[(size_t)x * wpad + (y >> 6)] |= (uint64_t)1 << (y & 63);
                ++pupsum;
            }
        }
    if ((rc = ensure(c, c->rows, rows.size() * sizeof(uint64_t)))) return rc;
    HIPCHK(hipMemcpy(c->rows.p, rows.data(), rows.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    if ((rc = ensure(c, c->tel, (size_t)(H + 1) * N * rsize(c)))) return rc;
    {
        ProfScope ps(c, K_TEL_OTF);
        launch_tel_otf(c->stream, N, (const uint64_t*)c->rows.p, words, (double)pupsum, c->tel.p,
                       c->f64);
    }
    // log2 of the line maxima of the telescope OTF (line pruning, stage_a.hip)
    if ((rc = ensure(c, c->tlmax, (size_t)(H + 1) * sizeof(float)))) return rc;
    launch_tel_linemax(c->stream, N, c->tel.p, (float*)c->tlmax.p, c->f64);
    if (!c->f64) {
        // log2 of the telescope OTF and of its block maxima (otf_mfma.hip)
        if ((rc = ensure(c, c->tl2, mf_tl2_bytes(N)))) return rc;
        if ((rc = ensure(c, c->tlb, mf_tlb_bytes(N)))) return rc;
        launch_mf_tel(c->stream, N, c->tel.p, (float*)c->tl2.p, (float*)c->tlb.p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return build_series_tables(c);
}


}  // namespace

extern "C" {

const char* mpsfr_last_error(void) { return g_err.c_str(); }

int mpsfr_version(void) { return 102; }

int mpsfr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

#ifndef MPSFR_BUILD_ID
#define MPSFR_BUILD_ID "unstamped"
#endif
const char* mpsfr_build_id(void) { return MPSFR_BUILD_ID; }

int mpsfr_create(mpsfr_ctx** out, int device_id, int dim, int dimpsf, double pixscale,
                 int precision) {
    if (!out) return fail(MPSFR_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!supported_dim(dim))
        return fail(MPSFR_E_INVALID, "dim=%d not supported (128, 256, 512, 1024, 1280)", dim);
    if (dimpsf != NS) return fail(MPSFR_E_INVALID, "dimpsf=%d not supported (only 40)", dimpsf);
    if (!(pixscale > 0.0)) return fail(MPSFR_E_INVALID, "pixscale must be > 0");
    if (precision != MPSFR_PREC_MIXED && precision != MPSFR_PREC_F64)
        return fail(MPSFR_E_INVALID, "precision must be 0 (mixed) or 1 (f64)");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev)
        return fail(MPSFR_E_INVALID, "device_id=%d out of range (%d devices)", device_id, ndev);
    HIPCHK(hipSetDevice(device_id));
    mpsfr_ctx* c = new mpsfr_ctx();
    c->device = device_id;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && ncu > 0)
            c->ncu = ncu;
    }
    c->N = dim;
    c->dimpsf = dimpsf;
    c->pixscale = pixscale;
    c->prec = precision;
    c->f64 = precision == MPSFR_PREC_F64;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(MPSFR_E_HIP, "hipStreamCreate failed");
    }
    {   // the pinned words of the parameter-copy kernels (optional: without them a lean call queues one marker)
        void* hp = nullptr;
        if (hipHostMalloc(&hp, mpsfr_ctx::NSTAGE * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess) {
            c->seq_host = (unsigned long long*)hp;
            for (int k = 0; k < mpsfr_ctx::NSTAGE; ++k) c->seq_host[k] = 0;
        }
    }
    const int rc = build_constant_tables(c);
    if (rc) {
        mpsfr_destroy(c);
        return rc;
    }
    *out = c;
    return MPSFR_OK;
}

void mpsfr_destroy(mpsfr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->pending) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    hipEvent_t evs[] = {c->tables_ready, c->cache_ready, c->lsum_done, c->stagger_ev, c->stream_tail};
    for (auto e : evs)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k) {
        mpsfr_ctx::Lane& ln = c->lane[k];
        if (ln.stream) { (void)hipStreamSynchronize(ln.stream); (void)hipStreamDestroy(ln.stream); }
        if (ln.done) (void)hipEventDestroy(ln.done);
        DevBuf* lb[] = {&ln.C, &ln.s00, &ln.D0t, &ln.Tq, &ln.pre, &ln.fin, &ln.dmin, &ln.dblk, &ln.vkeep, &ln.dminb, &ln.order, &ln.mown, &ln.muni, &ln.msched, &ln.mpart,
                         &ln.pP, &ln.pT, &ln.psp, &ln.dlin, &ln.thrf, &ln.band};
        for (auto b : lb) release(*b);
    }
    for (int k = 0; k < mpsfr_ctx::NSTAGE; ++k) {
        mpsfr_ctx::Slot& sl = c->slot[k];
        if (sl.staged) (void)hipEventDestroy(sl.staged);
        if (sl.call_done) (void)hipEventDestroy(sl.call_done);
        if (sl.host) (void)hipHostFree(sl.host);
        release(sl.params);
        release(sl.ktt);
    }
    for (int k = 0; k < mpsfr_ctx::NTICKET; ++k) {
        mpsfr_ctx::Ticket& tk = c->ticket[k];
        if (tk.done) (void)hipEventDestroy(tk.done);
        if (tk.host) (void)hipHostFree(tk.host);
        release(tk.dpsf);
        release(tk.dsum);
        release(tk.dfit);
    }
    DevBuf* all[] = {&c->scoef, &c->stwk, &c->ssup, &c->tw64, &c->tel, &c->rows, &c->tlmax, &c->tl2, &c->tlb, &c->aotab, &c->samp_p,
                     &c->samp_a, &c->G, &c->xtab, &c->etab, &c->gtab, &c->kmuse, &c->fit, &c->sum,
                     &c->stage, &c->lsum, &c->mfclk, &c->specx, &c->render, &c->find, &c->group, &c->framefit, &c->cubefit};
    for (auto b : all) release(*b);
    if (c->p2p.stream) { (void)hipStreamSynchronize(c->p2p.stream); (void)hipStreamDestroy(c->p2p.stream); }
    DevBuf* p2p[] = {&c->p2p.twm, &c->p2p.psd, &c->p2p.cm, &c->p2p.d0t, &c->p2p.pup, &c->p2p.phase, &c->p2p.lbda,
                     &c->p2p.cl, &c->p2p.t1, &c->p2p.q, &c->p2p.otf, &c->p2p.g, &c->p2p.out};
    for (auto b : p2p) release(*b);
    if (c->seq_host) (void)hipHostFree(c->seq_host);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mpsfr_set_option(mpsfr_ctx* c, const char* key, double value) {
    if (!c || !key) return fail(MPSFR_E_INVALID, "NULL argument");
    if (!strcmp(key, "chunk_tasks")) {
        if (value < 0 || value > 4096) return fail(MPSFR_E_INVALID, "chunk_tasks out of range");
        c->chunk_tasks = (int)value;
    } else if (!strcmp(key, "fast_exp")) {
        c->fast_exp = value != 0.0;
    } else if (!strcmp(key, "streams") || !strcmp(key, "cu_partition")) {
        const bool lanes = key[0] == 's';
        if (lanes && (value < 0.0 || value > 4.0 || value != (int)value))
            return fail(MPSFR_E_INVALID, "streams must be 0 (automatic) or 1..4");
        if (!lanes && value != 0.0 && value != 1.0) return fail(MPSFR_E_INVALID, "cu_partition must be 0 or 1");
        if (c->cu_partition || (!lanes && value != 0.0)) {
            // the lanes' streams carry their CU masks: drain and drop them, the next call creates them anew
            HIPCHK(hipSetDevice(c->device));
            for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k) {
                mpsfr_ctx::Lane& ln = c->lane[k];
                if (!ln.stream) continue;
                HIPCHK(hipStreamSynchronize(ln.stream));
                HIPCHK(hipStreamDestroy(ln.stream));
                ln.stream = nullptr;
                ln.busy = false;
                ln.marked = false;
                ln.ncu = 0;
            }
            HIPCHK(hipStreamSynchronize(c->stream));
            // everything has drained: no slot is owed to a lane any more (a lean call leaves call_pending /
            // last_lane behind, which the next call on another lane would chase through lane_end)
            for (int k = 0; k < mpsfr_ctx::NSTAGE; ++k) {
                c->slot[k].call_pending = false;
                c->slot[k].last_lane = -1;
                c->slot[k].staged_pending = false;
            }
        }
        if (lanes) c->nlanes = (int)value;
        else c->cu_partition = (int)value;
    } else if (!strcmp(key, "prune_fixed")) {
        c->prune_fixed = (int)value;
    } else if (!strcmp(key, "prune_eps_f64")) {
        if (!(value >= 0.0) || value > 1.0e-6) return fail(MPSFR_E_INVALID, "prune_eps_f64 must be in [0, 1e-6]");
        c->prune_eps_f64 = value;
    } else if (!strcmp(key, "prune_eps")) {
        if (!(value >= 0.0) || value > 1.0e-3) return fail(MPSFR_E_INVALID, "prune_eps must be in [0, 1e-3]");
        c->prune_eps = value;
    } else if (!strcmp(key, "otf_mfma")) {
        c->otf_mfma = value != 0.0;
    } else if (!strcmp(key, "mf_floor")) {
        c->mf_floor = value != 0.0;
    } else if (!strcmp(key, "mf_kernel")) {
        if (value != 1.0 && value != 2.0) return fail(MPSFR_E_INVALID, "mf_kernel must be 1 or 2");
        c->mf_kernel = (int)value;
    } else if (!strcmp(key, "cold_stagger")) {
        c->cold_stagger = (int)value;
    } else if (!strcmp(key, "mf_permax")) {
        if (value != (int)value || value < 1.0 || value > 7.0) return fail(MPSFR_E_INVALID, "mf_permax must be 1..7");
        c->mf_permax = (int)value;
    } else if (!strcmp(key, "persist_reserve") || !strcmp(key, "persist_reserve_mf") || !strcmp(key, "persist_reserve_a")) {
        if (value != (int)value || value < -1.0 || value > 128.0) return fail(MPSFR_E_INVALID, "%s must be -1 (automatic) or 0..128", key);
        if (key[15] == '\0' || key[16] == 'm') c->reserve_mf = (int)value;
        if (key[15] == '\0' || key[16] == 'a') c->reserve_a = (int)value;
    } else if (!strcmp(key, "support_skip")) {
        c->support_skip = value != 0.0;
    } else if (!strcmp(key, "head_fusion")) {
        c->head_fusion = value != 0.0;
    } else if (!strcmp(key, "param_copy")) {
        c->param_copy_kernel = value != 0.0;
    } else if (!strcmp(key, "tier_eps")) {
        if (!(value >= 0.0)) return fail(MPSFR_E_INVALID, "tier_eps must be >= 0 (inf: tiers without a budget)");
        c->tier_eps = value;
    } else if (!strcmp(key, "mf_floor_log2")) {
        c->mf_floor_log2 = value;
    } else if (!strcmp(key, "mf_mid_log2")) {
        c->mf_mid_log2 = value;
    } else if (!strcmp(key, "stage_a")) {
        if (value != 0.0 && value != 1.0 && value != 2.0)
            return fail(MPSFR_E_INVALID, "stage_a must be 0 (full-size transforms), 1 (automatic) or 2 (series + patch)");
        c->stage_a = (int)value;
    } else if (!strcmp(key, "mf_clock")) {
        c->mf_clock = value != 0.0;
        if (c->mf_clock) {
            const int rc = ensure(c, c->mfclk, (size_t)65536 * 8 * 8 * sizeof(unsigned long long));
            if (rc) return rc;
            HIPCHK(hipMemset(c->mfclk.p, 0, c->mfclk.cap));
        }
    } else if (!strcmp(key, "pipeline_calls")) {
        c->pipeline_calls = value != 0.0;
    } else if (!strcmp(key, "fft_conv")) {
        c->fft_conv = value != 0.0;
    } else if (!strcmp(key, "profile")) {
        c->profile = value != 0.0;
    } else if (!strcmp(key, "profile_every")) {
        if (value != (int)value || value < 1.0 || value > 1024.0) return fail(MPSFR_E_INVALID, "profile_every must be 1..1024");
        c->prof_every = (int)value;
    } else if (!strcmp(key, "profile_only")) {
        if (value != (int)value || value < -1.0 || value >= K_COUNT)
            return fail(MPSFR_E_INVALID, "profile_only must be -1 or a kernel id");
        c->prof_only = (int)value;
    } else {
        return fail(MPSFR_E_INVALID, "unknown option '%s'", key);
    }
    return MPSFR_OK;
}

int mpsfr_sync(mpsfr_ctx* c) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
        if (c->lane[k].stream) HIPCHK(hipStreamSynchronize(c->lane[k].stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (long t = c->ticket_next - mpsfr_ctx::NTICKET; t < c->ticket_next; ++t)
        if (t >= 0) {
            mpsfr_ctx::Ticket& tk = c->ticket[t % mpsfr_ctx::NTICKET];
            const int rc = tk.id == t ? complete_ticket(c, tk) : MPSFR_OK;
            if (rc) return rc;
        }
    return MPSFR_OK;
}

int mpsfr_abandon(mpsfr_ctx* c) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    int rc = MPSFR_OK;
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
        if (c->lane[k].stream && hipStreamSynchronize(c->lane[k].stream) != hipSuccess) rc = MPSFR_E_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = MPSFR_E_HIP;
    // the results stay in the library's staging sets; the caller's arrays are never written
    for (int k = 0; k < mpsfr_ctx::NTICKET; ++k) {
        mpsfr_ctx::Ticket& tk = c->ticket[k];
        tk.pending = false;
        tk.u_psf = tk.u_sum = tk.u_fit = nullptr;
    }
    c->multi.pending = false;
    c->multi.user_sum = nullptr;
    if (rc != MPSFR_OK) return fail(rc, "a stream failed while the pending calls were drained");
    return MPSFR_OK;
}

long mpsfr_last_ticket(mpsfr_ctx* c) { return c ? c->ticket_next - 1 : -1; }

int mpsfr_wait(mpsfr_ctx* c, long ticket) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    if (ticket < 0 || ticket >= c->ticket_next) return fail(MPSFR_E_INVALID, "ticket %ld was never issued", ticket);
    HIPCHK(hipSetDevice(c->device));
    // tickets complete in order (a later call's results never reach the caller before an earlier one's)
    long first = ticket - mpsfr_ctx::NTICKET + 1;
    if (first < 0) first = 0;
    for (long t = first; t <= ticket; ++t) {
        mpsfr_ctx::Ticket& tk = c->ticket[t % mpsfr_ctx::NTICKET];
        if (tk.id != t) continue;            // already completed and its slot reused
        const int rc = complete_ticket(c, tk);
        if (rc) return rc;
    }
    return MPSFR_OK;
}

int mpsfr_wait_event(mpsfr_ctx* c, void* hip_event) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    c->wait_next = (hipEvent_t)hip_event;
    return MPSFR_OK;
}

// What the entry points other than mpsfr_reconstruct add to a pipeline call.
struct StageIO {
    // mpsfr_reconstruct_field: stage A evaluates the npos caller positions pos [npos][2] (arcsec) instead of the
    // npsflin grid, and stage B keeps them apart -- every (task, position) pair is a one-direction task of its own
    int npos = 0;
    const double* pos = nullptr;
    // mpsfr_reconstruct_profile / mpsfr_simul_psd_profile: the layers of the profile (they replace h, the wind speed
    // and the fixed wind directions) and the rows' weights cn2 [ntask][layers->n] (each row normalised here)
    const AoLayers* layers = nullptr;
    const double* cn2 = nullptr;
    // mpsfr_reconstruct_band: each (task, position)'s stamps reduced over wavelength with the weights bw [nband][nl]
    // (every band normalised to sum 1); psf_out, psf_sum_out and fit_out hold nband planes in place of nl
    int nband = 0;
    const double* bw = nullptr;
};

// One call of the pipeline, as its entry point describes it to guarded_call and reconstruct_impl.  The defaults are
// those of the stage-level entry points, which set only what they use: one row of the reference's atmosphere (its
// values do not reach their result), one direction, one wavelength, host buffers.
static const double kSeeing = 1.0, kGl = 0.5, kL0 = 20.0, kLbda = 700.0, kH[2] = {100.0, 10000.0};

struct CallArgs {
    int ntask = 1;
    const double* seeing = &kSeeing;
    const double* gl = &kGl;          // (gl only sets the tip-tilt kernel, which a PSD does not use)
    const double* l0 = &kL0;
    const uint8_t* three_lgs = nullptr;
    const double* h = kH;             // [2]
    double wind_speed = 12.0;
    int npsflin = 1;
    int nl = 1;
    const double* lbda_nm = &kLbda;   // (a PSD does not use the per-wavelength tables)
    const uint8_t* mask_rec = nullptr;
    const uint8_t* mask_res = nullptr;
    double* psf_out = nullptr;
    double* psf_sum_out = nullptr;
    double* fit_out = nullptr;
    int on_device = 0;
};

// The rows, wavelengths, masks and outputs of an entry point (what the five pipeline entry points share)
static CallArgs pipeline_args(int ntask, const double* seeing, const double* gl, const double* l0,
                              const uint8_t* three_lgs, int nl, const double* lbda_nm, const uint8_t* mask_rec,
                              const uint8_t* mask_res, double* psf_out, double* psf_sum_out, double* fit_out,
                              int on_device) {
    CallArgs a;
    a.ntask = ntask, a.seeing = seeing, a.gl = gl, a.l0 = l0, a.three_lgs = three_lgs;
    a.nl = nl, a.lbda_nm = lbda_nm, a.mask_rec = mask_rec, a.mask_res = mask_res;
    a.psf_out = psf_out, a.psf_sum_out = psf_sum_out, a.fit_out = fit_out, a.on_device = on_device;
    return a;
}

// The drivers: the pipeline, and the three stage-level calls that enter or leave it at another stage (host buffers,
// synchronous, on the same lanes, slots and tables)
static int reconstruct_impl(mpsfr_ctx* c, const CallArgs& a, const StageIO& io);
static int simul_psd_impl(mpsfr_ctx* c, const CallArgs& a, const StageIO& io, double* psd_out);
static int psf_from_psd_impl(mpsfr_ctx* c, const CallArgs& a, const double* psd_in);
static int convolve_stamps_impl(mpsfr_ctx* c, const CallArgs& a, const double* pre_in);

// Every entry point that runs a driver goes through this guard.  A call that fails leaves the
// pipelining state as it found it: the lane rotation and the ring of parameter slots do not advance, and
// an event registered with mpsfr_wait_event is consumed (the caller may destroy it after the call,
// whatever the outcome).
extern "C++" template <class Driver>
static int guarded(mpsfr_ctx* c, Driver&& run) {
    const unsigned lane_rr0 = c->lane_rr, stage0 = c->stage_next;
    const int rc = run();
    if (rc != MPSFR_OK) {
        // whatever the failed call has queued (it may have cleared a slot's guard and started chunks
        // on other lanes) must have drained before the next call reuses the slot and the workspaces
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
            if (c->lane[k].stream) (void)hipStreamSynchronize(c->lane[k].stream);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        c->lane_rr = lane_rr0;
        c->stage_next = stage0;
        c->wait_next = nullptr;
        // (everything has drained: every pinned blob is free, whether or not the kernel that would have said so ran)
        for (int k = 0; k < mpsfr_ctx::NSTAGE; ++k) c->slot[k].staged_pending = false;
    }
    return rc;
}

static int guarded_call(mpsfr_ctx* c, const CallArgs& a, const StageIO& io = StageIO()) {
    return guarded(c, [&] { return reconstruct_impl(c, a, io); });
}

// The directions of a call: the npsflin x npsflin grid (npos = 0, where min_npos allows it) or the caller's npos
// positions pos [npos][2] (arcsec), which take npsflin = 0.  Positions go to stage A through `io`, and npsflin becomes
// 1: every position is one direction.
static int grid_or_positions(int min_npos, int npos, const double* pos, int& npsflin, StageIO& io) {
    if (npos < min_npos || npos > 25) return fail(MPSFR_E_INVALID, "npos=%d out of range %d..25", npos, min_npos);
    if (npos == 0) {
        if (npsflin < 1 || npsflin > 5) return fail(MPSFR_E_INVALID, "npsflin=%d out of range 1..5", npsflin);
        return MPSFR_OK;
    }
    if (npsflin != 0) return fail(MPSFR_E_INVALID, "a call with positions (npos >= 1) takes npsflin = 0");
    if (!pos) return fail(MPSFR_E_INVALID, "pos_arcsec is NULL");
    for (int k = 0; k < 2 * npos; ++k)
        if (!std::isfinite(pos[k]) || std::fabs(pos[k]) > 60.0)
            return fail(MPSFR_E_INVALID, "position %d: need finite |x|, |y| <= 60 arcsec", k / 2);
    io.npos = npos;
    io.pos = pos;
    npsflin = 1;
    return MPSFR_OK;
}

int mpsfr_reconstruct(mpsfr_ctx* c, int ntask, const double* seeing, const double* gl,
                      const double* l0, const uint8_t* three_lgs, const double h[2],
                      double wind_speed, int npsflin, int nl, const double* lbda_nm,
                      const uint8_t* mask_rec, const uint8_t* mask_res, double* psf_out,
                      double* psf_sum_out, double* fit_out, int on_device) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    CallArgs a = pipeline_args(ntask, seeing, gl, l0, three_lgs, nl, lbda_nm, mask_rec, mask_res, psf_out, psf_sum_out,
                               fit_out, on_device);
    a.h = h, a.wind_speed = wind_speed, a.npsflin = npsflin;
    return guarded_call(c, a);
}

int mpsfr_reconstruct_field(mpsfr_ctx* c, int ntask, const double* seeing, const double* gl,
                            const double* l0, const uint8_t* three_lgs, const double h[2],
                            double wind_speed, int npos, const double* pos_arcsec,
                            int nl, const double* lbda_nm, const uint8_t* mask_rec,
                            const uint8_t* mask_res, double* psf_out, double* psf_sum_out,
                            double* fit_out, int on_device) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    StageIO io;
    CallArgs a = pipeline_args(ntask, seeing, gl, l0, three_lgs, nl, lbda_nm, mask_rec, mask_res, psf_out, psf_sum_out,
                               fit_out, on_device);
    a.npsflin = 0;
    if (int rc = grid_or_positions(1, npos, pos_arcsec, a.npsflin, io)) return rc;
    a.h = h, a.wind_speed = wind_speed;
    return guarded_call(c, a, io);
}

static_assert(MAX_BANDS == MPSFR_MAX_BANDS, "K_BAND_REDUCE keeps MPSFR_MAX_BANDS accumulators");

int mpsfr_reconstruct_band(mpsfr_ctx* c, int ntask, const double* seeing, const double* gl, const double* l0,
                           const uint8_t* three_lgs, const double h[2], double wind_speed, int npsflin, int npos,
                           const double* pos_arcsec, int nl, const double* lbda_nm, int nband, const double* weights,
                           const uint8_t* mask_rec, const uint8_t* mask_res, double* band_out, double* band_sum_out,
                           double* band_fit_out, int on_device) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    if (nband < 1 || nband > MPSFR_MAX_BANDS) return fail(MPSFR_E_INVALID, "nband=%d out of range 1..%d", nband, MPSFR_MAX_BANDS);
    if (nl < 1 || nl > 4096) return fail(MPSFR_E_INVALID, "nl=%d out of range", nl);
    if (!weights) return fail(MPSFR_E_INVALID, "weights is NULL");
    // every band normalised to sum 1 (a power-of-two scale of a band's weights leaves them bit for bit as they are)
    std::vector<double> w((size_t)nband * nl);
    for (int b = 0; b < nband; ++b) {
        const double* r = weights + (size_t)b * nl;
        double sum = 0.0;
        for (int l = 0; l < nl; ++l) {
            if (!std::isfinite(r[l]) || r[l] < 0.0) return fail(MPSFR_E_INVALID, "band %d: weight %d must be finite and >= 0", b, l);
            sum += r[l];
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail(MPSFR_E_INVALID, "band %d: the weights sum to %g", b, sum);
        for (int l = 0; l < nl; ++l) w[(size_t)b * nl + l] = r[l] / sum;
    }
    StageIO io;
    io.nband = nband;
    io.bw = w.data();
    CallArgs a = pipeline_args(ntask, seeing, gl, l0, three_lgs, nl, lbda_nm, mask_rec, mask_res, band_out, band_sum_out,
                               band_fit_out, on_device);
    a.npsflin = npsflin;
    if (int rc = grid_or_positions(0, npos, pos_arcsec, a.npsflin, io)) return rc;
    a.h = h, a.wind_speed = wind_speed;
    return guarded_call(c, a, io);
}

static_assert(MAXLAYER == MPSFR_MAX_LAYERS, "AoLayers holds MPSFR_MAX_LAYERS layers");

// The checks of a profile call, before anything is queued: the layers (1..MAXLAYER, finite, 0 <= h <= 50 km,
// 0 <= speed <= 100 m/s) and the rows' weights (finite, >= 0, a positive sum).  Fills `ly` (winds psfrec.py:594) and
// `w` [ntask][ly.n] with the layers that carry weight in some row: a layer of weight 0 in every row contributes
// nothing, and leaving it out keeps the tables, their cache key and the order of the mixing sum those of the
// profile without it (bit for bit).
static int profile_layers(int ntask, int nlayer, const double* h, const double* wind_speed, const double* wind_dir,
                          const double* cn2, AoLayers& ly, std::vector<double>& w) {
    if (nlayer < 1 || nlayer > MPSFR_MAX_LAYERS) return fail(MPSFR_E_INVALID, "nlayer=%d out of range 1..%d", nlayer, MPSFR_MAX_LAYERS);
    if (!h || !wind_speed || !wind_dir || !cn2) return fail(MPSFR_E_INVALID, "NULL profile array");
    memset(&ly, 0, sizeof ly);
    ly.n = nlayer;
    ly.ntab = ao_ntab(nlayer);
    for (int l = 0; l < nlayer; ++l) {
        if (!std::isfinite(h[l]) || !std::isfinite(wind_speed[l]) || !std::isfinite(wind_dir[l]))
            return fail(MPSFR_E_INVALID, "layer %d: non-finite altitude or wind", l);
        if (h[l] < 0.0 || h[l] > 50000.0) return fail(MPSFR_E_INVALID, "layer %d: h=%g outside [0, 50000] m", l, h[l]);
        if (wind_speed[l] < 0.0 || wind_speed[l] > 100.0)
            return fail(MPSFR_E_INVALID, "layer %d: wind speed %g outside [0, 100] m/s", l, wind_speed[l]);
        ly.h[l] = h[l];
        ly.wind[0][l] = wind_speed[l] * std::cos(wind_dir[l]);
        ly.wind[1][l] = wind_speed[l] * std::sin(wind_dir[l]);
    }
    for (int t = 0; t < ntask; ++t) {
        double sum = 0.0;
        for (int l = 0; l < nlayer; ++l) {
            const double w = cn2[(size_t)t * nlayer + l];
            if (!std::isfinite(w) || w < 0.0) return fail(MPSFR_E_INVALID, "row %d: weight %d must be finite and >= 0", t, l);
            sum += w;
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail(MPSFR_E_INVALID, "row %d: the weights sum to %g", t, sum);
    }
    int keep[MAXLAYER], nk = 0;
    for (int l = 0; l < nlayer; ++l) {
        bool used = false;
        for (int t = 0; t < ntask && !used; ++t) used = cn2[(size_t)t * nlayer + l] != 0.0;
        if (used) keep[nk++] = l;
    }
    for (int k = 0; k < nk; ++k) {
        ly.h[k] = ly.h[keep[k]];
        ly.wind[0][k] = ly.wind[0][keep[k]];
        ly.wind[1][k] = ly.wind[1][keep[k]];
    }
    for (int k = nk; k < MAXLAYER; ++k) ly.h[k] = ly.wind[0][k] = ly.wind[1][k] = 0.0;
    ly.n = nk;
    ly.ntab = ao_ntab(nk);
    w.resize((size_t)ntask * nk);
    for (int t = 0; t < ntask; ++t)
        for (int k = 0; k < nk; ++k) w[(size_t)t * nk + k] = cn2[(size_t)t * nlayer + keep[k]];
    return MPSFR_OK;
}

static const double kNoH[2] = {0.0, 0.0};     // h of a profile call: the layers come from StageIO

int mpsfr_reconstruct_profile(mpsfr_ctx* c, int ntask, const double* seeing, const double* gl,
                              const double* l0, const uint8_t* three_lgs,
                              int nlayer, const double* h, const double* wind_speed, const double* wind_dir,
                              const double* cn2, int npsflin, int npos, const double* pos_arcsec,
                              int nl, const double* lbda_nm, const uint8_t* mask_rec, const uint8_t* mask_res,
                              double* psf_out, double* psf_sum_out, double* fit_out, int on_device) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    if (ntask < 1) return fail(MPSFR_E_INVALID, "ntask < 1");
    AoLayers ly;
    std::vector<double> w;
    if (int rc = profile_layers(ntask, nlayer, h, wind_speed, wind_dir, cn2, ly, w)) return rc;
    StageIO io;
    io.layers = &ly;
    io.cn2 = w.data();
    CallArgs a = pipeline_args(ntask, seeing, gl, l0, three_lgs, nl, lbda_nm, mask_rec, mask_res, psf_out, psf_sum_out,
                               fit_out, on_device);
    a.npsflin = npsflin;
    if (int rc = grid_or_positions(0, npos, pos_arcsec, a.npsflin, io)) return rc;
    a.h = kNoH, a.wind_speed = 0.0;
    return guarded_call(c, a, io);
}

int mpsfr_simul_psd_profile(mpsfr_ctx* c, double seeing, double l0, int three_lgs,
                            int nlayer, const double* h, const double* wind_speed, const double* wind_dir,
                            const double* cn2, int npsflin, int npos, const double* pos_arcsec,
                            const uint8_t* mask_rec, const uint8_t* mask_res, double* psd_out) {
    if (!c || !psd_out) return fail(MPSFR_E_INVALID, "NULL argument");
    AoLayers ly;
    std::vector<double> w;
    if (int rc = profile_layers(1, nlayer, h, wind_speed, wind_dir, cn2, ly, w)) return rc;
    StageIO io;
    io.layers = &ly;
    io.cn2 = w.data();
    CallArgs a;
    a.npsflin = npsflin;
    // (with positions, the PSD of each position: stage A's directions are the positions, as in a field call)
    if (int rc = grid_or_positions(0, npos, pos_arcsec, a.npsflin, io)) return rc;
    const uint8_t t3 = three_lgs ? 1 : 0;
    a.seeing = &seeing, a.l0 = &l0, a.three_lgs = &t3;
    a.h = kNoH, a.wind_speed = 0.0;
    a.mask_rec = mask_rec, a.mask_res = mask_res;
    return guarded(c, [&] { return simul_psd_impl(c, a, io, psd_out); });
}

// ===== The call path on the host ("The call path on the host").  Three kinds of steps, kept apart:
//   preparation   pure host arithmetic on the arguments; takes the context const, makes no HIP call and is the only
//                 place a call is refused for its arguments -- so a refused call has touched nothing;
//   context steps ticket, lanes, slot, waits, cached tables, workspaces, the call's end: they change context state
//                 and may queue waits, copies and table kernels;
//   chunk stages  stage A, stage B and the tail of one chunk on one lane: kernel launches only.

// ---- preparation

// The pruning and tier thresholds of the per-wavelength stage
struct Thresholds {
    bool prune = false;            // trailing OTF lines below eps of the PSF peak are neither transformed nor read
    bool floor_per_task = false;   // the kernel for several directions takes a per-task floor from K_PEAK_FLOOR
    float thr_sum = 0.f, thr_blk = 0.f, thr_eps = 0.f, thr_floor = -1.0e30f, thr_mid = -1.0e30f, tier_half = 0.f;
    float c2min = 0.f;             // log2-scaled exponent factor of the shortest wavelength (the most negative)
};

// What a call computes from its arguments before it touches the context: the shape, the paths its stages take, the
// scalars of its rows and wavelengths.  Later steps only read it.
struct CallPrep {
    int ntask = 0, nl = 0, N = 0, H1 = 0;
    // ndir: the directions stage A evaluates per task.  Stage B sums ndb of them into a stamp, for gpp stamp groups
    // per task: the averaged call (ndb = ndir, gpp = 1) or the field call (ndb = 1, gpp = npos: group g of a chunk is
    // task g / npos at position g % npos, and every stage-B kernel sees tc x npos one-direction tasks)
    int ndir = 0, gpp = 1, ndb = 0;
    // a band call: nout = nband output planes per stamp group (else the nl wavelengths); nsum = gpp x nout planes of
    // a task: the sums run over the tasks of [task][nsum] stamps
    int nout = 0, nsum = 0;
    bool band = false;
    const double* bw = nullptr;          // [nband][nl] the normalised weights of a band call
    const AoLayers* ly = nullptr;        // a profile call
    int ntab = 2, low = 0;               // layer tables per direction; the lowest layer
    bool series = false;                 // stage A in its series + patch form (stage_a2.hip)
    bool fft_conv = true;                // convolutions through 64-point FFTs (f64 mode: the same transforms in fp64)
    size_t ksz = 0;                      // bytes of one convolution kernel (spectrum or taps)
    bool mf = false, mf2 = false, r16 = false;   // stage B: matrix cores, its thin-wave kernel; the radix-16 row pass
    Thresholds th;
    AoGeom g;
    std::vector<LamPar> lp;              // [nl]
    std::vector<TaskPar> tp;             // [ntask]
    std::vector<double> gam, alp;        // [ntask + nl] Moffat widths and exponents: tip-tilt kernels, instrument kernels
    std::vector<double> wts;             // [ntask][ntab] profile weights, each row normalised
};

// The argument checks every driver shares, and the shape integers
static int call_shape(const mpsfr_ctx* c, const CallArgs& a, const StageIO& io, CallPrep& p) {
    if (a.ntask < 1 || !a.seeing || !a.gl || !a.l0 || !a.h || !a.lbda_nm)
        return fail(MPSFR_E_INVALID, "ntask < 1 or NULL input array");
    if (a.nl < 1 || a.nl > 4096) return fail(MPSFR_E_INVALID, "nl=%d out of range", a.nl);
    const bool field = io.npos > 0;
    if (field && !io.pos) return fail(MPSFR_E_INVALID, "field call without positions");
    if (!field && (a.npsflin < 1 || a.npsflin > 5)) return fail(MPSFR_E_INVALID, "npsflin=%d out of range 1..5", a.npsflin);
    if ((a.mask_rec == nullptr) != (a.mask_res == nullptr))
        return fail(MPSFR_E_INVALID, "mask_rec and mask_res must both be given or both be NULL");
    p.band = io.nband > 0;
    if (p.band && (!io.bw || io.nband > MAX_BANDS)) return fail(MPSFR_E_INVALID, "bad band request");
    p.ntask = a.ntask, p.nl = a.nl, p.N = c->N, p.H1 = c->N / 2 + 1;
    p.ndir = field ? io.npos : a.npsflin * a.npsflin;
    p.gpp = field ? p.ndir : 1;
    p.ndb = field ? 1 : p.ndir;
    p.nout = p.band ? io.nband : a.nl;
    p.nsum = p.gpp * p.nout;
    p.bw = io.bw;
    p.fft_conv = c->fft_conv;
    p.ksz = p.fft_conv ? (size_t)KHAT * 2 * rsize(c) : (size_t)KS * KS * rsize(c);
    return MPSFR_OK;
}

// Per-wavelength scalars (psfrec.py:662-665, 717).  cropped: the call crops the OTF at npixc, which must fit the grid.
static int wavelength_scalars(const mpsfr_ctx* c, const CallArgs& a, bool cropped, CallPrep& p) {
    p.lp.resize(a.nl);
    for (int l = 0; l < a.nl; ++l) {
        if (!(a.lbda_nm[l] > 0.0)) return fail(MPSFR_E_INVALID, "lbda[%d] must be > 0", l);
        const double k = 2.0 * M_PI / a.lbda_nm[l];
        p.lp[l].c = -0.5 * k * k;
        p.lp[l].npixc = npix_crop(a.lbda_nm[l], c->dimpsf, c->pixscale);
        p.lp[l].pad = 0;
        if (cropped && (p.lp[l].npixc > c->N || p.lp[l].npixc < NS))
            return fail(MPSFR_E_GRID,
                        "lbda=%.3f nm needs a %d-pixel crop, outside [%d, dim=%d] "
                        "(psfrec.py:663-683)", a.lbda_nm[l], p.lp[l].npixc, NS, c->N);
    }
    return MPSFR_OK;
}

// Per-task scalars (psfrec.py:57-58, 108, 183-187), the weights of a profile call -- every row normalised to sum 1
// (psfrec.py:57-58), padded to ntab with zeros -- and the Moffat parameters of the tip-tilt and instrument kernels.
// Decides the form of stage A: the series form needs every 1/L0^2 inside the radius of its expansion (L0 >= 7 m; the
// SPARTA front end only lets 8 < L0 < 30 through, psfrec.py:1049-1051); a call with a shorter outer scale takes the
// full-size transforms.
static int task_scalars(const mpsfr_ctx* c, const CallArgs& a, const StageIO& io, CallPrep& p) {
    const int ntask = a.ntask, nl = a.nl;
    p.ly = io.layers;
    p.ntab = p.ly ? p.ly->ntab : 2;
    p.low = 0;
    if (p.ly) {
        if (!io.cn2) return fail(MPSFR_E_INVALID, "profile call without weights");
        p.wts.assign((size_t)ntask * p.ntab, 0.0);
        for (int l = 1; l < p.ly->n; ++l)
            if (p.ly->h[l] < p.ly->h[p.low]) p.low = l;
        for (int t = 0; t < ntask; ++t) {
            const double* r = io.cn2 + (size_t)t * p.ly->n;
            double sum = 0.0;
            for (int l = 0; l < p.ly->n; ++l) sum += r[l];
            for (int l = 0; l < p.ly->n; ++l) p.wts[(size_t)t * p.ntab + l] = r[l] / sum;
        }
    }
    p.tp.resize(ntask);
    p.gam.resize((size_t)ntask + nl);
    p.alp.resize((size_t)ntask + nl);
    for (int t = 0; t < ntask; ++t) {
        if (!(a.seeing[t] > 0.0) || !(a.l0[t] > 0.0) || !(a.gl[t] >= 0.0) || !(a.gl[t] <= 1.0))
            return fail(MPSFR_E_INVALID, "task %d: need seeing > 0, L0 > 0, 0 <= GL <= 1", t);
        const double r0 = 0.976 * 0.5 / a.seeing[t] / 4.85;
        double c0 = a.gl[t], c1 = 1.0 - a.gl[t];
        const double cs = c0 + c1;
        c0 /= cs;
        c1 /= cs;
        TaskPar& tp = p.tp[t];
        tp.r0m53 = std::pow(r0, -5.0 / 3.0);
        tp.inv_l0sq = (1.0 / a.l0[t]) * (1.0 / a.l0[t]);
        tp.cn2_0 = c0;
        tp.cn2_1 = c1;
        if (p.ly) {    // (the kernels read the weights; cn2_1 only orders the tasks: the weight above the lowest layer)
            tp.cn2_0 = p.wts[(size_t)t * p.ntab + p.low];
            tp.cn2_1 = 1.0 - tp.cn2_0;
        }
        tp.geom = (a.three_lgs && a.three_lgs[t]) ? 1 : 0;
        tp.basis = 0;
        p.gam[t] = tiptilt_alpha(a.seeing[t], a.gl[t], a.l0[t], c->pixscale);
        p.alp[t] = 2.0;                                    // beta_tt, psfrec.py:879
    }
    for (int l = 0; l < nl; ++l) muse_kernel_params(a.lbda_nm[l], c->pixscale, &p.gam[ntask + l], &p.alp[ntask + l]);
    p.series = c->stage_a == 2 || (c->stage_a == 1 && (p.N >= 512 || (p.N >= 256 && p.ndir >= 2)));
    for (int t = 0; t < ntask; ++t) p.series = p.series && p.tp[t].inv_l0sq <= series_eps_max();
    return MPSFR_OK;
}

// Geometry of the AO tables (psfrec.py:61, 66, 86-93, 99, 154-158, 536-537, 594)
static AoGeom ao_geometry(const CallArgs& a, const StageIO& io, int ndir) {
    AoGeom g;
    memset(&g, 0, sizeof g);
    g.h[0] = a.h[0];
    g.h[1] = a.h[1];
    const double arg_v[2] = {0.628163, -0.326497};
    for (int l = 0; l < 2; ++l) {
        g.wind[0][l] = a.wind_speed * std::cos(arg_v[l]);
        g.wind[1][l] = a.wind_speed * std::sin(arg_v[l]);
    }
    const double pos4[4][2] = {{1, 1}, {-1, -1}, {-1, 1}, {1, -1}};
    g.nlgs[0] = 4;
    g.nlgs[1] = 3;
    for (int ge = 0; ge < 2; ++ge)
        for (int q = 0; q < g.nlgs[ge]; ++q) {
            g.poslgs[ge][0][q] = pos4[q][0] * 63.0 / 60;
            g.poslgs[ge][1][q] = pos4[q][1] * 63.0 / 60;
        }
    g.ndir = ndir;
    const int npsflin = a.npsflin;
    for (int d = 0; d < ndir; ++d) {
        if (io.npos > 0) {              // (the convention of direction_perf: x = dirperf[0], in arcmin here)
            g.dir[0][d] = io.pos[2 * d] / 60;
            g.dir[1][d] = io.pos[2 * d + 1] / 60;
        } else {
            g.dir[0][d] = (double)(d / npsflin - npsflin / 2) * 60 / 2 / 60;
            g.dir[1][d] = (double)(d % npsflin - npsflin / 2) * 60 / 2 / 60;
        }
    }
    return g;
}

// The paths of stage B and its thresholds.
// Line pruning of the per-wavelength stage (mixed mode): the trailing lines of the OTF half plane that together
// weigh less than eps of the PSF peak are neither transformed nor read by the second pass (stage_a.hip, "Line
// pruning").  Matrix-core path: half of eps for the lines, half for the 16 x 32 blocks inside them (every element of
// a dropped block is below 2^thr_blk; both half planes, all directions; ndb: the directions one stamp sums -- a field
// stamp has one, and the whole budget).
// Precision tiers of the matrix-core stage.  The OTF is generated times 2^15, so an element
// below 2^-29 of OTF[0][0] has both fp16 halves in the subnormal range: a block whose bound is below
// 2^-29.01 carries a few bits per element and is dropped ("floor"); a block below 2^-18.01 runs without
// the low half ("mid").  Both are approximations (the matrix cores do not flush subnormals), held to a
// budget: per (task, wavelength) the OTF mass each tier leaves out -- an upper bound from the block bounds --
// stays below tier_eps / 2 of a lower bound of the PSF peak; K_MF_PREP lowers the thresholds where it
// would not.  The kernel for several directions (otf_mfma.hip) has no such pass: its floor is the
// per-task floor from K_PEAK_FLOOR (the same budget against the OTF of the shortest wavelength, blocks counted).
static void stage_b_paths(const mpsfr_ctx* c, CallPrep& p) {
    const int N = p.N, ndb = p.ndb;
    // per-wavelength stage on the matrix cores (otf_mfma = 0: LDS FFTs on the vector pipe)
    p.mf = !c->f64 && c->otf_mfma;
    p.mf2 = p.mf && ndb == 1 && c->mf_kernel == 2;       // thin-wave kernel (otf_mfma2.hip)
    p.r16 = !p.mf && otf_uses_r16(N, c->f64, p.nl, ndb);
    Thresholds& th = p.th;
    const double eps_prune = c->f64 ? c->prune_eps_f64 : c->prune_eps;
    th.prune = eps_prune > 0.0;
    th.thr_sum = th.prune ? (float)((p.mf ? 0.5 : 1.0) * eps_prune / (2.0 * N * ndb)) : 0.f;
    th.thr_blk = (th.prune && p.mf)
        ? (float)std::log2(0.5 * eps_prune / (2.0 * ndb * 16 * 32 * mf_block_count(N))) : 0.f;
    th.thr_eps = th.thr_blk;
    th.thr_floor = -1.0e30f;
    const bool tiers = th.prune && p.mf && c->tier_eps > 0.0;
    th.floor_per_task = tiers && c->mf_floor && !p.mf2 && std::isfinite(c->tier_eps);
    if (tiers && c->mf_floor) {
        th.thr_floor = (float)c->mf_floor_log2;
        // tier_eps = inf: the plain floor
        if (!p.mf2 && !th.floor_per_task && th.thr_blk < th.thr_floor) th.thr_blk = th.thr_floor;
    }
    th.c2min = 0.f;
    for (int l = 0; l < p.nl; ++l) th.c2min = std::fmin(th.c2min, (float)(p.lp[l].c * 1.44269504088896340736));
    th.thr_mid = (tiers && c->mf_floor) ? (float)c->mf_mid_log2 : -1.0e30f;
    th.tier_half = std::isfinite(c->tier_eps) ? (float)(0.5 * c->tier_eps) : 0.f;
}

// Everything a pipeline call computes from its arguments, and every refusal for them
static int prepare_call(const mpsfr_ctx* c, const CallArgs& a, const StageIO& io, CallPrep& p) {
    if (int rc = call_shape(c, a, io, p)) return rc;
    if (int rc = wavelength_scalars(c, a, true, p)) return rc;
    if (int rc = task_scalars(c, a, io, p)) return rc;
    p.g = ao_geometry(a, io, p.ndir);
    stage_b_paths(c, p);
    return MPSFR_OK;
}

// Tasks per pipeline pass of a call that does not set "chunk_tasks".  spt: stamps per task; ws_per_task: bytes of
// the largest workspace a task takes (0: none that counts); alone: the call has no neighbour call on another lane.
// One chunk as long as it fits: up to 512 tasks (65536 stamps) and 4 GiB of that workspace.  Beyond that,
// balanced chunks, a multiple of the lane count of them.  (The chunks used to be cut at ~4096
// stamps, "enough to fill the GPU": a 125-row call then ran as 118 + 7 rows and reached 9.8 M
// PSFs/s where one chunk reaches 14.6 M; 250 rows 11.3 -> 15.3 M, 1000 rows 14.5 -> 15.1 M.)
static int auto_chunk_tasks(int ntask, int spt, double ws_per_task, int nlanes, bool alone) {
    int big = 65536 / spt;
    const int soft = (4096 + spt - 1) / spt < 8 ? 8 : (4096 + spt - 1) / spt;
    if (big > 512) big = 512;
    if (big < soft) big = soft;
    if (ws_per_task > 0.0) {
        const int cap = (int)(4.0 * 1024 * 1024 * 1024 / ws_per_task);
        if (big > cap) big = cap < 1 ? 1 : cap;
    }
    int nch = (ntask + big - 1) / big;
    if (nch > 1) nch = (nch + nlanes - 1) / nlanes * nlanes;
    // A synchronous call (host outputs, or pipelining off) has no neighbour call on the other lane:
    // from 8192 stamps on, one pass per lane overlaps the stages of the halves (250 rows x 35
    // wavelengths at 512^2: 0.78 -> 0.75 ms per call; 100 rows: 0.42 either way; four passes lose).
    if (nch == 1 && nlanes > 1 && (long)ntask * spt >= 8192 && alone) nch = nlanes;
    return (ntask + nch - 1) / nch;
}

// ... of a call through stages A and B (stamps per task: gpp x nl, and the band stamps of a band call; the largest
// workspace per task: the row transforms C of the full-size form; D and the patch transforms of the series form)
static int pipeline_chunk_tasks(const mpsfr_ctx* c, const CallPrep& p, bool alone) {
    if (c->chunk_tasks > 0) return c->chunk_tasks;
    const int spt = p.gpp * p.nl + (p.band ? p.gpp * p.nout : 0);
    const double ws = p.series ? (double)p.ndir * p.H1 * (p.N * (double)rsize(c) + kNH * 16.0)
                               : (double)p.ndir * (p.N / 2 + NAO / 2) * p.H1 * 16.0;
    return auto_chunk_tasks(p.ntask, spt, ws, c->nlanes == 0 ? 2 : c->nlanes, alone);
}

// The AO tables are cached on their inputs (geometry + cut-off masks): the masks -- 12.8 KB of the ~20 KB a call used
// to upload -- only travel with a call that rebuilds the tables.  A profile call: the key holds the whole profile
// too -- layers, altitudes, winds -- behind a byte that tells it from a legacy key.
static std::vector<unsigned char> ao_cache_key(const AoGeom& g, const AoLayers* ly, const uint8_t* mask_rec,
                                               const uint8_t* mask_res) {
    const size_t ko = sizeof(AoGeom) + 1 + (ly ? sizeof(AoLayers) : 0);
    std::vector<unsigned char> key(ko + 1 + (mask_rec ? 2 * NAO * NAO : 0));
    memcpy(key.data(), &g, sizeof(AoGeom));
    key[sizeof(AoGeom)] = ly ? 1 : 0;
    if (ly) {
        AoLayers lk;                     // (a copy without padding garbage: the key compares bytes)
        memset(&lk, 0, sizeof lk);
        lk.n = ly->n;
        lk.ntab = ly->ntab;
        for (int l = 0; l < ly->n; ++l) {
            lk.h[l] = ly->h[l];
            lk.wind[0][l] = ly->wind[0][l];
            lk.wind[1][l] = ly->wind[1][l];
        }
        memcpy(key.data() + sizeof(AoGeom) + 1, &lk, sizeof lk);
    }
    key[ko] = mask_rec ? 1 : 0;
    if (mask_rec) {
        memcpy(key.data() + ko + 1, mask_rec, NAO * NAO);
        memcpy(key.data() + ko + 1 + NAO * NAO, mask_res, NAO * NAO);
    }
    return key;
}

// The device views of a call's parameter blob, and what else the kernels of a chunk read from its slot
struct DevParams {
    const LamPar* lp = nullptr;
    const TaskPar* tp = nullptr;
    const double *gam = nullptr, *alp = nullptr, *w = nullptr, *bw = nullptr;
    const uint8_t *mrec = nullptr, *mres = nullptr;     // (read by K_AO_TABLES only)
    int ntab = 2;
    const char* ktt = nullptr;           // [ntask] tip-tilt kernels of the call (spectra or taps), ksz bytes each
    LayerMix mix(int t0) const {
        LayerMix m;
        m.w = w ? w + (size_t)t0 * ntab : nullptr;
        m.ntab = ntab;
        return m;
    }
};

// The small per-call parameters: one pinned blob [LamPar nl][TaskPar ntask][gam][alp]([mask_rec][mask_res])
// ([profile weights])([band weights])
struct Blob {
    size_t o_lp, o_tp, o_gam, o_alp, o_mr, o_ms, o_w, o_bw, bytes;
    int bstride;                         // a band call: its weights [nl][band_stride(nband)], zero beyond nband
    bool masks;
    static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
    Blob(const CallPrep& p, bool send_masks) : masks(send_masks) {
        o_lp = 0;
        o_tp = al16(o_lp + p.nl * sizeof(LamPar));
        o_gam = al16(o_tp + p.ntask * sizeof(TaskPar));
        o_alp = al16(o_gam + p.gam.size() * sizeof(double));
        o_mr = al16(o_alp + p.alp.size() * sizeof(double));
        o_ms = al16(o_mr + (masks ? NAO * NAO : 0));
        o_w = al16(o_ms + (masks ? NAO * NAO : 0));
        bstride = p.band ? band_stride(p.nout) : 0;
        o_bw = al16(o_w + p.wts.size() * sizeof(double));
        bytes = al16(o_bw + (size_t)p.nl * bstride * sizeof(double));
    }
    void fill(void* host, const CallPrep& p, const uint8_t* mask_rec, const uint8_t* mask_res) const {
        char* hb = (char*)host;
        memcpy(hb + o_lp, p.lp.data(), p.nl * sizeof(LamPar));
        memcpy(hb + o_tp, p.tp.data(), p.ntask * sizeof(TaskPar));
        memcpy(hb + o_gam, p.gam.data(), p.gam.size() * sizeof(double));
        memcpy(hb + o_alp, p.alp.data(), p.alp.size() * sizeof(double));
        if (p.ly) memcpy(hb + o_w, p.wts.data(), p.wts.size() * sizeof(double));
        if (p.band) {
            double* bw = reinterpret_cast<double*>(hb + o_bw);
            for (int l = 0; l < p.nl; ++l)
                for (int b = 0; b < bstride; ++b) bw[(size_t)l * bstride + b] = b < p.nout ? p.bw[(size_t)b * p.nl + l] : 0.0;
        }
        if (masks) {
            memcpy(hb + o_mr, mask_rec, NAO * NAO);
            memcpy(hb + o_ms, mask_res, NAO * NAO);
        }
    }
    DevParams views(const mpsfr_ctx::Slot& sl, const CallPrep& p) const {
        const char* db = (const char*)sl.params.p;
        DevParams d;
        d.lp = (const LamPar*)(db + o_lp);
        d.tp = (const TaskPar*)(db + o_tp);
        d.gam = (const double*)(db + o_gam);
        d.alp = (const double*)(db + o_alp);
        d.w = p.ly ? (const double*)(db + o_w) : nullptr;
        d.bw = p.band ? (const double*)(db + o_bw) : nullptr;
        d.mrec = masks ? (const uint8_t*)(db + o_mr) : nullptr;
        d.mres = masks ? (const uint8_t*)(db + o_ms) : nullptr;
        d.ntab = p.ntab;
        d.ktt = (const char*)sl.ktt.p;
        return d;
    }
};

// ---- context steps

// Host cost of queueing a call: the wall time inside it, not the time spent waiting for the GPU to catch up
struct HostClock {
    std::chrono::steady_clock::time_point enter = std::chrono::steady_clock::now();
    double blocked = 0.0;
    void finish(mpsfr_ctx* c) const {
        c->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - enter).count() - blocked;
        c->host_calls += 1;
    }
};

// Where a call's results go: the caller's pointers (host or device), or the result set of a ticket
struct CallOuts {
    double *psf = nullptr, *sum = nullptr, *fit = nullptr;
    bool dev = false;                    // they are device buffers
    // where the chunks write: d_fin_all [ntask][nsum][1600] if the stamps go straight to a device buffer (else the
    // lanes' workspaces), the fits of the whole call, the stamp sum
    double *d_fin_all = nullptr, *d_fit_all = nullptr, *d_sum = nullptr;
};

// Asynchronous host outputs: the call writes a result set of the ring and is, from here on, a device-output call;
// ticket_finish then copies the set to its pinned mirror on the join stream
static int ticket_begin(mpsfr_ctx* c, const CallPrep& p, CallOuts& o, mpsfr_ctx::Ticket*& out) {
    int rc;
    mpsfr_ctx::Ticket* tk = &c->ticket[c->ticket_next % mpsfr_ctx::NTICKET];
    if ((rc = complete_ticket(c, *tk))) return rc;         // NTICKET calls ago: hand it over first
    tk->u_psf = o.psf;
    tk->u_sum = o.sum;
    tk->u_fit = o.fit;
    tk->n_psf = o.psf ? (size_t)p.ntask * p.nsum * NS * NS : 0;
    tk->n_sum = o.sum ? (size_t)p.nsum * NS * NS : 0;
    tk->n_fit = o.fit ? (size_t)p.ntask * p.nsum * NFIT : 0;
    const size_t hb = (tk->n_psf + tk->n_sum + tk->n_fit) * sizeof(double);
    if (hb > tk->host_cap) {
        if (tk->host) HIPCHK(hipHostFree(tk->host));
        tk->host = nullptr;
        tk->host_cap = 0;
        HIPCHK(hipHostMalloc(&tk->host, hb + hb / 8, hipHostMallocDefault));
        tk->host_cap = hb + hb / 8;
    }
    if (tk->n_psf && (rc = ensure(c, tk->dpsf, tk->n_psf * sizeof(double)))) return rc;
    if (tk->n_sum && (rc = ensure(c, tk->dsum, tk->n_sum * sizeof(double)))) return rc;
    if (tk->n_fit && (rc = ensure(c, tk->dfit, tk->n_fit * sizeof(double)))) return rc;
    if (!tk->done) HIPCHK(hipEventCreateWithFlags(&tk->done, hipEventDisableTiming));
    o.psf = tk->n_psf ? (double*)tk->dpsf.p : nullptr;
    o.sum = tk->n_sum ? (double*)tk->dsum.p : nullptr;
    o.fit = tk->n_fit ? (double*)tk->dfit.p : nullptr;
    o.dev = true;
    out = tk;
    return MPSFR_OK;
}

static int ticket_finish(mpsfr_ctx* c, mpsfr_ctx::Ticket* tk) {
    hipStream_t s = c->stream;
    double* h = (double*)tk->host;
    if (tk->n_psf) HIPCHK(hipMemcpyAsync(h, tk->dpsf.p, tk->n_psf * sizeof(double), hipMemcpyDeviceToHost, s));
    if (tk->n_sum) HIPCHK(hipMemcpyAsync(h + tk->n_psf, tk->dsum.p, tk->n_sum * sizeof(double), hipMemcpyDeviceToHost, s));
    if (tk->n_fit)
        HIPCHK(hipMemcpyAsync(h + tk->n_psf + tk->n_sum, tk->dfit.p, tk->n_fit * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(tk->done, s));
    tk->id = c->ticket_next++;
    tk->pending = true;
    return MPSFR_OK;
}

// The lanes of a call.  Consecutive chunks go to successive lanes (HIP streams with their own workspaces); the
// rotation carries over from call to call, so back-to-back asynchronous calls overlap like the chunks of one call do
// (+20 % PSFs/s on the 100-row bench step, +13 % inside a 1000-row call).
struct CallLanes {
    int NLmax = 2;       // lanes of the context
    int TC = 1;          // tasks per chunk
    int nchunks = 1;
    int NL = 1;          // lanes this call uses.  Never more than chunks: a lane without a chunk would leave its
                         // partial stamp sum unwritten, and the final sum over lanes would read stale memory
    int first = 0;       // lane of the first chunk
    // Stagger of the lanes at a cold start.  Two lanes that start together -- the first two calls (or
    // chunks) after the GPU has drained -- settle into one of two phase relations, which then persists
    // for as long as the pipeline stays full; on the bench workload (100 rows x 35 wavelengths, 512^2)
    // the one they mostly find from a standing start is the slower (14.1 M PSFs/s against 14.6 M).  So
    // the first chunk after a cold start records an event behind its column transforms and the next
    // chunk on another lane waits for it: a one-time offset of half a stage A, after which the lanes run
    // free.  OFF by default ("cold_stagger" = 1 / 2 switches it on): which relation a one-time offset
    // selects depends on the shape of the call (measured in the sustained run: 100 rows +3 %, 125 rows 0,
    // 250 rows -3 %, 500 rows +2.5 %, 1024^2 -2 %, 1280^2 -1 %), and the offset itself costs a short burst
    // of calls what it gains a long one (20 calls from a standing start: -1 %).
    bool cold_first = false;             // this call found every lane idle: its first chunk records the stagger event
    int index(int j) const { return (first + j) % NLmax; }
    mpsfr_ctx::Lane& at(mpsfr_ctx* c, int j) const { return c->lane[index(j)]; }
};

static bool lane_idle(const mpsfr_ctx::Lane& ln) {
    return (ln.marked ? hipEventQuery(ln.done_ev) : hipStreamQuery(ln.stream)) == hipSuccess;
}

// Takes the call's place in the lane rotation and creates what its lanes lack.  rotate: the call is pipelined with
// its neighbours (a synchronous call has nothing to overlap, and starts on lane 0).
static int lanes_begin(mpsfr_ctx* c, int ntask, int chunk_tasks, bool rotate, CallLanes& L) {
    L.NLmax = c->nlanes == 0 ? 2 : c->nlanes;
    L.TC = chunk_tasks > ntask ? ntask : chunk_tasks;
    L.nchunks = (ntask + L.TC - 1) / L.TC;
    L.NL = L.NLmax < L.nchunks ? L.NLmax : L.nchunks;
    if (!rotate) c->lane_rr = 0;
    L.first = (int)(c->lane_rr % (unsigned)L.NLmax);
    c->lane_rr += (unsigned)L.nchunks;
    for (int j = 0; j < L.NL; ++j) {
        mpsfr_ctx::Lane& ln = L.at(c, j);
        if (!ln.stream) {
            const int li = L.index(j);
            if (c->cu_partition && L.NLmax > 1) {
                // CU-mask bit i is CU i / 8 of XCD i % 8 (the driver deals the bits round the XCDs), so a
                // contiguous range of bits is the same share of every XCD: each lane keeps all eight L2s
                const int lo = c->ncu * li / L.NLmax, hi = c->ncu * (li + 1) / L.NLmax;
                uint32_t mask[16] = {0};
                for (int b = lo; b < hi && b < 512; ++b) mask[b >> 5] |= 1u << (b & 31);
                HIPCHK(hipExtStreamCreateWithCUMask(&ln.stream, (uint32_t)((c->ncu + 31) / 32), mask));
                ln.ncu = hi - lo;
            } else {
                HIPCHK(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
                ln.ncu = 0;
            }
        }
        if (!ln.done) HIPCHK(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
    }
    L.cold_first = false;
    if (c->cold_stagger && L.NLmax > 1) {
        L.cold_first = true;
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
            if (c->lane[k].busy && !lane_idle(c->lane[k])) L.cold_first = false;
        if (!c->stagger_ev) HIPCHK(hipEventCreateWithFlags(&c->stagger_ev, hipEventDisableTiming));
    }
    return MPSFR_OK;
}

// The cold-start stagger at point `which` of a chunk (1: behind the column transforms, 2: behind the preparation of
// the per-wavelength stage): the first chunk of a call that found every lane idle records the event there
static int stagger_here(mpsfr_ctx* c, CallLanes& L, int which, mpsfr_ctx::Lane& ln) {
    if (L.cold_first && c->cold_stagger == which) {
        if (hipEventRecord(c->stagger_ev, ln.stream) != hipSuccess) return fail(MPSFR_E_HIP, "hipEventRecord failed");
        c->stagger_armed = true;
        c->stagger_lane = (int)(&ln - c->lane);
        L.cold_first = false;
    }
    return MPSFR_OK;
}

// ... and the next chunk on another lane waits for it, once
static int stagger_wait(mpsfr_ctx* c, mpsfr_ctx::Lane& ln) {
    if (c->stagger_armed && (int)(&ln - c->lane) != c->stagger_lane) {
        HIPCHK(hipStreamWaitEvent(ln.stream, c->stagger_ev, 0));
        c->stagger_armed = false;
    }
    return MPSFR_OK;
}

// Takes the next slot of the ring -- pinned blob, device blob, tip-tilt kernels -- once the copy that last used the
// pinned blob has left it, and sizes it.  `blocked` receives the time spent waiting for that.
static int slot_acquire(mpsfr_ctx* c, size_t blob, size_t ktt_bytes, mpsfr_ctx::Slot*& out, double& blocked) {
    mpsfr_ctx::Slot& sl = c->slot[c->stage_next++ % mpsfr_ctx::NSTAGE];
    if (sl.staged_pending) {
        const auto tb = std::chrono::steady_clock::now();
        if (sl.staged_mode == 2) {               // (only blocks once the host is NSTAGE calls ahead)
            volatile unsigned long long* flag = c->seq_host + (&sl - c->slot);
            const auto t_lim = tb + std::chrono::seconds(5);
            // (spin briefly -- the flag is usually there: the host is NSTAGE calls ahead -- then yield the core
            // between looks; a failed kernel never writes its flag: after 5 s the lane is synchronised instead)
            for (long spins = 0; *flag < sl.seq; ++spins) {
                if (spins < 4096) {
#if defined(__x86_64__) || defined(__i386__)
                    __builtin_ia32_pause();
#elif defined(__aarch64__)
                    asm volatile("yield" ::: "memory");
#endif
                    continue;
                }
                std::this_thread::yield();
                if ((spins & 255) == 0 && std::chrono::steady_clock::now() > t_lim) {
                    if (sl.last_lane >= 0 && c->lane[sl.last_lane].stream)
                        HIPCHK(hipStreamSynchronize(c->lane[sl.last_lane].stream));
                    else
                        HIPCHK(hipDeviceSynchronize());
                    break;
                }
            }
        } else {
            HIPCHK(hipEventSynchronize(sl.staged_ev));
        }
        blocked = std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count();
        sl.staged_pending = false;
    }
    if (blob > sl.host_cap) {
        if (sl.host) HIPCHK(hipHostFree(sl.host));
        sl.host = nullptr;
        sl.host_cap = 0;
        HIPCHK(hipHostMalloc(&sl.host, blob * 2, hipHostMallocDefault));
        sl.host_cap = blob * 2;
    }
    if (!sl.staged) HIPCHK(hipEventCreateWithFlags(&sl.staged, hipEventDisableTiming));
    if (!sl.call_done) HIPCHK(hipEventCreateWithFlags(&sl.call_done, hipEventDisableTiming));
    int rc;
    if ((rc = ensure(c, sl.params, blob))) return rc;
    if ((rc = ensure(c, sl.ktt, ktt_bytes))) return rc;
    out = &sl;
    return MPSFR_OK;
}

// What the call's lanes must wait for before they touch anything:
//  * the call that used this slot NSTAGE calls ago (device blob, tip-tilt spectra);
//  * an event the caller registered (mpsfr_wait_event);
//  * the most recent call of any other lane that wrote the same output buffers `outs` (a caller that
//    reuses its buffers gets its calls in order);
//  * the previous consumer of the per-lane partial sums.
static int queue_call_waits(mpsfr_ctx* c, const CallLanes& L, mpsfr_ctx::Slot& sl, const void* const outs[3]) {
    // (an event the caller registered that has already happened is no dependency any more)
    if (c->wait_next && hipEventQuery(c->wait_next) == hipSuccess) c->wait_next = nullptr;
    // (the call that used this slot NSTAGE calls ago has usually finished: then no lane waits for it)
    const bool slot_done = sl.call_pending && sl.has_event && hipEventQuery(sl.call_done) == hipSuccess;
    for (int j = 0; j < L.NL; ++j) {
        mpsfr_ctx::Lane& ln = L.at(c, j);
        hipStream_t ls = ln.stream;
        // (a lean call ran on one lane: on that lane stream order suffices; another lane waits for the slot's
        // event, or -- the call queued none -- for the end of that lane as it stands now)
        if (sl.call_pending && !slot_done && sl.last_lane != L.index(j)) {
            if (sl.has_event) HIPCHK(hipStreamWaitEvent(ls, sl.call_done, 0));
            else if (sl.last_lane >= 0) HIPCHK(hipStreamWaitEvent(ls, lane_end(c, c->lane[sl.last_lane]), 0));
        }
        if (c->wait_next) HIPCHK(hipStreamWaitEvent(ls, c->wait_next, 0));
        if (c->lsum_busy && L.NL > 1) HIPCHK(hipStreamWaitEvent(ls, c->lsum_done, 0));
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k) {
            mpsfr_ctx::Lane& o = c->lane[k];
            if (&o == &ln || !o.busy) continue;
            bool same = false;
            for (int hsl = 0; hsl < mpsfr_ctx::Lane::NHIST; ++hsl)
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) same = same || (outs[a] && outs[a] == o.outs[hsl][b]);
            if (same) HIPCHK(hipStreamWaitEvent(ls, lane_end(c, o), 0));
        }
    }
    c->wait_next = nullptr;
    sl.call_pending = false;
    return MPSFR_OK;
}

// How much of the join a call can do without.
// join: everything queued on the lanes becomes a dependency of the context's stream -- if anybody uses that
// stream: a caller that asked for it (mpsfr_stream), the copies of host outputs, the sum over several lanes.
// A device-output call on one lane of a context whose stream was never asked for stays on its lane: this GPU
// runs two active queues well and a third one at a loss (profiles/r05_experiments.md).
// "lean" calls -- device outputs on one lane of a context whose stream nobody uses -- queue NO marker packet
// (a marker is a packet the queue stops at: ~7 us in the kernel trace, and the three of a call -- behind the
// parameter copy, the lane's, the slot's -- were a tenth of a 100-row call): the copy kernel itself tells the
// host, through a pinned word, when the blob may be refilled ("zero"); the slot and the lane get an event only when
// another lane has to wait for them (lane_end).  With the hipMemcpyAsync form of the copy a lean call queues
// one: the slot's event at the end of the lane's chain.
struct Markers {
    bool lean, zero;
    Markers(const mpsfr_ctx* c, bool dev_out, bool ticket, int nlanes) {
        const bool join = c->stream_exported || ticket || !dev_out || nlanes > 1 || !c->pipeline_calls;
        lean = !join;
        zero = lean && c->param_copy_kernel && c->seq_host != nullptr;
    }
};

// Sends the blob of the slot to the device at the head of the call's first lane.  It travels as a KERNEL of the
// call's own queue that reads the pinned host memory: a hipMemcpyAsync of these ~20 KB is a hand-over to a copy
// engine and back, and sat at the head of every call ("param_copy" = 0 brings it back).
static int send_params(mpsfr_ctx* c, mpsfr_ctx::Slot& sl, hipStream_t s0, size_t blob, const Markers& m) {
    sl.seq = ++c->seq_next;
    if (m.zero) {
        launch_param_copy(s0, sl.params.p, sl.host, blob, c->seq_host + (&sl - c->slot), sl.seq);
        sl.staged_mode = 2;
    } else {
        if (c->param_copy_kernel) launch_param_copy(s0, sl.params.p, sl.host, blob, nullptr, 0);
        else HIPCHK(hipMemcpyAsync(sl.params.p, sl.host, blob, hipMemcpyHostToDevice, s0));
        if (m.lean) {
            sl.staged_ev = sl.call_done;
            sl.staged_mode = 1;
        } else {
            HIPCHK(hipEventRecord(sl.staged, s0));
            sl.staged_ev = sl.staged;
            sl.staged_mode = 0;
        }
    }
    sl.staged_pending = true;
    return MPSFR_OK;
}

// ---- cached tables: the AO tables on (geometry, masks, profile), the per-wavelength tables on (wavelengths, form of
// the convolutions, paths of stage B).  Sizing comes first, because a buffer that moved is no cache hit; a stage-level
// call sizes and builds only the tables it reads, and so never displaces the cached ones of the last real call.

static int size_ao_tables(mpsfr_ctx* c, const CallPrep& p, const std::vector<unsigned char>& key, bool& cached) {
    if (int rc = ensure(c, c->aotab, (size_t)2 * p.ndir * (p.ntab + 1) * NAO * NAO * sizeof(double))) return rc;
    cached = key == c->cache_geom && c->cache_ao_ptr == c->aotab.p;
    return MPSFR_OK;
}

static int size_wavelength_tables(mpsfr_ctx* c, const CallPrep& p, const std::vector<double>& lb_key, bool& cached) {
    int rc;
    const int nl = p.nl;
    if ((rc = ensure(c, c->samp_p, (size_t)nl * NS * sizeof(int)))) return rc;
    if ((rc = ensure(c, c->samp_a, (size_t)nl * NS * rsize(c)))) return rc;
    // G rows are padded to a multiple of 8 lines (paired-line layout of the fp32 second pass)
    if ((rc = ensure(c, c->G, (size_t)nl * ((p.H1 + 7) / 8 * 8) * NS * 2 * rsize(c)))) return rc;
    if ((rc = ensure(c, c->kmuse, (size_t)nl * p.ksz))) return rc;
    if (p.r16 && (rc = ensure(c, c->xtab, xtab_bytes(nl)))) return rc;
    if (p.mf) {
        if ((rc = ensure(c, c->etab, mf_etab_bytes(p.N, nl)))) return rc;
        if ((rc = ensure(c, c->gtab, mf_gtab_bytes(p.N, nl)))) return rc;
    }
    cached = lb_key == c->cache_lbda && c->cache_lbda_mode == (p.fft_conv ? 1 : 0) &&
             c->cache_G_ptr == c->G.p && c->cache_kmuse_ptr == c->kmuse.p &&
             (!p.r16 || (c->cache_xtab_valid && c->cache_xtab_ptr == c->xtab.p)) &&
             (!p.mf || (c->cache_mf_valid && c->cache_etab_ptr == c->etab.p && c->cache_gtab_ptr == c->gtab.p));
    return MPSFR_OK;
}

static void build_ao_tables(mpsfr_ctx* c, hipStream_t s0, const CallPrep& p, const DevParams& d,
                            std::vector<unsigned char>& key) {
    ProfScope ps(c, K_AO_TABLES, s0);
    if (p.ly) launch_ao_tables_profile(s0, p.g, *p.ly, d.mrec, d.mres, (double*)c->aotab.p);
    else launch_ao_tables(s0, p.g, d.mrec, d.mres, (double*)c->aotab.p);
    c->cache_geom.swap(key);
    c->last_ntab = p.ntab;
    c->cache_ao_ptr = c->aotab.p;
}

static void build_wavelength_tables(mpsfr_ctx* c, hipStream_t s0, const CallPrep& p, const DevParams& d,
                                    const std::vector<double>& lb_key) {
    const int N = p.N, nl = p.nl;
    {
        ProfScope ps(c, K_GTABLE, s0);
        launch_gtable(s0, N, nl, d.lp, c->tw64.p, (int*)c->samp_p.p, c->samp_a.p, c->G.p, c->f64);
        if (p.r16) launch_xtab(s0, N, nl, (const int*)c->samp_p.p, c->samp_a.p, c->tw64.p, c->xtab.p);
        if (p.mf) launch_mf_tables(s0, N, nl, d.lp, c->tw64.p, c->etab.p, c->gtab.p);
    }
    ProfScope ps(c, K_MOFFAT_KERNELS, s0);
    if (p.fft_conv) launch_khat(s0, nl, d.gam + p.ntask, d.alp + p.ntask, c->kmuse.p, c->f64);
    else launch_moffat_kernels(s0, nl, d.gam + p.ntask, d.alp + p.ntask, c->kmuse.p, c->f64);
    c->cache_lbda = lb_key;
    c->cache_lbda_mode = p.fft_conv ? 1 : 0;
    c->cache_G_ptr = c->G.p;
    c->cache_kmuse_ptr = c->kmuse.p;
    c->cache_xtab_ptr = c->xtab.p;
    c->cache_xtab_valid = p.r16;
    c->cache_etab_ptr = c->etab.p;
    c->cache_gtab_ptr = c->gtab.p;
    c->cache_mf_valid = p.mf;
}

// Rebuilds on s0 the tables whose key is given (ao_key / lb_key: nullptr for a table that is cached, or that the call
// does not read).  A rebuild waits for every lane (an older call may still read the old tables) and is announced by
// `cache_ready`, which every later call's first lane waits for.
static int refresh_tables(mpsfr_ctx* c, hipStream_t s0, const CallPrep& p, const DevParams& d,
                          std::vector<unsigned char>* ao_key, const std::vector<double>* lb_key) {
    if (ao_key || lb_key) {
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
            if (c->lane[k].busy && c->lane[k].stream != s0)
                HIPCHK(hipStreamWaitEvent(s0, lane_end(c, c->lane[k]), 0));
        if (ao_key) build_ao_tables(c, s0, p, d, *ao_key);
        if (lb_key) build_wavelength_tables(c, s0, p, d, *lb_key);
        if (!c->cache_ready) HIPCHK(hipEventCreateWithFlags(&c->cache_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->cache_ready, s0));
        c->cache_ready_valid = true;
    } else if (c->cache_ready_valid) {
        // (once the tables are known to be complete no call has to wait for them any more: a wait on a
        // finished event is still a barrier packet at the head of the call's queue)
        if (hipEventQuery(c->cache_ready) == hipSuccess) c->cache_ready_valid = false;
        else HIPCHK(hipStreamWaitEvent(s0, c->cache_ready, 0));
    }
    return MPSFR_OK;
}

// Tip-tilt kernels of this call's tasks (psfrec.py:879-917) into the slot.  (Measured: moving this small
// launch to a side stream, off the head of the call's chain, and folding the DC sum into
// the column-transform kernel both LOWER the two-lane throughput, by 2-4 %: the short
// serial kernels keep the two lanes out of phase.)
// fused: in the series form of stage A they are extra workgroups of K_PATCH_ROWS, per chunk -- a launch less at the
// head of a call ("head_fusion" = 0: K_KHAT as a kernel of its own); the timed scope stays, empty.
static void launch_tiptilt(mpsfr_ctx* c, hipStream_t s0, const CallPrep& p, const DevParams& d, mpsfr_ctx::Slot& sl,
                           bool fused) {
    ProfScope ps(c, K_MOFFAT_KERNELS, s0);
    if (fused) return;
    if (p.fft_conv) launch_khat(s0, p.ntask, d.gam, d.alp, sl.ktt.p, c->f64);   // [n][33][64] complex
    else launch_moffat_kernels(s0, p.ntask, d.gam, d.alp, sl.ktt.p, c->f64);
}

// The workspaces of a lane for chunks of TC tasks, for the stages the call runs on it
enum : unsigned { STAGE_A = 1, STAGE_B = 2, STAGE_TAIL = 4 };

static int size_lane(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, const CallPrep& p, int TC, unsigned stages, bool band_buf) {
    int rc;
    const int N = p.N, H1 = p.H1, nl = p.nl, ndir = p.ndir;
    const int TB = TC * p.gpp;              // stage-B tasks of a chunk: (task, position) pairs in a field call
    const size_t per_stamp = kStampPix;
    const bool prune = p.th.prune;
    if ((rc = ensure(c, ln.pre, (size_t)TB * nl * per_stamp * (c->f64 ? 8 : 4)))) return rc;
    if (stages & STAGE_TAIL) {
        if ((rc = ensure(c, ln.fin, (size_t)TB * nl * per_stamp * sizeof(double)))) return rc;
        if (band_buf && (rc = ensure(c, ln.band, (size_t)TB * p.nout * per_stamp * sizeof(double)))) return rc;
    }
    if (stages & STAGE_A) {
        if (p.series) {
            if ((rc = ensure(c, ln.pP, (size_t)TC * ndir * NAO * NAO * sizeof(double)))) return rc;
            if ((rc = ensure(c, ln.pT, (size_t)TC * ndir * H1 * kNH * 2 * sizeof(double)))) return rc;
            if ((rc = ensure(c, ln.psp, (size_t)TC * ndir * sizeof(double)))) return rc;
            if (prune && (rc = ensure(c, ln.dlin, (size_t)TC * ndir * H1 * (N / 32) * sizeof(float)))) return rc;
        } else {
            // row FFTs of the PSD: only the N/2 + 40 distinct rows are stored (K_PSD_ROWFFT)
            if ((rc = ensure(c, ln.C, (size_t)TC * ndir * (N / 2 + NAO / 2) * H1 * 2 * sizeof(double)))) return rc;
            if ((rc = ensure(c, ln.s00, (size_t)TC * ndir * psd_rowfft_groups(N) * sizeof(double)))) return rc;
        }
    }
    if (!(stages & (STAGE_A | STAGE_B))) return MPSFR_OK;
    {   // 16 lines of padding behind D: the last m-tile of the matrix-core kernel reads past line
        // N/2 (where its telescope table is -inf); fresh memory is zeroed so that what it reads
        // there is always a finite number
        const size_t cap_before = ln.D0t.cap;       // (a reallocation may return the same address)
        if ((rc = ensure(c, ln.D0t, ((size_t)TC * ndir * H1 + 16) * N * rsize(c)))) return rc;
        if (ln.D0t.cap != cap_before) {
            HIPCHK(hipMemset(ln.D0t.p, 0, ln.D0t.cap));
            ln.d0t_stale = 0;
        }
    }
    if (!p.mf && (rc = ensure(c, ln.Tq, (size_t)TB * nl * H1 * NSH * 2 * rsize(c)))) return rc;
    if (p.mf2) {
        if ((rc = ensure(c, ln.mown, mf2_own_bytes(N, TB, nl)))) return rc;
        if ((rc = ensure(c, ln.muni, mf2_uni_bytes(N, TB, nl)))) return rc;
        if ((rc = ensure(c, ln.msched, mf2_sched_bytes(N, TB, nl, c->mf_permax)))) return rc;
        if ((rc = ensure(c, ln.mpart, mf2_part_bytes(N, TB, nl)))) return rc;
    }
    if (prune) {
        if ((rc = ensure(c, ln.dmin, (size_t)TC * ndir * H1 * sizeof(float)))) return rc;
        if ((rc = ensure(c, ln.dblk, (size_t)ndir * mf_dminb_bytes(N, TC)))) return rc;
        if (p.mf && (rc = ensure(c, ln.dminb, mf_dminb_bytes(N, TB)))) return rc;
        if (p.mf && (rc = ensure(c, ln.order, (size_t)TB * sizeof(int)))) return rc;
        if (p.mf && (rc = ensure(c, ln.thrf, (size_t)TB * sizeof(float)))) return rc;
        if ((rc = ensure(c, ln.vkeep, (size_t)TB * ((nl + 1) / 2) * sizeof(int)))) return rc;
    }
    return MPSFR_OK;
}

// Where the chunks of a pipeline call write: the caller's device buffers, or the context's
static int size_outputs(mpsfr_ctx* c, const CallPrep& p, int NL, CallOuts& o) {
    int rc;
    if (NL > 1 && (rc = ensure(c, c->lsum, (size_t)NL * p.nsum * kStampPix * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->sum, (size_t)p.nsum * kStampPix * sizeof(double)))) return rc;
    o.d_fin_all = (o.dev && o.psf && !p.band) ? o.psf : nullptr;
    if (o.dev && o.fit) {
        o.d_fit_all = o.fit;
    } else {
        if ((rc = ensure(c, c->fit, (size_t)p.ntask * p.nsum * NFIT * sizeof(double)))) return rc;
        o.d_fit_all = (double*)c->fit.p;
    }
    o.d_sum = (o.dev && o.sum) ? o.sum : (double*)c->sum.p;
    return MPSFR_OK;
}

// the call's tables are produced on its first lane; the other lanes wait for them
static int share_tables(mpsfr_ctx* c, const CallLanes& L) {
    if (L.NL > 1) {
        if (!c->tables_ready) HIPCHK(hipEventCreateWithFlags(&c->tables_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->tables_ready, L.at(c, 0).stream));
        for (int j = 1; j < L.NL; ++j) HIPCHK(hipStreamWaitEvent(L.at(c, j).stream, c->tables_ready, 0));
    }
    return MPSFR_OK;
}

// Does this call share the GPU with another lane's kernels?  Then its two persistent kernels leave an eighth of
// the CUs free (persist_grid): K_OTF_MFMA2 (136 KB of LDS, 3 x 168 registers per SIMD) and K_DPHI_SERIES (two
// waves of 238 registers) admit nothing beside them on a CU they hold, and the other lane's latency-bound
// kernels (the patch, K_MF_PREP, K_MF_FINISH) stood parked behind them for 30-50 us (profiles/r05_trace_gaps.txt).
// A call that runs alone keeps the whole chip (one lane: -5 % with the reserve).
static bool lanes_are_shared(const mpsfr_ctx* c, const CallLanes& L) {
    if (L.NL > 1) return true;
    if (L.NLmax > 1 && c->pipeline_calls && (c->reserve_mf < 0 || c->reserve_a < 0))
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k) {
            const mpsfr_ctx::Lane& o = c->lane[k];
            if (k == L.index(0) || !o.busy || !o.stream) continue;
            if (!lane_idle(o)) return true;
        }
    return false;
}

// The end of a call on its lanes, its slot and the join stream: the lanes' markers (none, the slot's or their own:
// Markers), the outputs they wrote, the sum of the per-lane stamp sums in lane order (d_sum, or nullptr for a call
// without one)
static int call_end(mpsfr_ctx* c, const CallLanes& L, mpsfr_ctx::Slot& sl, const Markers& m, const void* const outs[3],
                    int nsum, double* d_sum) {
    hipStream_t s = c->stream;
    for (int j = 0; j < L.NL; ++j) {
        mpsfr_ctx::Lane& ln = L.at(c, j);
        if (m.zero) {
            ln.marked = false;               // (lane_end records a marker if somebody has to wait for the lane)
        } else if (m.lean) {
            HIPCHK(hipEventRecord(sl.call_done, ln.stream));
            ln.done_ev = sl.call_done;
            ln.marked = true;
        } else {
            HIPCHK(hipEventRecord(ln.done, ln.stream));
            ln.done_ev = ln.done;
            ln.marked = true;
            HIPCHK(hipStreamWaitEvent(s, ln.done, 0));
        }
        ln.busy = true;
        for (int a = 0; a < 3; ++a) ln.outs[ln.nouts % mpsfr_ctx::Lane::NHIST][a] = outs[a];
        ln.nouts += 1;
    }
    if (d_sum && L.NL > 1) {       // add the per-lane sums in lane order
        {
            ProfScope ps(c, K_STAMP_SUM);
            launch_stamp_sum(s, L.NL, nsum, c->lsum.p, false, d_sum, 0);
        }
        if (!c->lsum_done) HIPCHK(hipEventCreateWithFlags(&c->lsum_done, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->lsum_done, s));
        c->lsum_busy = true;
    }
    if (!m.lean) {
        HIPCHK(hipEventRecord(sl.call_done, s));
        if (!c->stream_tail) HIPCHK(hipEventCreateWithFlags(&c->stream_tail, hipEventDisableTiming));
    }
    sl.call_pending = true;
    sl.last_lane = m.lean ? L.index(0) : -1;
    sl.has_event = !m.zero;
    return MPSFR_OK;
}

// bookkeeping for debug_fetch.  dlin: the series form of stage A wrote its line minima
static void remember_call(mpsfr_ctx* c, const CallPrep& p, bool dlin) {
    c->last_ndir = p.ndir;
    c->last_gpp = p.gpp;
    c->last_nl = p.nl;
    c->last_mf = p.mf;
    c->last_mf2 = p.mf2;
    c->last_pruned = p.th.prune;
    c->last_dlin = dlin;
    c->last_thr_blk = p.th.thr_blk;
    c->last_floor_per_task = p.th.floor_per_task;
    const float thr[7] = {p.th.thr_eps, p.th.thr_floor, p.th.thr_mid, p.th.tier_half, p.th.thr_blk, p.th.thr_sum,
                          p.th.c2min};
    for (int k = 0; k < 7; ++k) c->last_thr[k] = thr[k];
    c->last_lpc.resize(p.nl);
    for (int l = 0; l < p.nl; ++l) c->last_lpc[l] = p.lp[l].c;
}

// ---- chunk stages: tasks [t0, t0 + tc) of a call on one lane

struct Chunk {
    int t0, tc;
    int j;               // position of the lane among the call's lanes
    bool accumulate;     // the lane has summed a chunk of this call already
    bool shared;         // the call shares the GPU with another lane's kernels (lanes_are_shared)
};

// What an earlier call left in D0t where this one does not write but reads (Lane::d0t_stale): cleared once, the whole
// buffer, on the lane's stream behind that call's readers.  A run of series calls never comes here.  skip_form: the
// writer is the series form with the support skip; `leaves`: the state the writer leaves behind.
static int d0t_begin(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, bool skip_form, int leaves) {
    if (ln.d0t_stale == 2 || (ln.d0t_stale == 1 && skip_form)) {
        HIPCHK(hipMemsetAsync(ln.D0t.p, 0, ln.D0t.cap, ln.stream));
        ln.d0t_stale = 0;
        ++c->d0t_clears;
    }
    if (ln.d0t_stale < leaves) ln.d0t_stale = leaves;
    return MPSFR_OK;
}

// Stage A: the structure functions D of the chunk's tasks and directions into the lane's D0t, in the series + patch
// form or through the full-size transforms.  fuse_khat: the chunk's tip-tilt spectra ride in the patch launch.
static int stage_a(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, const CallPrep& p, const DevParams& d, const Chunk& ck,
                   bool fuse_khat) {
    hipStream_t ls = ln.stream;
    const int N = p.N, ndir = p.ndir, ntd = ck.tc * ndir, t0 = ck.t0;
    const bool skip_form = p.series && c->support_skip;
    if (int rc = d0t_begin(c, ln, skip_form, skip_form ? 0 : 1)) return rc;
    const double cfit = fit_constant(), scale2 = dphi_scale2();
    int* msched = p.mf2 ? (int*)ln.msched.p : nullptr;
    if (p.series) {
        {
            ProfScope ps(c, K_PATCH, ls);
            PatchKhat kh;
            if (fuse_khat) {
                kh.n = ck.tc;
                kh.gam = d.gam + t0;
                kh.alp = d.alp + t0;
                kh.out = const_cast<char*>(d.ktt) + (size_t)t0 * p.ksz;
                kh.f64 = c->f64;
            }
            launch_patch(ls, N, ntd, ndir, d.tp + t0, (const double*)c->aotab.p, cfit, c->stwk.p,
                         (double*)ln.pP.p, ln.pT.p, (double*)ln.psp.p, c->f64, kh, d.mix(t0));
        }
        ProfScope ps(c, K_DPHI_SERIES, ls);
        launch_dphi_series(ls, N, ntd, ndir, d.tp + t0, ln.pT.p, (const double*)ln.psp.p, c->scoef.p,
                           c->stwk.p, scale2, ln.D0t.p, p.th.prune ? (float*)ln.dlin.p : nullptr, c->f64,
                           msched, persist_grid(c, ln, c->reserve_a, ck.shared),
                           c->support_skip ? (const unsigned*)c->ssup.p : nullptr);
    } else {
        {
            ProfScope ps(c, K_PSD_ROWFFT, ls);
            launch_psd_rowfft(ls, N, ntd, ndir, d.tp + t0, (const double*)c->aotab.p, cfit, ln.C.p,
                              c->tw64.p, (double*)ln.s00.p, c->f64, d.mix(t0));
        }
        ProfScope ps(c, K_COLFFT_DPHI, ls);
        launch_colfft_dphi(ls, N, ntd, ln.C.p, (const double*)ln.s00.p, scale2, ln.D0t.p,
                           c->f64, c->tw64.p, msched);
    }
    return MPSFR_OK;
}

// Stage B: its preparation (line and block bounds, masks, work lists) and the per-wavelength stage itself, from the
// lane's D0t into its `pre` stamps: the thin-wave kernel, the kernel for several directions, or the FFTs.
// from_lines: stage A's series form left the per-line minima in dlin.
static int stage_b(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, const CallPrep& p, const DevParams& d, const Chunk& ck,
                   bool from_lines, CallLanes& L) {
    hipStream_t ls = ln.stream;
    const int N = p.N, nl = p.nl, ndb = p.ndb, ntd = ck.tc * p.ndir;
    const int tb = ck.tc * p.gpp;            // stage-B tasks of the chunk
    const Thresholds& th = p.th;
    const bool prune = th.prune;
    if (p.mf2) {
        // thin-wave kernel: block minima (one direction: they are the minima over the directions),
        // then masks and work lists (otf_mfma2.hip); no line bounds needed
        ProfScope ps(c, K_MF_PREP, ls);
        // (series form of stage A: the per-line minima go straight to K_MF_PREP, which takes the minimum
        // over a block's 16 lines itself -- K_DMIN16 was 6 us of latency at 512^2, 13 at 1280^2)
        const bool lines = prune && from_lines;
        if (prune && !lines) launch_dmin(ls, N, ntd, ln.D0t.p, (float*)ln.dmin.p, (float*)ln.dblk.p);
        launch_mf_prep(ls, N, tb, nl, c->mf_permax, d.lp, (prune && !lines) ? (const float*)ln.dblk.p : nullptr,
                       (const float*)c->tlb.p, th.thr_eps, th.thr_floor, th.thr_mid, th.tier_half, ln.D0t.p,
                       (const float*)c->tl2.p, ln.mown.p, ln.muni.p, ln.msched.p,
                       lines ? (const float*)ln.dlin.p : nullptr);
    } else if (prune) {
        ProfScope ps(c, p.mf ? K_MF_PREP : K_VKEEP, ls);
        if (from_lines) launch_dmin16(ls, N, ntd, (const float*)ln.dlin.p, (float*)ln.dmin.p, (float*)ln.dblk.p);
        else launch_dmin(ls, N, ntd, ln.D0t.p, (float*)ln.dmin.p, (float*)ln.dblk.p, c->f64);
        launch_vkeep(ls, N, tb, ndb, nl, d.lp, (const float*)ln.dmin.p, (const float*)ln.dblk.p,
                     (const float*)c->tlmax.p, th.thr_sum, (int*)ln.vkeep.p, c->prune_fixed,
                     p.mf ? (float*)ln.dminb.p : nullptr);
        if (p.mf) launch_task_order(ls, tb, nl, (const int*)ln.vkeep.p, (int*)ln.order.p);
    }
    const int* d_vkeep = prune ? (const int*)ln.vkeep.p : nullptr;
    if (int rc = stagger_here(c, L, 2, ln)) return rc;
    if (p.mf2) {
        // (timed through the dispatch packet of K_OTF_MFMA2 itself: the persistent kernel alone, without
        // K_MF_FINISH and without marker packets round it)
        ProfScope ps(c, K_OTF_MFMA, ls, false);
        launch_otf_mfma2(ls, N, tb, nl, c->mf_permax, persist_grid(c, ln, c->reserve_mf, ck.shared), ln.D0t.p,
                         (const float*)c->tl2.p, d.lp, c->etab.p, c->gtab.p, ln.mown.p, ln.muni.p, ln.msched.p,
                         ln.mpart.p, ln.pre.p, c->mf_clock ? c->mfclk.p : nullptr, ps.a, ps.b);
    } else if (p.mf) {
        ProfScope ps(c, K_OTF_MFMA, ls);
        if (th.floor_per_task)
            launch_peak_floor(ls, N, tb, ndb, ln.D0t.p, (const float*)c->tl2.p, th.c2min, th.tier_half, th.thr_floor,
                              (float*)ln.thrf.p);
        launch_otf_mfma(ls, N, tb, ndb, nl, ln.D0t.p, (const float*)c->tl2.p, d.lp, c->etab.p,
                        c->gtab.p, d_vkeep, prune ? (const float*)ln.dminb.p : nullptr,
                        (const float*)c->tlb.p, th.thr_blk, ln.pre.p,
                        prune ? (const int*)ln.order.p : nullptr, c->mf_clock ? c->mfclk.p : nullptr,
                        th.floor_per_task ? (const float*)ln.thrf.p : nullptr);
    } else {
        {
            ProfScope ps(c, K_OTF_ROWFFT, ls);
            launch_otf_rowfft(ls, N, tb, ndb, nl, ln.D0t.p, c->tel.p, d.lp,
                              (const int*)c->samp_p.p, c->samp_a.p, c->xtab.p, ln.Tq.p, c->tw64.p,
                              c->f64, c->fast_exp, d_vkeep);
        }
        ProfScope ps(c, K_COLPASS, ls);
        launch_colpass(ls, N, tb, nl, ln.Tq.p, c->G.p, ln.pre.p, c->f64, d_vkeep);
    }
    return MPSFR_OK;
}

// The tail: the two convolutions of the lane's `pre` stamps, the band reduction of a band call, the fit with the
// chunk's stamp sum (or the sum alone), the copy of host stamps.  NL: the lanes of the call (several: the lane sums
// into its own partial sum).
static int chunk_tail(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, const CallPrep& p, const DevParams& d, const CallOuts& o,
                      const Chunk& ck, int NL) {
    hipStream_t ls = ln.stream;
    const int nl = p.nl, nsum = p.nsum, t0 = ck.t0, tc = ck.tc;
    const int tb = tc * p.gpp;
    const size_t per_stamp = kStampPix;
    // final stamps: straight into the caller's device buffer (double), else a lane workspace --
    // float when the FFT convolution produces them and nobody outside reads them
    // (a band call keeps its per-wavelength stamps in the lane: float in mixed mode)
    const bool fin_f32 = p.band ? (p.fft_conv && !c->f64)
                                : (p.fft_conv && !c->f64 && !o.d_fin_all && !(o.psf && !o.dev));
    void* d_fin = o.d_fin_all ? (void*)(o.d_fin_all + (size_t)t0 * nsum * per_stamp) : ln.fin.p;
    {
        ProfScope ps(c, K_CONV, ls);
        const char* ktt = d.ktt + (size_t)t0 * p.ksz;
        if (p.fft_conv) launch_conv_fft(ls, tb, nl, ln.pre.p, ktt, c->kmuse.p, d_fin, fin_f32, c->f64, p.gpp);
        else launch_conv(ls, tb, nl, ln.pre.p, ktt, c->kmuse.p, (double*)d_fin, c->f64, p.gpp);
    }
    // a band call: the chunk's stamps reduced over wavelength (timed as the stamp sum); what follows -- fit, sum,
    // copies -- then reads the double band stamps
    void* d_res = d_fin;
    bool res_f32 = fin_f32;
    if (p.band) {
        ProfScope ps(c, K_STAMP_SUM, ls);
        double* d_band = (o.dev && o.psf) ? o.psf + (size_t)t0 * nsum * per_stamp : (double*)ln.band.p;
        launch_band_reduce(ls, tb, nl, p.nout, d_fin, fin_f32, d.bw, d_band);
        d_res = d_band;
        res_f32 = false;
    }
    // per-lane partial stamp sums in chunk order; combined in lane order by call_end (deterministic)
    double* lsum = !o.sum ? nullptr : NL > 1 ? (double*)c->lsum.p + (size_t)ck.j * nsum * per_stamp : o.d_sum;
    if (o.fit) {               // (with the chunk's stamp sum as the first workgroups of the same launch)
        ProfScope ps(c, K_FIT, ls);
        launch_fit(ls, tb * p.nout, d_res, res_f32, o.d_fit_all + (size_t)t0 * nsum * NFIT, c->f64,
                   o.sum ? tc : 0, nsum, o.sum ? lsum : nullptr, ck.accumulate ? 1 : 0);
    } else if (o.sum) {
        ProfScope ps(c, K_STAMP_SUM, ls);
        launch_stamp_sum(ls, tc, nsum, d_res, res_f32, lsum, ck.accumulate ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    if (!o.dev && o.psf) {
        HIPCHK(hipMemcpyAsync(o.psf + (size_t)t0 * nsum * per_stamp, d_res,
                              (size_t)tc * nsum * per_stamp * sizeof(double), hipMemcpyDeviceToHost, ls));
    }
    return MPSFR_OK;
}

// The chunks of a call in order over its lanes: run(lane, chunk) queues one
extern "C++" template <class Run>
static int for_each_chunk(mpsfr_ctx* c, int ntask, const CallLanes& L, bool shared, Run&& run) {
    int nchunk_lane[mpsfr_ctx::MAX_LANES] = {0, 0, 0, 0};      // by lane position j in this call
    int ci = 0;
    for (int t0 = 0; t0 < ntask; t0 += L.TC, ++ci) {
        const int j = ci % L.NL;
        const Chunk ck = {t0, (ntask - t0) < L.TC ? (ntask - t0) : L.TC, j, nchunk_lane[j] > 0, shared};
        mpsfr_ctx::Lane& ln = L.at(c, j);
        int rc;
        if ((rc = stagger_wait(c, ln))) return rc;
        if ((rc = run(ln, ck))) return rc;
        ++nchunk_lane[j];
        c->last_chunk_tasks = ck.tc;
        c->last_lane = L.index(j);
    }
    return MPSFR_OK;
}

// ---- the drivers

// The pipeline: every stamp, sum and fit of mpsfr_reconstruct, _field, _band, _profile and _multi*.
// (refuses) marks the steps that may refuse the call for its arguments; everything after them only fails with the GPU.
static int reconstruct_impl(mpsfr_ctx* c, const CallArgs& a, const StageIO& io) {
    HostClock clock;
    CallPrep p;
    int rc;
    if ((rc = prepare_call(c, a, io, p))) return rc;                      // (refuses)  pure host
    HIPCHK(hipSetDevice(c->device));
    // context state: ticket, lanes, slot
    CallOuts o;
    o.psf = a.psf_out, o.sum = a.psf_sum_out, o.fit = a.fit_out, o.dev = a.on_device != 0;
    mpsfr_ctx::Ticket* tk = nullptr;
    if (a.on_device == 2 && (rc = ticket_begin(c, p, o, tk))) return rc;
    const bool pipelined = c->pipeline_calls && o.dev;     // (else a synchronous call: no neighbour on another lane)
    CallLanes L;
    if ((rc = lanes_begin(c, p.ntask, pipeline_chunk_tasks(c, p, !pipelined), pipelined, L))) return rc;
    const Markers marks(c, o.dev, tk != nullptr, L.NL);
    hipStream_t s0 = L.at(c, 0).stream;        // the call's tables are produced on its first lane
    std::vector<unsigned char> ao_key = ao_cache_key(p.g, p.ly, a.mask_rec, a.mask_res);
    bool ao_cached = false, lam_cached = false;
    if ((rc = size_ao_tables(c, p, ao_key, ao_cached))) return rc;
    const Blob blob(p, a.mask_rec && !ao_cached);
    mpsfr_ctx::Slot* sl = nullptr;
    if ((rc = slot_acquire(c, blob.bytes, (size_t)p.ntask * p.ksz, sl, clock.blocked))) return rc;
    blob.fill(sl->host, p, a.mask_rec, a.mask_res);
    // queueing: waits, parameters, tables
    const void* outs[3] = {o.dev ? (const void*)o.psf : nullptr, o.dev ? (const void*)o.sum : nullptr,
                           o.dev ? (const void*)o.fit : nullptr};
    if ((rc = queue_call_waits(c, L, *sl, outs))) return rc;
    const std::vector<double> lb_key(a.lbda_nm, a.lbda_nm + a.nl);
    if ((rc = size_wavelength_tables(c, p, lb_key, lam_cached))) return rc;
    if ((rc = send_params(c, *sl, s0, blob.bytes, marks))) return rc;
    const DevParams d = blob.views(*sl, p);
    if ((rc = refresh_tables(c, s0, p, d, ao_cached ? nullptr : &ao_key, lam_cached ? nullptr : &lb_key))) return rc;
    const bool fuse_khat = c->head_fusion && p.series && p.fft_conv;
    launch_tiptilt(c, s0, p, d, *sl, fuse_khat);
    // workspaces
    for (int j = 0; j < L.NL; ++j)
        if ((rc = size_lane(c, L.at(c, j), p, L.TC, STAGE_A | STAGE_B | STAGE_TAIL, p.band && !(o.dev && o.psf))))
            return rc;
    if ((rc = size_outputs(c, p, L.NL, o))) return rc;
    if ((rc = share_tables(c, L))) return rc;
    // the chunks
    rc = for_each_chunk(c, p.ntask, L, lanes_are_shared(c, L), [&](mpsfr_ctx::Lane& ln, const Chunk& ck) {
        int r;
        if ((r = stage_a(c, ln, p, d, ck, fuse_khat))) return r;
        if ((r = stagger_here(c, L, 1, ln))) return r;
        if ((r = stage_b(c, ln, p, d, ck, p.th.prune && p.series, L))) return r;
        return chunk_tail(c, ln, p, d, o, ck, L.NL);
    });
    if (rc) return rc;
    // the end: markers, lane sum, slot; results to the host
    if ((rc = call_end(c, L, *sl, marks, outs, p.nsum, o.sum ? o.d_sum : nullptr))) return rc;
    remember_call(c, p, p.th.prune && p.series);
    if (tk && (rc = ticket_finish(c, tk))) return rc;
    if (!o.dev) {
        hipStream_t s = c->stream;
        if (o.fit)
            HIPCHK(hipMemcpyAsync(o.fit, o.d_fit_all, (size_t)p.ntask * p.nsum * NFIT * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
        if (o.sum)
            HIPCHK(hipMemcpyAsync(o.sum, o.d_sum, (size_t)p.nsum * kStampPix * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    clock.finish(c);
    return MPSFR_OK;
}

// A device buffer that lives as long as a stage-level driver's call, released on every path out of it
struct ScopedBuf : DevBuf {
    ~ScopedBuf() { release(*this); }
};

// What the stage-level drivers share with the pipeline at their head: lanes for chunks of `chunk_tasks` tasks, a slot,
// the call's waits, the parameters on their way, the cached tables the call reads (`tables`) and the tip-tilt
// spectra.  Synchronous host-buffer calls: they join, and they name no device outputs.
enum : unsigned { TABLES_AO = 1, TABLES_WAVELENGTH = 2 };
static const void* const kNoOuts[3] = {nullptr, nullptr, nullptr};

struct StageCall {
    CallLanes L;
    mpsfr_ctx::Slot* sl = nullptr;
    hipStream_t s0 = nullptr;
    DevParams d;
};

static int stage_call_begin(mpsfr_ctx* c, const CallPrep& p, const CallArgs& a, int chunk_tasks, unsigned tables,
                            HostClock& clock, StageCall& sc) {
    int rc;
    std::vector<unsigned char> ao_key;
    bool ao_cached = true, lam_cached = true;
    if (tables & TABLES_AO) {
        ao_key = ao_cache_key(p.g, p.ly, a.mask_rec, a.mask_res);
        if ((rc = size_ao_tables(c, p, ao_key, ao_cached))) return rc;
    }
    const Blob blob(p, a.mask_rec && !ao_cached);
    if ((rc = lanes_begin(c, p.ntask, chunk_tasks, false, sc.L))) return rc;
    sc.s0 = sc.L.at(c, 0).stream;
    if ((rc = slot_acquire(c, blob.bytes, (size_t)p.ntask * p.ksz, sc.sl, clock.blocked))) return rc;
    blob.fill(sc.sl->host, p, a.mask_rec, a.mask_res);
    if ((rc = queue_call_waits(c, sc.L, *sc.sl, kNoOuts))) return rc;
    const std::vector<double> lb_key(a.lbda_nm, a.lbda_nm + a.nl);
    if ((tables & TABLES_WAVELENGTH) && (rc = size_wavelength_tables(c, p, lb_key, lam_cached))) return rc;
    if ((rc = send_params(c, *sc.sl, sc.s0, blob.bytes, Markers(c, false, false, sc.L.NL)))) return rc;
    sc.d = blob.views(*sc.sl, p);
    if ((rc = refresh_tables(c, sc.s0, p, sc.d, ao_cached ? nullptr : &ao_key, lam_cached ? nullptr : &lb_key))) return rc;
    launch_tiptilt(c, sc.s0, p, sc.d, *sc.sl, false);
    return MPSFR_OK;
}

// ... and at their end: the lanes' markers, the slot, `last_*`, the join stream drained
static int stage_call_end(mpsfr_ctx* c, const CallPrep& p, StageCall& sc, const HostClock& clock) {
    if (int rc = call_end(c, sc.L, *sc.sl, Markers(c, false, false, sc.L.NL), kNoOuts, p.nsum, nullptr)) return rc;
    remember_call(c, p, false);
    HIPCHK(hipStreamSynchronize(c->stream));
    clock.finish(c);
    return MPSFR_OK;
}

// Stamps between the host's doubles and a lane's `pre` (float in mixed mode), n values, synchronously
static int copy_pre(mpsfr_ctx* c, mpsfr_ctx::Lane& ln, const double* in, double* out, size_t n) {
    hipStream_t ls = ln.stream;
    if (c->f64) {
        if (in) HIPCHK(hipMemcpyAsync(ln.pre.p, in, n * sizeof(double), hipMemcpyHostToDevice, ls));
        else HIPCHK(hipMemcpyAsync(out, ln.pre.p, n * sizeof(double), hipMemcpyDeviceToHost, ls));
        HIPCHK(hipStreamSynchronize(ls));
        return MPSFR_OK;
    }
    std::vector<float> tmp(n);
    if (in) {
        for (size_t i = 0; i < n; ++i) tmp[i] = (float)in[i];
        HIPCHK(hipMemcpyAsync(ln.pre.p, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, ls));
        HIPCHK(hipStreamSynchronize(ls));
    } else {
        HIPCHK(hipMemcpyAsync(tmp.data(), ln.pre.p, n * sizeof(float), hipMemcpyDeviceToHost, ls));
        HIPCHK(hipStreamSynchronize(ls));
        for (size_t i = 0; i < n; ++i) out[i] = (double)tmp[i];
    }
    return MPSFR_OK;
}

// simul_psd_wfm: the PSD of task 0, every direction, as an image.  Parameters up, AO tables, the image, copy out.
// Nothing of it stays in flight, so it leaves the lane and the slot unmarked (and its host time uncounted).
static int simul_psd_impl(mpsfr_ctx* c, const CallArgs& a, const StageIO& io, double* psd_out) {
    HostClock clock;
    CallPrep p;
    int rc;
    if ((rc = call_shape(c, a, io, p))) return rc;                        // (refuses)
    if ((rc = wavelength_scalars(c, a, false, p))) return rc;             // (the placeholder wavelength)
    if ((rc = task_scalars(c, a, io, p))) return rc;                      // (refuses)
    p.g = ao_geometry(a, io, p.ndir);
    HIPCHK(hipSetDevice(c->device));
    StageCall sc;
    if ((rc = stage_call_begin(c, p, a, p.ntask, TABLES_AO, clock, sc))) return rc;
    const size_t n = (size_t)p.ndir * p.N * p.N;
    ScopedBuf img;
    if ((rc = ensure(c, img, n * sizeof(double)))) return rc;
    launch_psd_image(sc.s0, p.N, p.ndir, p.tp[0], (const double*)c->aotab.p, fit_constant(), dphi_scale2() * 128.0,
                     (double*)img.p, sc.d.mix(0));
    const hipError_t e1 = hipMemcpyAsync(psd_out, img.p, n * sizeof(double), hipMemcpyDeviceToHost, sc.s0);
    const hipError_t e2 = hipStreamSynchronize(sc.s0);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(MPSFR_E_HIP, "copying the PSD image failed");
    return MPSFR_OK;
}

// psf_muse on the caller's PSD (one task, ndir planes, centred, in the reference's units): wavelength tables, the
// structure function of the PSD into a lane's D0t, stage B, and the stamps before the convolutions out as float64.
// The caller's PSD may leave anything in D0t (d0t_stale 2): the next call that writes it clears it first.
static int psf_from_psd_impl(mpsfr_ctx* c, const CallArgs& a, const double* psd_in) {
    HostClock clock;
    CallPrep p;
    int rc;
    if ((rc = call_shape(c, a, StageIO(), p))) return rc;                 // (refuses)
    if ((rc = wavelength_scalars(c, a, true, p))) return rc;              // (refuses)
    if ((rc = task_scalars(c, a, StageIO(), p))) return rc;               // (the placeholder row)
    p.series = false;
    stage_b_paths(c, p);
    HIPCHK(hipSetDevice(c->device));
    StageCall sc;
    if ((rc = stage_call_begin(c, p, a, p.ntask, TABLES_WAVELENGTH, clock, sc))) return rc;
    if ((rc = size_lane(c, sc.L.at(c, 0), p, sc.L.TC, STAGE_B, false))) return rc;
    rc = for_each_chunk(c, p.ntask, sc.L, lanes_are_shared(c, sc.L), [&](mpsfr_ctx::Lane& ln, const Chunk& ck) {
        int r;
        hipStream_t ls = ln.stream;
        const int N = p.N, ndir = p.ndir;
        const size_t n = (size_t)ndir * N * N;
        if ((r = d0t_begin(c, ln, false, 2))) return r;
        {
            ScopedBuf img, cm;
            if ((r = ensure(c, img, n * sizeof(double)))) return r;
            if ((r = ensure(c, cm, (size_t)ndir * N * p.H1 * 2 * sizeof(double)))) return r;
            hipError_t e1 = hipMemcpyAsync(img.p, psd_in, n * sizeof(double), hipMemcpyHostToDevice, ls);
            launch_dphi_from_psd(ls, N, ndir, (const double*)img.p, cm.p, 2.0 / 256.0, ln.D0t.p, c->f64, c->tw64.p);
            if (p.mf2 && e1 == hipSuccess) e1 = hipMemsetAsync(ln.msched.p, 0, kMfSchedInts * sizeof(int), ls);
            const hipError_t e2 = hipStreamSynchronize(ls);
            if (e1 != hipSuccess || e2 != hipSuccess) return fail(MPSFR_E_HIP, "the structure function of the PSD failed");
        }
        if ((r = stagger_here(c, sc.L, 1, ln))) return r;
        if ((r = stage_b(c, ln, p, sc.d, ck, false, sc.L))) return r;
        if ((r = copy_pre(c, ln, nullptr, a.psf_out, (size_t)ck.tc * p.nl * kStampPix))) return r;
        HIPCHK(hipGetLastError());
        return MPSFR_OK;
    });
    if (rc) return rc;
    return stage_call_end(c, p, sc, clock);
}

// convolve_final_psf on the caller's stamps: wavelength tables and tip-tilt spectra, the stamps into a lane per
// chunk, the tail.  It needs none of the workspaces of stages A and B and leaves D0t alone; its host copies are per
// chunk, so it keeps the chunking of a call's stamps.
static int convolve_stamps_impl(mpsfr_ctx* c, const CallArgs& a, const double* pre_in) {
    HostClock clock;
    CallPrep p;
    int rc;
    if ((rc = call_shape(c, a, StageIO(), p))) return rc;                 // (refuses)
    if ((rc = wavelength_scalars(c, a, false, p))) return rc;             // (refuses)
    if ((rc = task_scalars(c, a, StageIO(), p))) return rc;               // (refuses)
    stage_b_paths(c, p);                 // (which tables ride with the wavelengths' cache; last_* as a pipeline call)
    HIPCHK(hipSetDevice(c->device));
    const int nlanes = c->nlanes == 0 ? 2 : c->nlanes;
    const int TC = c->chunk_tasks > 0 ? c->chunk_tasks : auto_chunk_tasks(p.ntask, p.nl, 0.0, nlanes, true);
    StageCall sc;
    if ((rc = stage_call_begin(c, p, a, TC, TABLES_WAVELENGTH, clock, sc))) return rc;
    for (int j = 0; j < sc.L.NL; ++j)
        if ((rc = size_lane(c, sc.L.at(c, j), p, sc.L.TC, STAGE_TAIL, false))) return rc;
    if ((rc = share_tables(c, sc.L))) return rc;
    CallOuts o;
    o.psf = a.psf_out;
    rc = for_each_chunk(c, p.ntask, sc.L, false, [&](mpsfr_ctx::Lane& ln, const Chunk& ck) {
        int r;
        const size_t first = (size_t)ck.t0 * p.nl * kStampPix;
        if ((r = copy_pre(c, ln, pre_in + first, nullptr, (size_t)ck.tc * p.nl * kStampPix))) return r;
        if ((r = stagger_here(c, sc.L, 1, ln)) || (r = stagger_here(c, sc.L, 2, ln))) return r;
        return chunk_tail(c, ln, p, sc.d, o, ck, sc.L.NL);
    });
    if (rc) return rc;
    return stage_call_end(c, p, sc, clock);
}

// The checks the multi-context calls share: the contexts are there, and ...
static int check_multi(mpsfr_ctx* const* ctxs, int nctx, int ntask, int nl) {
    if (!ctxs || nctx < 1) return fail(MPSFR_E_INVALID, "need at least one context");
    for (int k = 0; k < nctx; ++k)
        if (!ctxs[k]) return fail(MPSFR_E_INVALID, "context %d is NULL", k);
    if (ntask < 1 || nl < 1) return fail(MPSFR_E_INVALID, "ntask and nl must be positive");
    return MPSFR_OK;
}

// ... they are alike
static int check_multi_alike(mpsfr_ctx* const* ctxs, int nctx) {
    for (int k = 1; k < nctx; ++k)
        if (ctxs[k]->dimpsf != ctxs[0]->dimpsf || ctxs[k]->N != ctxs[0]->N || ctxs[k]->prec != ctxs[0]->prec ||
            ctxs[k]->pixscale != ctxs[0]->pixscale)
            return fail(MPSFR_E_INVALID, "the contexts must share dim, dimpsf, pixscale and precision "
                                         "(context %d differs from context 0)", k);
    return MPSFR_OK;
}

// Contiguous, balanced row shards over `used` contexts: start[k] .. start[k + 1], the first ntask % used one row more
// (start has nctx + 1 entries: the contexts beyond `used` get no rows)
static std::vector<int> shard_bounds(int ntask, int nctx, int used) {
    std::vector<int> start(nctx + 1, ntask);
    start[0] = 0;
    for (int k = 0; k < used; ++k) start[k + 1] = start[k] + ntask / used + (k < ntask % used ? 1 : 0);
    return start;
}

// Row shards over several contexts (one per device), one host thread each.
int mpsfr_reconstruct_multi(mpsfr_ctx* const* ctxs, int nctx, int ntask, const double* seeing,
                            const double* gl, const double* l0, const uint8_t* three_lgs,
                            const double h[2], double wind_speed, int npsflin, int nl,
                            const double* lbda_nm, const uint8_t* mask_rec, const uint8_t* mask_res,
                            double* psf_out, double* psf_sum_out, double* fit_out) {
    if (int rc = check_multi(ctxs, nctx, ntask, nl)) return rc;
    if (nctx == 1 || ntask < nctx)
        return mpsfr_reconstruct(ctxs[0], ntask, seeing, gl, l0, three_lgs, h, wind_speed, npsflin, nl,
                                 lbda_nm, mask_rec, mask_res, psf_out, psf_sum_out, fit_out, 0);
    const size_t per_stamp = (size_t)ctxs[0]->dimpsf * ctxs[0]->dimpsf;
    if (int rc = check_multi_alike(ctxs, nctx)) return rc;
    const std::vector<int> start = shard_bounds(ntask, nctx, nctx);
    std::vector<std::vector<double>> sums(psf_sum_out ? nctx : 0);
    for (auto& v : sums) v.resize((size_t)nl * per_stamp);
    std::vector<int> rcs(nctx, MPSFR_OK);
    std::vector<std::string> errs(nctx);
    std::vector<std::thread> th;
    th.reserve(nctx);
    for (int k = 0; k < nctx; ++k)
        th.emplace_back([&, k] {
            const int a = start[k], n = start[k + 1] - a;
            rcs[k] = mpsfr_reconstruct(ctxs[k], n, seeing + a, gl + a, l0 + a, three_lgs ? three_lgs + a : nullptr, h,
                                       wind_speed, npsflin, nl, lbda_nm, mask_rec, mask_res,
                                       psf_out ? psf_out + (size_t)a * nl * per_stamp : nullptr,
                                       psf_sum_out ? sums[k].data() : nullptr,
                                       fit_out ? fit_out + (size_t)a * nl * NFIT : nullptr, 0);
            if (rcs[k] != MPSFR_OK) errs[k] = g_err;        // (the message is thread-local)
        });
    for (auto& t : th) t.join();
    for (int k = 0; k < nctx; ++k)
        if (rcs[k] != MPSFR_OK) return fail(rcs[k], "context %d: %s", k, errs[k].c_str());
    if (psf_sum_out)        // in context order: the result does not depend on which shard finished first
        for (size_t e = 0; e < (size_t)nl * per_stamp; ++e) {
            double t = sums[0][e];
            for (int k = 1; k < nctx; ++k) t += sums[k][e];
            psf_sum_out[e] = t;
        }
    return MPSFR_OK;
}

int mpsfr_reconstruct_multi_async(mpsfr_ctx* const* ctxs, int nctx, int ntask, const double* seeing,
                                  const double* gl, const double* l0, const uint8_t* three_lgs,
                                  const double h[2], double wind_speed, int npsflin, int nl,
                                  const double* lbda_nm, const uint8_t* mask_rec, const uint8_t* mask_res,
                                  double* psf_out, double* psf_sum_out, double* fit_out) {
    if (int rc = check_multi(ctxs, nctx, ntask, nl)) return rc;
    mpsfr_ctx::Multi& m = ctxs[0]->multi;
    if (m.pending) return fail(MPSFR_E_INVALID, "a multi-context call is pending on this context: mpsfr_wait_multi first");
    if (int rc = check_multi_alike(ctxs, nctx)) return rc;
    const size_t per_stamp = (size_t)ctxs[0]->dimpsf * ctxs[0]->dimpsf;
    const int used = ntask < nctx ? 1 : nctx;            // (like the blocking form: too few rows go to context 0)
    const std::vector<int> start = shard_bounds(ntask, nctx, used);
    m.nctx = nctx;
    m.n = (size_t)nl * per_stamp;
    m.user_sum = psf_sum_out;
    m.sums.assign(psf_sum_out ? (size_t)nctx * m.n : 0, 0.0);
    m.tickets.assign(nctx, -1);
    for (int k = 0; k < used; ++k) {
        const int a = start[k], n = start[k + 1] - a;
        const int rc = mpsfr_reconstruct(ctxs[k], n, seeing + a, gl + a, l0 + a, three_lgs ? three_lgs + a : nullptr, h,
                                         wind_speed, npsflin, nl, lbda_nm, mask_rec, mask_res,
                                         psf_out ? psf_out + (size_t)a * nl * per_stamp : nullptr,
                                         psf_sum_out ? m.sums.data() + (size_t)k * m.n : nullptr,
                                         fit_out ? fit_out + (size_t)a * nl * NFIT : nullptr, 2);
        if (rc != MPSFR_OK) {
            // the shards already queued still point at the caller's arrays and at m.sums: give them up -- on EVERY
            // context of the call, so that what is left pending does not depend on which shard failed (a caller
            // that also has single asynchronous calls in flight on these contexts loses them: include/mpsfr.h)
            const std::string msg = g_err;
            for (int q = 0; q < nctx; ++q) (void)mpsfr_abandon(ctxs[q]);
            return fail(rc, "context %d: %s", k, msg.c_str());
        }
        m.tickets[k] = mpsfr_last_ticket(ctxs[k]);
    }
    m.pending = true;
    return MPSFR_OK;
}

int mpsfr_wait_multi(mpsfr_ctx* const* ctxs, int nctx) {
    if (!ctxs || nctx < 1 || !ctxs[0]) return fail(MPSFR_E_INVALID, "need at least one context");
    mpsfr_ctx::Multi& m = ctxs[0]->multi;
    if (!m.pending) return MPSFR_OK;
    if (nctx != m.nctx) return fail(MPSFR_E_INVALID, "mpsfr_wait_multi: %d contexts, the pending call had %d", nctx, m.nctx);
    int rc = MPSFR_OK;
    std::string msg;
    for (int k = 0; k < nctx; ++k) {
        if (m.tickets[k] < 0) continue;
        const int r = mpsfr_wait(ctxs[k], m.tickets[k]);
        if (r != MPSFR_OK && rc == MPSFR_OK) { rc = r; msg = g_err; }
    }
    m.pending = false;
    if (rc != MPSFR_OK) return fail(rc, "%s", msg.c_str());
    if (m.user_sum)          // in context order: the result does not depend on which shard finished first
        for (size_t e = 0; e < m.n; ++e) {
            double t = m.sums[e];
            for (int k = 1; k < nctx; ++k)
                if (m.tickets[k] >= 0) t += m.sums[(size_t)k * m.n + e];
            m.user_sum[e] = t;
        }
    return MPSFR_OK;
}

int mpsfr_simul_psd(mpsfr_ctx* c, double seeing, double gl, double l0, int three_lgs, const double h[2],
                    double wind_speed, int npsflin, const uint8_t* mask_rec, const uint8_t* mask_res,
                    double* psd_out) {
    if (!c || !psd_out) return fail(MPSFR_E_INVALID, "NULL argument");
    const uint8_t t3 = three_lgs ? 1 : 0;
    CallArgs a;
    a.seeing = &seeing, a.gl = &gl, a.l0 = &l0, a.three_lgs = &t3;
    a.h = h, a.wind_speed = wind_speed, a.npsflin = npsflin;
    a.mask_rec = mask_rec, a.mask_res = mask_res;
    return guarded(c, [&] { return simul_psd_impl(c, a, StageIO(), psd_out); });
}

int mpsfr_psf_from_psd(mpsfr_ctx* c, int ndir, const double* psd, int nl, const double* lbda_nm, double* psf_out) {
    if (!c || !psd || !psf_out) return fail(MPSFR_E_INVALID, "NULL argument");
    int npl = 0;
    for (int k = 1; k <= 5; ++k)
        if (k * k == ndir) npl = k;
    if (npl == 0) return fail(MPSFR_E_INVALID, "ndir=%d is not the square of 1..5", ndir);
    // (a NaN or an infinity would spread through the whole transform: refused before anything is queued)
    const size_t npix = (size_t)ndir * c->N * c->N;
    for (size_t i = 0; i < npix; ++i)
        if (!std::isfinite(psd[i])) return fail(MPSFR_E_INVALID, "psd[%zu] is not finite", i);
    CallArgs a;
    a.npsflin = npl, a.nl = nl, a.lbda_nm = lbda_nm, a.psf_out = psf_out;
    return guarded(c, [&] { return psf_from_psd_impl(c, a, psd); });
}

int mpsfr_convolve_stamps(mpsfr_ctx* c, int ntask, const double* seeing, const double* gl, const double* l0,
                          int nl, const double* lbda_nm, const double* psf_in, double* psf_out) {
    if (!c || !psf_in || !psf_out) return fail(MPSFR_E_INVALID, "NULL argument");
    CallArgs a;
    a.ntask = ntask, a.seeing = seeing, a.gl = gl, a.l0 = l0;
    a.nl = nl, a.lbda_nm = lbda_nm, a.psf_out = psf_out;
    return guarded(c, [&] { return convolve_stamps_impl(c, a, psf_in); });
}

int mpsfr_psd_to_psf(mpsfr_ctx* c, int npsd, const double* psd, int npup, const double* pup,
                     const double* phase_static, double D, int nl, const double* lbda_m, int dimnum,
                     double* psf_out, int on_device) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    if (!psd || !pup || !lbda_m || !psf_out) return fail(MPSFR_E_INVALID, "NULL argument");
    const int N = c->N, M = dimnum, P = npup;
    if (!p2p_supported(M))
        return fail(MPSFR_E_INVALID, "dimnum=%d not supported (128, 256, 512, 1024, 1280)", M);
    if (M > N) return fail(MPSFR_E_INVALID, "dimnum=%d larger than the grid (dim=%d)", M, N);
    if (npsd < 1 || nl < 1) return fail(MPSFR_E_INVALID, "npsd=%d, nl=%d: both must be >= 1", npsd, nl);
    if (P < 1 || P > M) return fail(MPSFR_E_INVALID, "npup=%d must be in [1, dimnum=%d]", P, M);
    if (!(D > 0.0)) return fail(MPSFR_E_INVALID, "D must be > 0");
    for (int i = 0; i < nl; ++i)
        if (!(lbda_m[i] > 0.0)) return fail(MPSFR_E_INVALID, "lbda_m[%d] must be > 0", i);
    double pupsum = 0.0;
    for (long i = 0; i < (long)P * P; ++i) pupsum += pup[i];
    if (pupsum == 0.0 || !std::isfinite(pupsum)) return fail(MPSFR_E_INVALID, "sum(pup) must be finite and non-zero");
    HIPCHK(hipSetDevice(c->device));
    mpsfr_ctx::P2P& w = c->p2p;
    if (!w.stream) HIPCHK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    hipStream_t s = w.stream;
    // wavelengths per chunk: the workspace is bounded whatever nl and npsd are (~50 MB per plane at 1280^2)
    constexpr int kChunk = 8;
    const int CH = std::min(nl, kChunk), nchunk = (nl + CH - 1) / CH;
    const bool phased = phase_static != nullptr;
    const int notf = phased ? CH : 1;
    const size_t H1 = (size_t)M / 2 + 1, plane = (size_t)M * M;
    int rc;
    if ((rc = ensure(c, w.twm, 2 * (size_t)M * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.psd, (size_t)N * N * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.cm, (size_t)N * (N / 2 + 1) * 2 * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.d0t, (size_t)(N / 2 + 1) * N * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.pup, (size_t)P * P * sizeof(double)))) return rc;
    if (phased && (rc = ensure(c, w.phase, (size_t)P * P * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.lbda, (size_t)nl * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.cl, (size_t)nl * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.t1, (size_t)notf * P * M * 2 * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.q, (size_t)notf * M * H1 * 2 * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.otf, (size_t)notf * H1 * M * sizeof(double)))) return rc;
    if ((rc = ensure(c, w.g, (size_t)CH * H1 * H1 * 2 * sizeof(double)))) return rc;
    if (!on_device && (rc = ensure(c, w.out, (size_t)CH * plane * sizeof(double)))) return rc;
    if (w.twm_len != M) {
        std::vector<double> tw(2 * (size_t)M);
        for (int m = 0; m < M; ++m) {
            const long double ang = -2.0L * 3.141592653589793238462643383279502884L * m / M;
            tw[2 * m] = (double)cosl(ang);
            tw[2 * m + 1] = (double)sinl(ang);
        }
        HIPCHK(hipMemcpy(w.twm.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
        w.twm_len = M;
    }
    // psfrec.py:717-722: Dphi(lambda) = (2 pi / lambda_nm)^2 Dphi0, Dphi0 = 2 Re(bg00 - bg) with bg of the raw PSD
    std::vector<double> cl(nl);
    for (int i = 0; i < nl; ++i) {
        const double conv = 2.0 * M_PI / (lbda_m[i] * 1e9);
        cl[i] = -0.5 * conv * conv;
    }
    const double L = D * N / P;                       // psfrec.py:710-711
    const double dscale = 2.0 / (L * L);
    const double oscale = 1.0 / ((double)M * M * (double)M * M * pupsum);
    HIPCHK(hipMemcpyAsync(w.pup.p, pup, (size_t)P * P * sizeof(double), hipMemcpyHostToDevice, s));
    if (phased)
        HIPCHK(hipMemcpyAsync(w.phase.p, phase_static, (size_t)P * P * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.lbda.p, lbda_m, (size_t)nl * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.cl.p, cl.data(), (size_t)nl * sizeof(double), hipMemcpyHostToDevice, s));
    const double* d_lbda = (const double*)w.lbda.p;
    const double* d_cl = (const double*)w.cl.p;
    double* d_otf = (double*)w.otf.p;
    // the OTFs: one for the call without a static phase, else one per wavelength (built once if one chunk holds them)
    auto build_otf = [&](int l0, int nz) {
        launch_p2p_otf(s, M, P, nz, (const double*)w.pup.p, phased ? (const double*)w.phase.p : nullptr,
                       d_lbda + l0, oscale, w.t1.p, w.q.p, d_otf, w.twm.p);
    };
    if (!phased || nchunk == 1) build_otf(0, phased ? CH : 1);
    const size_t otf_stride = phased ? H1 * M : 0;
    for (int p = 0; p < npsd; ++p) {
        HIPCHK(hipMemcpyAsync(w.psd.p, psd + (size_t)p * N * N, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice, s));
        launch_dphi_from_psd(s, N, 1, (const double*)w.psd.p, w.cm.p, dscale, w.d0t.p, true, c->tw64.p);
        for (int k = 0; k < nchunk; ++k) {
            const int l0 = k * CH, nz = std::min(CH, nl - l0);
            if (phased && nchunk > 1) build_otf(l0, nz);
            double* dst = psf_out + ((size_t)p * nl + l0) * plane;
            launch_p2p_psf(s, M, N, nz, (const double*)w.d0t.p, d_otf, otf_stride, d_cl + l0, w.g.p,
                           on_device ? dst : (double*)w.out.p, w.twm.p);
            HIPCHK(hipGetLastError());
            if (!on_device) {
                HIPCHK(hipMemcpyAsync(dst, w.out.p, (size_t)nz * plane * sizeof(double), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));      // (w.out is refilled by the next chunk)
            }
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return MPSFR_OK;
}

long mpsfr_debug_fetch(mpsfr_ctx* c, const char* what, double* out, size_t capacity) {
    if (!c || !what || !out) return fail(MPSFR_E_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int N = c->N, H1 = N / 2 + 1;
    size_t n = 0;
    const void* src = nullptr;
    bool is_real_r = false;   // stored in the context's R type
    if (!strcmp(what, "ao_tables")) {
        n = (size_t)2 * c->last_ndir * (c->last_ntab + 1) * NAO * NAO;
        src = c->aotab.p;
    } else if (!strcmp(what, "tel")) {
        n = (size_t)H1 * N;
        src = c->tel.p;
        is_real_r = true;
    } else if (!strcmp(what, "dphi0")) {
        n = (size_t)c->last_chunk_tasks * c->last_ndir * H1 * N;
        src = c->lane[c->last_lane].D0t.p;
        is_real_r = true;
    } else if (!strcmp(what, "dlin")) {
        if (!c->last_dlin)
            return fail(MPSFR_E_INVALID, "no line minima in the last call (prune_eps = 0, or stage A did not run in "
                                         "its series form)");
        n = (size_t)c->last_chunk_tasks * c->last_ndir * H1 * (N / 32);
        if (n > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, n);
        std::vector<float> tmp(n);
        HIPCHK(hipMemcpy(tmp.data(), c->lane[c->last_lane].dlin.p, n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) out[i] = (double)tmp[i];
        return (long)n;
    } else if (!strcmp(what, "pre")) {
        n = (size_t)c->last_chunk_tasks * c->last_gpp * c->last_nl * NS * NS;
        src = c->lane[c->last_lane].pre.p;
        is_real_r = true;
    } else if (!strcmp(what, "mf_work")) {
        // Work of the matrix-core per-wavelength kernel in the last chunk, recomputed on the host
        // from the kernel's own inputs: [0] tile steps executed (16 lines x 32 columns each),
        // [1] m-tiles with a second pass, [2] tile steps without any pruning.
        if (capacity < 3) return fail(MPSFR_E_INVALID, "capacity %zu < 3", capacity);
        if (!c->last_mf) return fail(MPSFR_E_INVALID, "the last call did not use the matrix-core kernel");
        const int tc = c->last_chunk_tasks * c->last_gpp, nl = c->last_nl, npair = (nl + 1) / 2;
        const int nks = N / 32, nmt = (H1 + 15) / 16, nb = nmt * nks;
        const mpsfr_ctx::Lane& ln = c->lane[c->last_lane];
        std::vector<int> vk((size_t)tc * npair);
        std::vector<float> dm((size_t)tc * nb), tb((size_t)nb);
        if (c->last_pruned && !c->last_mf2) {
            HIPCHK(hipMemcpy(vk.data(), ln.vkeep.p, vk.size() * sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(dm.data(), ln.dminb.p, dm.size() * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(tb.data(), c->tlb.p, tb.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
        double steps = 0.0, tiles = 0.0, steps_full = 0.0, steps_mid = 0.0, steps_union = -1.0, steps_support = -1.0;
        if (c->last_mf2) {          // the masks the thin-wave kernel ran on (K_MF_PREP)
            std::vector<unsigned long long> own((size_t)tc * nl * nmt * 2);
            HIPCHK(hipMemcpy(own.data(), ln.mown.p, own.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < own.size(); i += 2) {
                const int nf = __builtin_popcountll(own[i]), nm = __builtin_popcountll(own[i + 1]);
                steps_full += nf;
                steps_mid += nm;
                tiles += (nf + nm) > 0;
            }
            steps = steps_full + steps_mid;
            // the blocks ANY wavelength of a task keeps (what stage A has to deliver at all), and the blocks inside
            // the support of the telescope OTF
            steps_union = 0.0;
            for (int t = 0; t < tc; ++t)
                for (int mt = 0; mt < nmt; ++mt) {
                    unsigned long long u = 0;
                    for (int l = 0; l < nl; ++l) {
                        const size_t i = (((size_t)t * nl + l) * nmt + mt) * 2;
                        u |= own[i] | own[i + 1];
                    }
                    steps_union += __builtin_popcountll(u);
                }
            HIPCHK(hipMemcpy(tb.data(), c->tlb.p, tb.size() * sizeof(float), hipMemcpyDeviceToHost));
            steps_support = 0.0;
            for (size_t i = 0; i < tb.size(); ++i) steps_support += std::isfinite(tb[i]) ? 1.0 : 0.0;
            steps_support *= tc;
        } else {
        std::vector<float> thrf((size_t)tc, -1.0e30f);
        if (c->last_pruned && c->last_floor_per_task)
            HIPCHK(hipMemcpy(thrf.data(), ln.thrf.p, thrf.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int t = 0; t < tc; ++t)
            for (int l = 0; l < nl; ++l) {
                const float c2 = (float)c->last_lpc[l] * 1.44269504088896340736f;
                const float thr_t = std::fmax(c->last_thr_blk, thrf[t]);
                const int nv = c->last_pruned ? vk[(size_t)t * npair + (l >> 1)] : H1;
                for (int mt = 0; mt < (nv + 15) / 16; ++mt) {
                    int n = 0;
                    for (int ks = 0; ks < nks; ++ks)
                        n += !c->last_pruned ||
                             std::fmaf(c2, dm[((size_t)t * nmt + mt) * nks + ks], tb[mt * nks + ks]) > thr_t;
                    steps += n;
                    tiles += n > 0;
                }
            }
        steps_full = steps;
        }
        out[0] = steps;
        out[1] = tiles;
        out[2] = (double)tc * nl * nb;
        if (capacity < 5) return 3;
        out[3] = steps_full;         // tile steps with all three products (9 MFMA)
        out[4] = steps_mid;          // tile steps without the low half of the OTF (6 MFMA)
        if (capacity < 7) return 5;
        out[5] = steps_union;        // blocks kept by at least one wavelength, summed over the tasks (-1: not the thin-wave kernel)
        out[6] = steps_support;      // blocks with a non-zero telescope OTF, times the tasks
        return 7;
    } else if (!strcmp(what, "mf_clock")) {
        if (!c->mfclk.p) return fail(MPSFR_E_INVALID, "mf_clock is off");
        n = capacity < (size_t)65536 * 64 ? capacity : (size_t)65536 * 64;
        std::vector<unsigned long long> tmp(n);
        HIPCHK(hipMemcpy(tmp.data(), c->mfclk.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) out[i] = (double)tmp[i];
        return (long)n;
    } else if (!strcmp(what, "d0t_clears")) {
        if (capacity < 1) return fail(MPSFR_E_INVALID, "capacity %zu < 1", capacity);
        out[0] = (double)c->d0t_clears;
        return 1;
    } else if (!strcmp(what, "vkeep")) {
        if (!c->last_pruned || c->last_mf2)
            return fail(MPSFR_E_INVALID, "no line pruning in the last call (prune_eps = 0, or the block-masked "
                                         "matrix-core kernel ran)");
        n = (size_t)c->last_chunk_tasks * c->last_gpp * ((c->last_nl + 1) / 2);
        if (n > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, n);
        std::vector<int> tmp(n);
        HIPCHK(hipMemcpy(tmp.data(), c->lane[c->last_lane].vkeep.p, n * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) out[i] = (double)tmp[i];
        return (long)n;
    } else if (!strcmp(what, "mf_par") || !strcmp(what, "mf_own") || !strcmp(what, "mf_uni") ||
               !strcmp(what, "mf_ksum") || !strcmp(what, "mf_kuni") || !strcmp(what, "mf_gsw") ||
               !strcmp(what, "mf_sched") || !strcmp(what, "mf_items") || !strcmp(what, "tlb") ||
               !strcmp(what, "dminb") || !strcmp(what, "dblk") || !strcmp(what, "dline") || !strcmp(what, "thrf") ||
               !strcmp(what, "order")) {
        // The work plan of the per-wavelength stage in the last chunk, as its kernels read it (K_MF_PREP, K_DMIN,
        // K_VKEEP, K_TASK_ORDER, K_PEAK_FLOOR): copies only, nothing is launched or written.
        if (c->last_nl <= 0) return fail(MPSFR_E_INVALID, "no call yet");
        const mpsfr_ctx::Lane& ln = c->lane[c->last_lane];
        const int tc = c->last_chunk_tasks * c->last_gpp, ntd = c->last_chunk_tasks * c->last_ndir, nl = c->last_nl;
        const int nks = N / 32, nmt = (H1 + 15) / 16, nsw = (nmt + 7) / 8;
        int per = 0, ngr = 0;
        mf2_groups(nl, c->mf_permax, &per, &ngr);
        const bool mf2 = c->last_mf && c->last_mf2, mf1 = c->last_mf && !c->last_mf2;
        // K_DMIN / K_DMIN16 ran: always before K_VKEEP, before K_MF_PREP only without the line minima of stage A
        const bool dmin_ran = c->last_pruned && !(mf2 && c->last_dlin);
        auto put = [&](const void* dev, size_t count, auto tag) -> long {
            using T = decltype(tag);
            if (count > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, count);
            std::vector<T> tmp(count);
            if (count) HIPCHK(hipMemcpy(tmp.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < count; ++i) out[i] = (double)tmp[i];
            return (long)count;
        };
        typedef unsigned long long u64;
        if (!strcmp(what, "mf_par")) {
            n = 9 + (size_t)nl;
            if (n > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, n);
            for (int k = 0; k < 7; ++k) out[k] = (double)c->last_thr[k];
            out[7] = per;
            out[8] = ngr;
            for (int l = 0; l < nl; ++l) out[9 + l] = c->last_lpc[l];
            return (long)n;
        }
        if (!strcmp(what, "tlb")) {
            if (!c->tlb.p) return fail(MPSFR_E_INVALID, "no block maxima of the telescope OTF (otf_mfma = 0, or f64 mode)");
            return put(c->tlb.p, (size_t)nmt * nks, float());
        }
        if (!strncmp(what, "mf_", 3)) {
            if (!mf2) return fail(MPSFR_E_INVALID, "the last call did not use the thin-wave matrix-core kernel");
            const u64* uni = (const u64*)ln.muni.p;
            const u64* ksum = uni + (size_t)tc * nl * nmt;
            const u64* kuni = ksum + (size_t)tc * nl * nsw;
            const int* sched = (const int*)ln.msched.p;
            const int* gsw = sched + 68;
            if (!strcmp(what, "mf_own")) return put(ln.mown.p, (size_t)tc * nl * nmt * 2, u64());
            if (!strcmp(what, "mf_uni")) return put(uni, (size_t)tc * ngr * nmt, u64());
            if (!strcmp(what, "mf_ksum")) return put(ksum, (size_t)tc * nl * nsw, u64());
            if (!strcmp(what, "mf_kuni")) return put(kuni, (size_t)tc * ngr * nsw, u64());
            if (!strcmp(what, "mf_gsw")) return put(gsw, (size_t)tc * ngr, int());
            if (!strcmp(what, "mf_sched")) return put(sched, (size_t)kMfLists, int());
            // mf_items: the filled part of every list, (class, task, grp, sweep, sweeps) per item
            int len[kMfLists];
            HIPCHK(hipMemcpy(len, sched, sizeof(len), hipMemcpyDeviceToHost));
            const size_t cap = (size_t)tc * ngr * nsw;
            const int* items = sched + 68 + (((size_t)tc * nl + 3) & ~(size_t)3);
            for (int k = 0; k < kMfLists; ++k) {
                if (len[k] < 0 || (size_t)len[k] > cap) return fail(MPSFR_E_INVALID, "work list %d holds %d items of at most %zu", k, len[k], cap);
                n += (size_t)len[k];
            }
            if (5 * n > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, 5 * n);
            std::vector<int> tmp;
            size_t o = 0;
            for (int k = 0; k < kMfLists; ++k) {
                if (!len[k]) continue;
                tmp.resize((size_t)4 * len[k]);
                HIPCHK(hipMemcpy(tmp.data(), items + (size_t)k * cap * 4, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
                for (int i = 0; i < len[k]; ++i, o += 5) {
                    out[o] = k;
                    for (int j = 0; j < 4; ++j) out[o + 1 + j] = tmp[(size_t)4 * i + j];
                }
            }
            return (long)(5 * n);
        }
        if (!strcmp(what, "dminb")) {
            // one direction and the thin-wave kernel: the block minima of K_DMIN are the minima over the directions
            if (mf2 && dmin_ran) return put(ln.dblk.p, (size_t)tc * nmt * nks, float());
            if (mf1 && c->last_pruned) return put(ln.dminb.p, (size_t)tc * nmt * nks, float());
            return fail(MPSFR_E_INVALID, "no block minima over the directions in the last call (prune_eps = 0, the "
                                         "FFT form, or the thin-wave kernel on the line minima of stage A)");
        }
        if (!strcmp(what, "dblk") || !strcmp(what, "dline")) {
            if (!dmin_ran)
                return fail(MPSFR_E_INVALID, "no minima per direction in the last call (prune_eps = 0, or the thin-wave "
                                             "kernel on the line minima of stage A)");
            if (!strcmp(what, "dblk")) return put(ln.dblk.p, (size_t)ntd * nmt * nks, float());
            return put(ln.dmin.p, (size_t)ntd * H1, float());
        }
        if (!strcmp(what, "thrf")) {
            if (!(mf1 && c->last_pruned && c->last_floor_per_task))
                return fail(MPSFR_E_INVALID, "no floor per task in the last call (the kernel for several directions "
                                             "with a finite tier_eps > 0 writes it)");
            return put(ln.thrf.p, (size_t)tc, float());
        }
        if (!(mf1 && c->last_pruned))
            return fail(MPSFR_E_INVALID, "no task order in the last call (mf_kernel = 1 or several directions, "
                                         "prune_eps > 0)");
        return put(ln.order.p, (size_t)tc, int());
    } else {
        return fail(MPSFR_E_INVALID, "unknown buffer '%s'", what);
    }
    if (n == 0 || !src) return fail(MPSFR_E_INVALID, "buffer '%s' is empty", what);
    if (n > capacity) return fail(MPSFR_E_INVALID, "capacity %zu < %zu", capacity, n);
    if (is_real_r && !c->f64) {
        std::vector<float> tmp(n);
        HIPCHK(hipMemcpy(tmp.data(), src, n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) out[i] = (double)tmp[i];
    } else {
        HIPCHK(hipMemcpy(out, src, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return (long)n;
}

void* mpsfr_stream(mpsfr_ctx* c) {
    if (!c) return nullptr;
    if (!c->stream_exported) {
        // from now on every call joins its lanes into the stream; what is already queued joins here
        c->stream_exported = true;
        (void)hipSetDevice(c->device);
        for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
            if (c->lane[k].busy) (void)hipStreamWaitEvent(c->stream, lane_end(c, c->lane[k]), 0);
    }
    return (void*)c->stream;
}

int mpsfr_stream_wait(mpsfr_ctx* c, void* caller_stream) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t cs = (hipStream_t)caller_stream;
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
        if (c->lane[k].busy) HIPCHK(hipStreamWaitEvent(cs, lane_end(c, c->lane[k]), 0));
    // (host-output and multi-lane calls finish on the context's stream: the lane sums, the copies)
    if (c->stream_tail) {
        HIPCHK(hipEventRecord(c->stream_tail, c->stream));
        HIPCHK(hipStreamWaitEvent(cs, c->stream_tail, 0));
    }
    return MPSFR_OK;
}

int mpsfr_profile_count(void) { return K_COUNT; }

const char* mpsfr_profile_name(int id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : ""; }

int mpsfr_profile_get(mpsfr_ctx* c, int id, double* total_ms, long* launches) {
    if (!c || id < 0 || id >= K_COUNT) return fail(MPSFR_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    const int rc = resolve_profile(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->prof_ms[id];
    if (launches) *launches = c->prof_n[id];
    return MPSFR_OK;
}

int mpsfr_host_time(mpsfr_ctx* c, double* seconds, long* calls) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    if (seconds) *seconds = c->host_seconds;
    if (calls) *calls = c->host_calls;
    return MPSFR_OK;
}

int mpsfr_profile_reset(mpsfr_ctx* c) {
    if (!c) return fail(MPSFR_E_INVALID, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    const int rc = resolve_profile(c);
    if (rc) return rc;
    c->host_seconds = 0.0;
    c->host_calls = 0;
    for (int i = 0; i < K_COUNT; ++i) {
        c->prof_ms[i] = 0.0;
        c->prof_n[i] = 0;
    }
    return MPSFR_OK;
}

}  // extern "C"
