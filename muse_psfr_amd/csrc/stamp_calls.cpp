// The stamp, frame and cube entry points of include/mpsfr.h: argument checks, then one staged call on the context stream.
#include <algorithm>
#include <cmath>

#include "host_ctx.h"
#include "stage_layout.h"

using namespace mpsfr;
using namespace mpsfr::host;

namespace {

// The arrays of one stamp, frame or cube call (the fits and the metrics of caller-provided stamps, the frame calls).  An
// entry point declares them with in() and out() in the order of the call and gets typed handles; a handle converts to
// the array's device pointer: the caller's own pointer when on_device, else its place in c->stage (StageLayout, where
// an absent optional gets no room), and NULL for an absent one either way.  Nothing is allocated per call.
class Staged {
public:
    template <class T> struct Ptr {
        const Staged* st;
        int k;
        operator T*() const { return static_cast<T*>(st->device(k)); }
    };
    template <class T> using In = Ptr<const T>;
    template <class T> using Out = Ptr<T>;
    Staged(mpsfr_ctx* ctx, int device_pointers) : c(ctx), on_device(device_pointers != 0) {}
    template <class T> In<T> in(const T* p, size_t count) { return {this, add(const_cast<T*>(p), count, sizeof(T), false)}; }
    template <class T> Out<T> out(T* p, size_t count) { return {this, add(p, count, sizeof(T), true)}; }

    // The call on the context stream, after the lanes, timed under the fit's profiling id: launch(s) with the handles.
    // on_device: it returns once it is queued.  Else the inputs are copied into c->stage in the order of their
    // declaration, the outputs are copied back and the call waits for them.
    template <class Launch>
    int run(Launch launch) {
        HIPCHK(hipSetDevice(c->device));
        hipStream_t s = c->stream;
        if (int rc = wait_for_lanes(c, s)) return rc;
        if (!on_device) {
            if (int rc = place()) return rc;
            for (int k = 0; k < lay.n; ++k)
                if (ptr[k] && !lay.a[k].output)
                    HIPCHK(hipMemcpyAsync(device(k), ptr[k], lay.a[k].bytes, hipMemcpyHostToDevice, s));
        }
        {
            ProfScope ps(c, K_FIT);
            launch(s);
        }
        HIPCHK(hipGetLastError());
        if (!on_device) {
            for (int k = 0; k < lay.n; ++k)
                if (ptr[k] && lay.a[k].output)
                    HIPCHK(hipMemcpyAsync(ptr[k], device(k), lay.a[k].bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        return MPSFR_OK;
    }

    // For a call that copies by itself (mpsfr_fit_cube_psf, batch by batch): room in c->stage for the declared arrays,
    // the total rounded up to `align` bytes; then copies of `count` elements into an input and out of an output.
    int place(size_t align = 1) {
        const int rc = ensure(c, c->stage, (lay.place() + align - 1) / align * align);
        base = static_cast<char*>(c->stage.p);
        return rc;
    }
    template <class T> void* address(Ptr<T> h) const { return device(h.k); }
    template <class T> hipError_t put(In<T> h, const T* src, size_t count) const {
        return hipMemcpyAsync(device(h.k), src, count * sizeof(T), hipMemcpyHostToDevice, c->stream);
    }
    template <class T> hipError_t get(T* dst, Out<T> h, size_t count) const {
        return hipMemcpyAsync(dst, device(h.k), count * sizeof(T), hipMemcpyDeviceToHost, c->stream);
    }

private:
    int add(void* p, size_t count, size_t elem, bool output) {
        ptr[lay.n] = p;
        return lay.add(p != nullptr, count, elem, output);
    }
    void* device(int k) const { return on_device || !ptr[k] ? ptr[k] : base + lay.a[k].offset; }
    mpsfr_ctx* c;
    bool on_device;
    StageLayout lay;
    void* ptr[StageLayout::kMaxArrays];      // the caller's arrays
    char* base = nullptr;
};

// The host form's refusal of a model list: every psf_index (n of them, or nullptr) in 0..npsf-1, then every one of the
// nshift shifts (or nullptr) finite and within 8 pixels; `what` is the caller's noun for a shift.
int check_model_list(const char* who, const char* what, int n, int npsf, const int32_t* psf_index, const double* shift,
                     size_t nshift) {
    if (psf_index)
        for (int k = 0; k < n; ++k)
            if (psf_index[k] < 0 || psf_index[k] >= npsf)
                return fail(MPSFR_E_INVALID, "%s: a psf_index outside 0..npsf-1", who);
    if (shift)
        for (size_t k = 0; k < nshift; ++k)
            if (!(std::fabs(shift[k]) <= MPSFR_FIT_PSF_MAX_SHIFT))
                return fail(MPSFR_E_INVALID, "%s: a %s that is not finite or beyond 8 pixels", who, what);
    return MPSFR_OK;
}

// ... and of the stars of a frame: finite scales (or nullptr), then origins within 2^30
int check_frame_stars(const char* who, int n, const int32_t* origin, const double* scale, const char* scale_name) {
    if (scale)
        for (int k = 0; k < n; ++k)
            if (!std::isfinite(scale[k])) return fail(MPSFR_E_INVALID, "%s: a %s that is not finite", who, scale_name);
    for (size_t k = 0; k < (size_t)2 * n; ++k)
        if (origin[k] < -(1 << 30) || origin[k] > (1 << 30)) return fail(MPSFR_E_INVALID, "%s: an origin beyond 2^30", who);
    return MPSFR_OK;
}

}  // namespace

extern "C" {

int mpsfr_fit_rows(const double* fit, long n, double pixscale, double* out, long stride) {
    if (!fit || !out || n < 0 || stride < 14) return fail(MPSFR_E_INVALID, "mpsfr_fit_rows: bad argument");
    for (long r = 0; r < n; ++r) {
        const double* f = fit + (size_t)r * NFIT;
        double* o = out + (size_t)r * stride;
        o[0] = f[1];                     // center
        o[1] = f[2];
        o[2] = f[15];                    // flux
        o[3] = o[4] = f[5] * pixscale;   // fwhm
        o[5] = f[4];                     // n
        o[6] = f[0];                     // peak
        o[7] = f[9];                     // err_center
        o[8] = f[10];
        const double a = f[8] / f[0], b = 2.0 * f[11] / f[3], d = f[12] / (f[4] - 1.0);
        o[9] = std::fabs(f[15]) * std::sqrt(a * a + b * b + d * d);      // err_flux
        o[10] = o[11] = f[13] * pixscale;                                // err_fwhm
        o[12] = f[12];                   // err_n
        o[13] = f[8];                    // err_peak
    }
    return MPSFR_OK;
}

int mpsfr_fit_stamps(mpsfr_ctx* c, int nstamp, const double* stamps, double* fit_out, int on_device) {
    if (!c || !stamps || !fit_out || nstamp < 1) return fail(MPSFR_E_INVALID, "bad argument");
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix);
    auto fit = st.out(fit_out, (size_t)nstamp * NFIT);
    return st.run([&](hipStream_t s) { launch_fit(s, nstamp, sp, false, fit, c->f64); });
}

int mpsfr_fit_stamps_elliptical(mpsfr_ctx* c, int nstamp, const double* stamps, double* fit_out, int on_device) {
    if (!c || !stamps || !fit_out || nstamp < 1) return fail(MPSFR_E_INVALID, "bad argument");
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix);
    auto fit = st.out(fit_out, (size_t)nstamp * NFIT_ELL);
    return st.run([&](hipStream_t s) { launch_fit_ell(s, nstamp, sp, fit, c->f64); });
}

int mpsfr_fit_stamps_observed(mpsfr_ctx* c, int nstamp, const double* stamps, const double* var, int flags,
                              double* fit_out, int on_device) {
    if (!c || !stamps || !fit_out || nstamp < 1) return fail(MPSFR_E_INVALID, "bad argument");
    if (flags & ~(MPSFR_FIT_BACKGROUND | MPSFR_FIT_ELLIPTICAL))
        return fail(MPSFR_E_INVALID, "fit_stamps_observed: unknown flag bits");
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix), va = st.in(var, nstamp * kStampPix);
    auto fit = st.out(fit_out, (size_t)nstamp * NFIT_ELL);
    return st.run([&](hipStream_t s) { launch_fit_obs(s, nstamp, sp, va, flags, fit, c->f64); });
}

static_assert(NFIT_PSF == MPSFR_NFIT_PSF, "K_FIT_PSF row layout");

int mpsfr_fit_stamps_psf(mpsfr_ctx* c, int nstamp, const double* stamps, const double* var, int npsf,
                         const double* psf, const int32_t* psf_index, const double* shift, int flags,
                         double* fit_out, int on_device) {
    if (!c || !stamps || !psf || !fit_out || nstamp < 1 || npsf < 1) return fail(MPSFR_E_INVALID, "bad argument");
    if (flags & ~(MPSFR_FIT_BACKGROUND | MPSFR_FIT_FIXED_SHIFT))
        return fail(MPSFR_E_INVALID, "fit_stamps_psf: unknown flag bits (the elliptical bit has no meaning here)");
    if (!psf_index && npsf != nstamp)
        return fail(MPSFR_E_INVALID, "fit_stamps_psf: without psf_index, npsf must equal nstamp");
    if ((flags & MPSFR_FIT_FIXED_SHIFT) && !shift)
        return fail(MPSFR_E_INVALID, "fit_stamps_psf: MPSFR_FIT_FIXED_SHIFT needs the shift array");
    int rc;
    if (!on_device &&
        (rc = check_model_list("fit_stamps_psf", "shift", nstamp, npsf, psf_index, shift, (size_t)2 * nstamp)))
        return rc;
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix), va = st.in(var, nstamp * kStampPix), ps = st.in(psf, npsf * kStampPix);
    auto sh = st.in(shift, (size_t)2 * nstamp);
    auto pi = st.in(psf_index, (size_t)nstamp);
    auto fit = st.out(fit_out, (size_t)nstamp * NFIT_PSF);
    return st.run([&](hipStream_t s) { launch_fit_psf(s, nstamp, sp, va, npsf, ps, pi, sh, flags, fit, c->f64); });
}

static_assert(NFIT_GROUP == MPSFR_NFIT_GROUP && MPSFR_NFIT_GROUP == 8 + 8 * MPSFR_MAX_GROUP + 8, "K_FIT_GROUP row layout");

int mpsfr_fit_groups_psf(mpsfr_ctx* c, int nstamp, int nsrc, const double* stamps, const double* var, int npsf,
                         const double* psf, const int32_t* psf_index, const double* shift, int flags,
                         double* fit_out, int on_device) {
    if (!c || !stamps || !psf || !shift || !fit_out || nstamp < 1 || npsf < 1)
        return fail(MPSFR_E_INVALID, "fit_groups_psf: bad argument (stamps, psf, shift and fit_out are required)");
    if (nsrc == 1)
        return fail(MPSFR_E_INVALID, "fit_groups_psf: a group has 2 to %d sources; one source is mpsfr_fit_stamps_psf",
                    MPSFR_MAX_GROUP);
    if (nsrc < 2 || nsrc > MPSFR_MAX_GROUP)
        return fail(MPSFR_E_INVALID, "fit_groups_psf: nsrc=%d outside 2..%d", nsrc, MPSFR_MAX_GROUP);
    if (flags & ~(MPSFR_FIT_BACKGROUND | MPSFR_FIT_FIXED_SHIFT | MPSFR_FIT_COMMON_SHIFT))
        return fail(MPSFR_E_INVALID, "fit_groups_psf: unknown flag bits (the elliptical bit has no meaning here)");
    if ((flags & MPSFR_FIT_FIXED_SHIFT) && (flags & MPSFR_FIT_COMMON_SHIFT))
        return fail(MPSFR_E_INVALID, "fit_groups_psf: MPSFR_FIT_FIXED_SHIFT and MPSFR_FIT_COMMON_SHIFT exclude each other");
    if (!psf_index && npsf != nstamp)
        return fail(MPSFR_E_INVALID, "fit_groups_psf: without psf_index, npsf must equal nstamp");
    const size_t npos = (size_t)2 * nsrc * nstamp;
    int rc;
    if (!on_device && (rc = check_model_list("fit_groups_psf", "position", nstamp, npsf, psf_index, shift, npos)))
        return rc;
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix), va = st.in(var, nstamp * kStampPix), ps = st.in(psf, npsf * kStampPix);
    auto sh = st.in(shift, npos);
    auto pi = st.in(psf_index, (size_t)nstamp);
    auto fit = st.out(fit_out, (size_t)nstamp * NFIT_GROUP);
    return st.run([&](hipStream_t s) { launch_fit_group(s, nstamp, nsrc, sp, va, npsf, ps, pi, sh, flags, fit, c->f64); });
}

int mpsfr_fit_spectra_psf(mpsfr_ctx* c, int nstar, int nl, const double* cubes, const double* var, int npsf,
                          const double* psf, const int32_t* psf_index, const double* shift, const double* x,
                          int flags, double* fit_out, int on_device) {
    if (!c || !cubes || !psf || !fit_out || nstar < 1 || npsf < 1)
        return fail(MPSFR_E_INVALID, "fit_spectra_psf: bad argument (cubes, psf and fit_out are required)");
    if (nl < 1 || nl > MPSFR_MAX_SPEC_LAYERS)
        return fail(MPSFR_E_INVALID, "fit_spectra_psf: nl=%d outside 1..%d", nl, MPSFR_MAX_SPEC_LAYERS);
    if (flags & ~(MPSFR_FIT_BACKGROUND | MPSFR_FIT_DRIFT))
        return fail(MPSFR_E_INVALID, "fit_spectra_psf: unknown flag bits (only the background and the drift bit have a meaning here)");
    if (!psf_index && npsf != nstar)
        return fail(MPSFR_E_INVALID, "fit_spectra_psf: without psf_index, npsf must equal nstar");
    const bool drift = (flags & MPSFR_FIT_DRIFT) != 0;
    if (drift) {
        if (!x || nl < 2) return fail(MPSFR_E_INVALID, "fit_spectra_psf: MPSFR_FIT_DRIFT needs x and at least two layers");
        bool differ = false;
        for (int l = 0; l < nl; ++l) {
            if (!(std::fabs(x[l]) <= 1.0)) return fail(MPSFR_E_INVALID, "fit_spectra_psf: x must be finite in [-1, 1]");
            differ = differ || x[l] != x[0];
        }
        if (!differ) return fail(MPSFR_E_INVALID, "fit_spectra_psf: at least two values of x must differ");
    }
    int rc;
    if (!on_device && (rc = check_model_list("fit_spectra_psf", "start", nstar, npsf, psf_index, shift, (size_t)2 * nstar)))
        return rc;
    const double* d_x = nullptr;
    if (drift) {           // x is the host's in both forms: into a buffer of the context, on the stream of the call
        HIPCHK(hipSetDevice(c->device));
        if ((rc = ensure(c, c->specx, (size_t)nl * sizeof(double)))) return rc;
        HIPCHK(hipMemcpyAsync(c->specx.p, x, (size_t)nl * sizeof(double), hipMemcpyHostToDevice, c->stream));
        d_x = (const double*)c->specx.p;
    }
    const size_t ncube = (size_t)nl * kStampPix;
    Staged st(c, on_device);
    auto cu = st.in(cubes, nstar * ncube), va = st.in(var, nstar * ncube), ps = st.in(psf, npsf * ncube);
    auto sh = st.in(shift, (size_t)2 * nstar);
    auto pi = st.in(psf_index, (size_t)nstar);
    auto fit = st.out(fit_out, (size_t)nstar * (MPSFR_NFIT_SPEC + (size_t)MPSFR_NFIT_SPEC_LAYER * nl));
    return st.run([&](hipStream_t s) { launch_fit_spec(s, nstar, nl, cu, va, npsf, ps, pi, sh, d_x, flags, fit, c->f64); });
}

static_assert(METRIC_MAX == MPSFR_MAX_METRIC_RADII && METRIC_HEAD == MPSFR_NMET_HEAD, "K_STAMP_METRICS row layout");

int mpsfr_stamp_metrics(mpsfr_ctx* c, int nstamp, const double* stamps, const double* centers, int nrad,
                        const double* radii_px, int nbox, const double* boxes_px, int nfrac, const double* fractions,
                        double* out, int on_device) {
    if (!c || !stamps || !out || nstamp < 1) return fail(MPSFR_E_INVALID, "bad argument");
    if (nrad < 0 || nrad > METRIC_MAX || nbox < 0 || nbox > METRIC_MAX || nfrac < 0 || nfrac > METRIC_MAX ||
        nrad + nbox + nfrac == 0)
        return fail(MPSFR_E_INVALID, "metrics: need 0..16 radii, boxes and fractions, and at least one of them");
    if ((nrad && !radii_px) || (nbox && !boxes_px) || (nfrac && !fractions))
        return fail(MPSFR_E_INVALID, "metrics: NULL parameter array");
    for (int k = 0; k < nrad; ++k)
        if (!(radii_px[k] > 0.0 && radii_px[k] <= 2.0 * NS))
            return fail(MPSFR_E_INVALID, "metrics: a radius must be finite, > 0 and at most 80 pixels");
    for (int k = 0; k < nbox; ++k)
        if (!(boxes_px[k] > 0.0 && boxes_px[k] <= 2.0 * NS))
            return fail(MPSFR_E_INVALID, "metrics: a box side must be finite, > 0 and at most 80 pixels");
    for (int k = 0; k < nfrac; ++k)
        if (!(fractions[k] > 0.0 && fractions[k] < 1.0))
            return fail(MPSFR_E_INVALID, "metrics: a fraction must lie in (0, 1)");
    Staged st(c, on_device);
    auto sp = st.in(stamps, nstamp * kStampPix), ce = st.in(centers, (size_t)2 * nstamp);
    auto rows = st.out(out, (size_t)nstamp * (METRIC_HEAD + nrad + nbox + nfrac));
    return st.run([&](hipStream_t s) {
        launch_stamp_metrics(s, nstamp, sp, ce, nrad, radii_px, nbox, boxes_px, nfrac, fractions, rows);
    });
}

static_assert(MPSFR_NRENDER == 4 && MPSFR_FIT_PSF_MAX_SHIFT == 8.0, "K_RENDER_PREPARE row layout and domain");

static int frame_shape(const char* who, int ny, int nx) {
    if (ny < 1 || ny > MPSFR_MAX_IMAGE_SIDE || nx < 1 || nx > MPSFR_MAX_IMAGE_SIDE || (size_t)ny * nx > ((size_t)1 << 26))
        return fail(MPSFR_E_INVALID, "%s: a frame has 1..%d rows and columns and at most 2^26 pixels, not %d x %d", who,
                    MPSFR_MAX_IMAGE_SIDE, ny, nx);
    return MPSFR_OK;
}

int mpsfr_cut_stamps(mpsfr_ctx* c, int ny, int nx, const double* image, const double* var, int nstar,
                     const int32_t* origin, double* stamps_out, double* var_out, int on_device) {
    if (!c || !image || !origin || !stamps_out || nstar < 1)
        return fail(MPSFR_E_INVALID, "cut_stamps: bad argument (image, origin and stamps_out are required)");
    int rc;
    if ((rc = frame_shape("cut_stamps", ny, nx))) return rc;
    if ((var == nullptr) != (var_out == nullptr))
        return fail(MPSFR_E_INVALID, "cut_stamps: var and var_out must both be NULL or both be given");
    const size_t npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto im = st.in(image, npix), va = st.in(var, npix);
    auto og = st.in(origin, (size_t)2 * nstar);
    auto so = st.out(stamps_out, nstar * kStampPix), vo = st.out(var_out, nstar * kStampPix);
    return st.run([&](hipStream_t s) { launch_cut_stamps(s, ny, nx, im, va, nstar, og, so, vo); });
}

int mpsfr_render_stars(mpsfr_ctx* c, int ny, int nx, const double* image_in, int nstar, int npsf, const double* psf,
                       const int32_t* psf_index, const int32_t* origin, const double* shift, const double* scale,
                       int flags, double* image_out, double* star_out, int on_device) {
    if (!c || !psf || !origin || !scale || !image_out || nstar < 1 || npsf < 1)
        return fail(MPSFR_E_INVALID, "render_stars: bad argument (psf, origin, scale and image_out are required)");
    int rc;
    if ((rc = frame_shape("render_stars", ny, nx))) return rc;
    if (flags & ~MPSFR_RENDER_SUBTRACT) return fail(MPSFR_E_INVALID, "render_stars: unknown flag bits");
    if ((flags & MPSFR_RENDER_SUBTRACT) && !image_in)
        return fail(MPSFR_E_INVALID, "render_stars: MPSFR_RENDER_SUBTRACT needs image_in");
    if (!psf_index && npsf != nstar)
        return fail(MPSFR_E_INVALID, "render_stars: without psf_index, npsf must equal nstar");
    if (!on_device) {
        if ((rc = check_model_list("render_stars", "shift", nstar, npsf, psf_index, shift, (size_t)2 * nstar))) return rc;
        if ((rc = check_frame_stars("render_stars", nstar, origin, scale, "scale"))) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->render, render_workspace_bytes(ny, nx, nstar)))) return rc;
    const size_t npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto im = st.in(image_in, npix), ps = st.in(psf, npsf * kStampPix);
    auto sh = st.in(shift, (size_t)2 * nstar), sc = st.in(scale, (size_t)nstar);
    auto og = st.in(origin, (size_t)2 * nstar), pi = st.in(psf_index, (size_t)nstar);
    auto io = st.out(image_out, npix), rows = st.out(star_out, (size_t)nstar * MPSFR_NRENDER);
    return st.run([&](hipStream_t s) {
        const bool subtract = (flags & MPSFR_RENDER_SUBTRACT) != 0;
        launch_render_stars(s, ny, nx, im, StarList{nstar, npsf, ps, pi, og, sh}, sc, subtract, io, rows, c->render.p);
    });
}

static_assert(MPSFR_NFIND == 8 && MPSFR_FIND_MAX_HALF <= NS / 2, "K_FIND_ROWS row layout and the core");

int mpsfr_find_stars(mpsfr_ctx* c, int ny, int nx, const double* image, const double* var, const double* psf, int half,
                     int sep, double threshold, int max_stars, double* star_out, int32_t* origin_out,
                     int32_t* count_out, double* map_out, int on_device) {
    if (!c || !image || !psf || !star_out || !count_out)
        return fail(MPSFR_E_INVALID, "find_stars: bad argument (image, psf, star_out and count_out are required)");
    int rc;
    if ((rc = frame_shape("find_stars", ny, nx))) return rc;
    if (half < 1 || half > MPSFR_FIND_MAX_HALF || half > NS / 2)
        return fail(MPSFR_E_INVALID, "find_stars: half=%d outside 1..%d", half, MPSFR_FIND_MAX_HALF);
    if (sep < 1 || sep > MPSFR_FIND_MAX_SEP)
        return fail(MPSFR_E_INVALID, "find_stars: sep=%d outside 1..%d", sep, MPSFR_FIND_MAX_SEP);
    if (max_stars < 1 || max_stars > (1 << 24))
        return fail(MPSFR_E_INVALID, "find_stars: max_stars=%d outside 1..2^24", max_stars);
    if (!std::isfinite(threshold)) return fail(MPSFR_E_INVALID, "find_stars: threshold is not finite");
    if (!on_device) {
        bool differ = false;
        const double* core = psf + (NS / 2 - half) * NS + (NS / 2 - half);
        for (int a = 0; a <= 2 * half; ++a)
            for (int b = 0; b <= 2 * half; ++b) {
                if (!std::isfinite(core[a * NS + b]))
                    return fail(MPSFR_E_INVALID, "find_stars: psf has a value that is not finite in its core");
                differ = differ || core[a * NS + b] != core[0];
            }
        if (!differ) return fail(MPSFR_E_INVALID, "find_stars: psf is constant over its core");
    }
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->find, find_workspace_bytes(ny, nx, max_stars, map_out != nullptr)))) return rc;
    const size_t npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto im = st.in(image, npix), va = st.in(var, npix), ps = st.in(psf, kStampPix);
    auto rows = st.out(star_out, (size_t)max_stars * MPSFR_NFIND), map = st.out(map_out, npix);
    auto og = st.out(origin_out, (size_t)2 * max_stars), count = st.out(count_out, 1);
    return st.run([&](hipStream_t s) {
        launch_find_stars(s, ny, nx, im, va, ps, half, sep, threshold, max_stars, rows, og, count, map, c->find.p);
    });
}

static_assert(MPSFR_NBACK == 8 && MPSFR_NBACK_HEAD == 4 && MPSFR_BACKGROUND_MAX_BOX == 64 && MPSFR_BACK_FILLED == 1 &&
                  MPSFR_BACK_CLIP_CAP == 2 && MPSFR_BACK_FLAT == 4,
              "k_bg_cell row layout, the keys of a cell in LDS and the flags");

int mpsfr_frame_background(mpsfr_ctx* c, int nl, int ny, int nx, const double* image, const double* var, int box,
                           int filter, double kappa, int max_clip, double min_frac, const double* apply_to,
                           double* mesh_out, double* head_out, double* map_out, double* rms_out, double* applied_out,
                           int on_device) {
    const char* who = "frame_background";
    if (!c || !image || !mesh_out || !head_out)
        return fail(MPSFR_E_INVALID, "%s: bad argument (image, mesh_out and head_out are required)", who);
    int rc;
    if ((rc = frame_shape(who, ny, nx))) return rc;
    if (nl < 1 || (size_t)nl * ny * nx > ((size_t)1 << 26))
        return fail(MPSFR_E_INVALID, "%s: 1 or more layers of at most 2^26 pixels in total, not %d x %d x %d", who, nl, ny,
                    nx);
    if (box < MPSFR_BACKGROUND_MIN_BOX || box > MPSFR_BACKGROUND_MAX_BOX)
        return fail(MPSFR_E_INVALID, "%s: box=%d outside %d..%d", who, box, MPSFR_BACKGROUND_MIN_BOX,
                    MPSFR_BACKGROUND_MAX_BOX);
    if (filter != 1 && filter != 3 && filter != 5)
        return fail(MPSFR_E_INVALID, "%s: filter=%d is not 1, 3 or 5", who, filter);
    if (!(kappa >= 1.0 && kappa <= 100.0)) return fail(MPSFR_E_INVALID, "%s: kappa must be finite, in 1..100", who);
    if (max_clip < 0 || max_clip > MPSFR_BACKGROUND_MAX_CLIP)
        return fail(MPSFR_E_INVALID, "%s: max_clip=%d outside 0..%d", who, max_clip, MPSFR_BACKGROUND_MAX_CLIP);
    if (!(min_frac > 0.0 && min_frac <= 1.0)) return fail(MPSFR_E_INVALID, "%s: min_frac must lie in (0, 1]", who);
    if ((apply_to == nullptr) != (applied_out == nullptr))
        return fail(MPSFR_E_INVALID, "%s: apply_to and applied_out must both be NULL or both be given", who);
    if (applied_out && applied_out == image) return fail(MPSFR_E_INVALID, "%s: applied_out may not be image", who);
    const double kc = kappa * 1.4826;
    const size_t npix = (size_t)nl * ny * nx;
    const size_t ncell = (size_t)nl * ((ny + box - 1) / box) * ((nx + box - 1) / box);
    Staged st(c, on_device);
    auto im = st.in(image, npix), va = st.in(var, npix), ap = st.in(apply_to, npix);
    auto mesh = st.out(mesh_out, ncell * MPSFR_NBACK), head = st.out(head_out, (size_t)nl * MPSFR_NBACK_HEAD);
    auto map = st.out(map_out, npix), rms = st.out(rms_out, npix), ao = st.out(applied_out, npix);
    return st.run([&](hipStream_t s) {
        launch_frame_background(s, nl, ny, nx, im, va, box, filter, kc, max_clip, min_frac, ap, mesh, head, map, rms, ao);
    });
}

static_assert(MPSFR_NGROUP == 8 && MPSFR_MAX_GROUP == 4 && MPSFR_GROUP_MAX_CRIT == 2.0 * MPSFR_FIT_PSF_MAX_SHIFT,
              "K_GROUP_ROWS row layout, the member slots and the cell side");

int mpsfr_group_stars(mpsfr_ctx* c, int ny, int nx, int nstar, const double* pos, int stride, double crit,
                      int max_groups, int32_t* label_out, int32_t* group_out, int32_t* origin_out, double* shift_out,
                      int32_t* count_out, int on_device) {
    if (!c || !pos || !label_out || !group_out || !count_out)
        return fail(MPSFR_E_INVALID, "group_stars: bad argument (pos, label_out, group_out and count_out are required)");
    int rc;
    if ((rc = frame_shape("group_stars", ny, nx))) return rc;
    if (nstar < 1 || nstar > (1 << 24)) return fail(MPSFR_E_INVALID, "group_stars: nstar=%d outside 1..2^24", nstar);
    if (stride < 2) return fail(MPSFR_E_INVALID, "group_stars: stride=%d below 2", stride);
    if (!(crit > 0.0 && crit <= MPSFR_GROUP_MAX_CRIT))
        return fail(MPSFR_E_INVALID, "group_stars: crit must be finite, > 0 and at most %g pixels", MPSFR_GROUP_MAX_CRIT);
    if (max_groups < 1) return fail(MPSFR_E_INVALID, "group_stars: max_groups=%d below 1", max_groups);
    if ((origin_out == nullptr) != (shift_out == nullptr))
        return fail(MPSFR_E_INVALID, "group_stars: origin_out and shift_out must both be NULL or both be given");
    if (!on_device)
        for (int k = 0; k < nstar; ++k) {
            const double y = pos[(size_t)k * stride], x = pos[(size_t)k * stride + 1];
            if (std::isnan(y) || std::isnan(x)) continue;
            if (!(y >= -1.0 && y <= (double)ny && x >= -1.0 && x <= (double)nx))
                return fail(MPSFR_E_INVALID, "group_stars: a position outside [-1, ny] x [-1, nx]");
        }
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->group, group_workspace_bytes(ny, nx, nstar, max_groups)))) return rc;
    Staged st(c, on_device);
    auto po = st.in(pos, (size_t)nstar * stride);
    auto sh = st.out(shift_out, (size_t)max_groups * 8);
    auto label = st.out(label_out, (size_t)nstar), group = st.out(group_out, (size_t)max_groups * MPSFR_NGROUP);
    auto og = st.out(origin_out, (size_t)2 * max_groups), count = st.out(count_out, 6);
    return st.run([&](hipStream_t s) {
        launch_group_stars(s, ny, nx, nstar, po, stride, crit, max_groups, label, group, og, sh, count, c->group.p);
    });
}

static_assert(MPSFR_NFRAMEFIT == 8 && MPSFR_FRAME_FIT_MAX_RADIUS + MPSFR_FIT_PSF_MAX_SHIFT + 2.0 <= NS / 2 + 10.0,
              "K_FRAME_FIT row layout; a disc stays inside its footprint at any legal shift");

// what mpsfr_fit_frame_psf and mpsfr_fit_cube_psf refuse alike, whatever the pointers are: shape, counts, parameters
static int frame_fit_ranges(const char* who, int ny, int nx, int nstar, int npsf, const int32_t* psf_index, double radius,
                            int flags, int max_iter, double tol) {
    int rc;
    if ((rc = frame_shape(who, ny, nx))) return rc;
    if (nstar < 1 || nstar > (1 << 20)) return fail(MPSFR_E_INVALID, "%s: nstar=%d outside 1..2^20", who, nstar);
    if (flags & ~MPSFR_FIT_BACKGROUND)
        return fail(MPSFR_E_INVALID, "%s: unknown flag bits (only the background bit has a meaning here)", who);
    if (!psf_index && npsf != nstar) return fail(MPSFR_E_INVALID, "%s: without psf_index, npsf must equal nstar", who);
    if (!(radius >= 1.0 && radius <= MPSFR_FRAME_FIT_MAX_RADIUS))
        return fail(MPSFR_E_INVALID, "%s: radius must be finite, in 1..%g pixels", who, MPSFR_FRAME_FIT_MAX_RADIUS);
    if (!(tol > 0.0 && tol < 1.0)) return fail(MPSFR_E_INVALID, "%s: tol must lie in (0, 1)", who);
    if (max_iter < 1 || max_iter > MPSFR_FRAME_FIT_MAX_ITER)
        return fail(MPSFR_E_INVALID, "%s: max_iter=%d outside 1..%d", who, max_iter, MPSFR_FRAME_FIT_MAX_ITER);
    return MPSFR_OK;
}

int mpsfr_fit_frame_psf(mpsfr_ctx* c, int ny, int nx, const double* image, const double* var, int nstar, int npsf,
                        const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                        const double* scale0, double radius, int flags, int max_iter, double tol, double* star_out,
                        double* head_out, double* resid_out, int on_device) {
    if (!c || !image || !psf || !origin || !star_out || !head_out || npsf < 1)
        return fail(MPSFR_E_INVALID, "fit_frame_psf: bad argument (image, psf, origin, star_out and head_out are required)");
    int rc;
    if ((rc = frame_fit_ranges("fit_frame_psf", ny, nx, nstar, npsf, psf_index, radius, flags, max_iter, tol))) return rc;
    if (!on_device) {
        if ((rc = check_model_list("fit_frame_psf", "shift", nstar, npsf, psf_index, shift, (size_t)2 * nstar))) return rc;
        if ((rc = check_frame_stars("fit_frame_psf", nstar, origin, scale0, "scale0"))) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->framefit, frame_fit_workspace_bytes(ny, nx, nstar)))) return rc;
    const size_t npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto im = st.in(image, npix), va = st.in(var, npix), ps = st.in(psf, npsf * kStampPix);
    auto sh = st.in(shift, (size_t)2 * nstar), s0 = st.in(scale0, (size_t)nstar);
    auto og = st.in(origin, (size_t)2 * nstar), pi = st.in(psf_index, (size_t)nstar);
    auto rows = st.out(star_out, (size_t)nstar * MPSFR_NFRAMEFIT), head = st.out(head_out, MPSFR_NFRAMEFIT);
    auto res = st.out(resid_out, npix);
    return st.run([&](hipStream_t s) {
        launch_fit_frame(s, ny, nx, im, va, StarList{nstar, npsf, ps, pi, og, sh}, s0, radius,
                         (flags & MPSFR_FIT_BACKGROUND) != 0, max_iter, tol, rows, head, res, c->framefit.p);
    });
}

static_assert(MPSFR_NFRAMEFREE == 16 && MPSFR_NFRAMEFREE_HEAD == 12 && MPSFR_FRAME_FREE_HELD == 1 &&
                  MPSFR_FRAME_FREE_BOUND == 2 && MPSFR_FRAME_FREE_CLIPPED == 4,
              "k_fr_step<FR_FINAL> row layout and flags");

// what mpsfr_fit_frame_psf_free and mpsfr_fit_cube_psf_free refuse alike: the parameters of the outer loop
static int frame_free_ranges(const char* who, int max_outer, double pos_tol, double max_step, double max_move,
                             double min_snr) {
    if (max_outer < 0 || max_outer > MPSFR_FRAME_FREE_MAX_OUTER)
        return fail(MPSFR_E_INVALID, "%s: max_outer=%d outside 0..%d", who, max_outer, MPSFR_FRAME_FREE_MAX_OUTER);
    if (!(pos_tol > 0.0 && std::isfinite(pos_tol))) return fail(MPSFR_E_INVALID, "%s: pos_tol must be finite and > 0", who);
    if (!(max_step > 0.0 && max_step <= MPSFR_FRAME_FREE_MAX_STEP))
        return fail(MPSFR_E_INVALID, "%s: max_step must lie in (0, %g] pixels", who, MPSFR_FRAME_FREE_MAX_STEP);
    if (!(max_move > 0.0 && max_move <= MPSFR_FRAME_FREE_MAX_MOVE))
        return fail(MPSFR_E_INVALID, "%s: max_move must lie in (0, %g] pixels", who, MPSFR_FRAME_FREE_MAX_MOVE);
    if (!(min_snr >= 0.0 && std::isfinite(min_snr))) return fail(MPSFR_E_INVALID, "%s: min_snr must be finite and >= 0", who);
    return MPSFR_OK;
}

int mpsfr_fit_frame_psf_free(mpsfr_ctx* c, int ny, int nx, const double* image, const double* var, int nstar, int npsf,
                             const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                             const double* scale0, double radius, int flags, int max_iter, double tol, int max_outer,
                             double pos_tol, double max_step, double max_move, double min_snr, double* star_out,
                             double* shift_out, double* head_out, double* resid_out, int on_device) {
    const char* who = "fit_frame_psf_free";
    if (!c || !image || !psf || !origin || !star_out || !shift_out || !head_out || npsf < 1)
        return fail(MPSFR_E_INVALID,
                    "%s: bad argument (image, psf, origin, star_out, shift_out and head_out are required)", who);
    int rc;
    if ((rc = frame_fit_ranges(who, ny, nx, nstar, npsf, psf_index, radius, flags, max_iter, tol))) return rc;
    if ((rc = frame_free_ranges(who, max_outer, pos_tol, max_step, max_move, min_snr))) return rc;
    if (!on_device) {
        if ((rc = check_model_list(who, "shift", nstar, npsf, psf_index, shift, (size_t)2 * nstar))) return rc;
        if ((rc = check_frame_stars(who, nstar, origin, scale0, "scale0"))) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->framefit, frame_free_workspace_bytes(ny, nx, nstar)))) return rc;
    const size_t npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto im = st.in(image, npix), va = st.in(var, npix), ps = st.in(psf, npsf * kStampPix);
    auto sh = st.in(shift, (size_t)2 * nstar), s0 = st.in(scale0, (size_t)nstar);
    auto og = st.in(origin, (size_t)2 * nstar), pi = st.in(psf_index, (size_t)nstar);
    auto rows = st.out(star_out, (size_t)nstar * MPSFR_NFRAMEFREE), so = st.out(shift_out, (size_t)2 * nstar);
    auto head = st.out(head_out, MPSFR_NFRAMEFREE_HEAD), res = st.out(resid_out, npix);
    return st.run([&](hipStream_t s) {
        launch_fit_frame_free(s, ny, nx, im, va, StarList{nstar, npsf, ps, pi, og, sh}, s0, radius,
                              (flags & MPSFR_FIT_BACKGROUND) != 0, max_iter, tol, max_outer, pos_tol, max_step, max_move,
                              min_snr, rows, so, head, res, c->framefit.p);
    });
}

// what mpsfr_fit_cube_psf and mpsfr_fit_cube_psf_free refuse alike on host pointers: the model list, the stars, scale0,
// layer_shift and the summed shifts
static int cube_fit_host_arguments(const char* who, int nl, int nstar, int npsf, const int32_t* psf_index,
                                   const int32_t* origin, const double* shift, const double* layer_shift,
                                   const double* scale0) {
    int rc;
    if ((rc = check_model_list(who, "shift", nstar, npsf, psf_index, shift, (size_t)2 * nstar))) return rc;
    if ((rc = check_frame_stars(who, nstar, origin, nullptr, "scale0"))) return rc;
    if (scale0)
        for (size_t k = 0; k < (size_t)nl * nstar; ++k)
            if (!std::isfinite(scale0[k])) return fail(MPSFR_E_INVALID, "%s: a scale0 that is not finite", who);
    if (layer_shift) {
        // (rounding is monotone: the sums of a layer stay in range when those of the extreme shifts do)
        double lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
        for (int k = 0; shift && k < 2 * nstar; ++k) {
            lo[k & 1] = k < 2 ? shift[k] : std::min(lo[k & 1], shift[k]);
            hi[k & 1] = k < 2 ? shift[k] : std::max(hi[k & 1], shift[k]);
        }
        for (int k = 0; k < 2 * nl; ++k) {
            const double t = layer_shift[k];
            if (!std::isfinite(t)) return fail(MPSFR_E_INVALID, "%s: a layer_shift that is not finite", who);
            if (!(std::fabs(lo[k & 1] + t) <= MPSFR_FIT_PSF_MAX_SHIFT && std::fabs(hi[k & 1] + t) <= MPSFR_FIT_PSF_MAX_SHIFT))
                return fail(MPSFR_E_INVALID, "%s: shift + layer_shift beyond 8 pixels", who);
        }
    }
    return MPSFR_OK;
}

int mpsfr_fit_cube_psf(mpsfr_ctx* c, int nl, int ny, int nx, const double* cube, const double* var, int nstar, int npsf,
                       const double* psf, const int32_t* psf_index, const int32_t* origin, const double* shift,
                       const double* layer_shift, const double* scale0, double radius, int flags, int max_iter,
                       double tol, int layer_batch, double* star_out, double* head_out, double* resid_out,
                       int on_device) {
    const char* who = "fit_cube_psf";
    if (!c || !cube || !psf || !origin || !star_out || !head_out || npsf < 1)
        return fail(MPSFR_E_INVALID, "%s: bad argument (cube, psf, origin, star_out and head_out are required)", who);
    int rc;
    if ((rc = frame_fit_ranges(who, ny, nx, nstar, npsf, psf_index, radius, flags, max_iter, tol))) return rc;
    if (nl < 1 || nl > MPSFR_CUBE_FIT_MAX_LAYERS)
        return fail(MPSFR_E_INVALID, "%s: nl=%d outside 1..%d", who, nl, MPSFR_CUBE_FIT_MAX_LAYERS);
    if (layer_batch < 0) return fail(MPSFR_E_INVALID, "%s: layer_batch=%d is negative", who, layer_batch);
    if (!on_device && (rc = cube_fit_host_arguments(who, nl, nstar, npsf, psf_index, origin, shift, layer_shift, scale0)))
        return rc;
    HIPCHK(hipSetDevice(c->device));
    // the layers of a batch: asked for, or what the budget of work memory holds
    const size_t fixed = cube_fit_workspace_bytes(ny, nx, nstar, 0), per = cube_fit_workspace_bytes(ny, nx, nstar, 1) - fixed;
    int nb = layer_batch > 0 ? layer_batch : (int)std::min<size_t>((size_t)nl, MPSFR_CUBE_FIT_WORK_BYTES / per);
    nb = std::max(1, std::min(nb, nl));
    if ((rc = ensure(c, c->cubefit, cube_fit_workspace_bytes(ny, nx, nstar, nb)))) return rc;
    hipStream_t s = c->stream;
    if ((rc = wait_for_lanes(c, s))) return rc;
    const bool back = (flags & MPSFR_FIT_BACKGROUND) != 0;
    const size_t npix = (size_t)ny * nx, nrow = (size_t)nstar * MPSFR_NFRAMEFIT;
    if (on_device) {
        ProfScope ps(c, K_FIT);
        for (int l0 = 0; l0 < nl; l0 += nb) {
            const size_t o = (size_t)l0;
            StarList stars{nstar, npsf, psf + o * kStampPix, psf_index, origin, shift};
            stars.lshift = layer_shift ? layer_shift + 2 * o : nullptr;
            stars.nl = nl;
            launch_fit_cube(s, ny, nx, std::min(nb, nl - l0), cube + o * npix, var ? var + o * npix : nullptr, stars,
                            scale0 ? scale0 + o * nstar : nullptr, radius, back, max_iter, tol, star_out + o * nrow,
                            head_out + o * MPSFR_NFRAMEFIT, resid_out ? resid_out + o * npix : nullptr, c->cubefit.p);
        }
        HIPCHK(hipGetLastError());
        return MPSFR_OK;
    }
    // Host pointers: what all layers share is staged once, the layers batch by batch -- cube, var, the models of the
    // batch as [npsf][layers][40][40], scale0, and the three outputs, each declared at the capacity of a batch
    const size_t B = (size_t)nb;
    Staged st(c, 0);
    auto sh = st.in(shift, (size_t)2 * nstar), ls = st.in(layer_shift, (size_t)2 * nl);
    auto og = st.in(origin, (size_t)2 * nstar), pi = st.in(psf_index, (size_t)nstar);
    auto cu = st.in(cube, B * npix), va = st.in(var, B * npix), ps = st.in(psf, npsf * B * kStampPix);
    auto s0 = st.in(scale0, B * nstar);
    auto rows = st.out(star_out, B * nrow), head = st.out(head_out, B * MPSFR_NFRAMEFIT), res = st.out(resid_out, B * npix);
    if ((rc = st.place(sizeof(double)))) return rc;
    if (shift) HIPCHK(st.put(sh, shift, (size_t)2 * nstar));
    if (layer_shift) HIPCHK(st.put(ls, layer_shift, (size_t)2 * nl));
    HIPCHK(st.put(og, origin, (size_t)2 * nstar));
    if (psf_index) HIPCHK(st.put(pi, psf_index, (size_t)nstar));
    {
        ProfScope prof(c, K_FIT);
        for (int l0 = 0; l0 < nl; l0 += nb) {
            const size_t o = (size_t)l0, n = (size_t)std::min(nb, nl - l0);
            HIPCHK(st.put(cu, cube + o * npix, n * npix));
            if (var) HIPCHK(st.put(va, var + o * npix, n * npix));
            if (scale0) HIPCHK(st.put(s0, scale0 + o * nstar, n * nstar));
            const size_t width = n * kStampPix * sizeof(double);
            HIPCHK(hipMemcpy2DAsync(st.address(ps), width, psf + o * kStampPix, (size_t)nl * kStampPix * sizeof(double),
                                    width, (size_t)npsf, hipMemcpyHostToDevice, s));
            StarList stars{nstar, npsf, ps, pi, og, sh};
            stars.lshift = layer_shift ? ls + 2 * o : nullptr;
            stars.nl = (int)n;
            launch_fit_cube(s, ny, nx, (int)n, cu, va, stars, s0, radius, back, max_iter, tol, rows, head, res,
                            c->cubefit.p);
            HIPCHK(hipGetLastError());
            HIPCHK(st.get(star_out + o * nrow, rows, n * nrow));
            HIPCHK(st.get(head_out + o * MPSFR_NFRAMEFIT, head, n * MPSFR_NFRAMEFIT));
            if (resid_out) HIPCHK(st.get(resid_out + o * npix, res, n * npix));
            HIPCHK(hipStreamSynchronize(s));      // (the staged batch is refilled by the next one)
        }
    }
    return MPSFR_OK;
}

static_assert(MPSFR_NCUBEFREE_POS == 8 && MPSFR_NCUBEFREE_CALL == 8, "k_cf_step<CF_FINAL> row layout");

int mpsfr_fit_cube_psf_free(mpsfr_ctx* c, int nl, int ny, int nx, const double* cube, const double* var, int nstar,
                            int npsf, const double* psf, const int32_t* psf_index, const int32_t* origin,
                            const double* shift, const double* layer_shift, const double* scale0, double radius,
                            int flags, int max_iter, double tol, int max_outer, double pos_tol, double max_step,
                            double max_move, double min_snr, double* star_out, double* head_out, double* pos_out,
                            double* shift_out, double* call_out, double* resid_out, int on_device) {
    const char* who = "fit_cube_psf_free";
    if (!c || !cube || !psf || !origin || !star_out || !head_out || !pos_out || !shift_out || !call_out || npsf < 1)
        return fail(MPSFR_E_INVALID,
                    "%s: bad argument (cube, psf, origin, star_out, head_out, pos_out, shift_out and call_out are required)",
                    who);
    int rc;
    if ((rc = frame_fit_ranges(who, ny, nx, nstar, npsf, psf_index, radius, flags, max_iter, tol))) return rc;
    if (nl < 1 || nl > MPSFR_CUBE_FIT_MAX_LAYERS)
        return fail(MPSFR_E_INVALID, "%s: nl=%d outside 1..%d", who, nl, MPSFR_CUBE_FIT_MAX_LAYERS);
    if ((rc = frame_free_ranges(who, max_outer, pos_tol, max_step, max_move, min_snr))) return rc;
    if (!on_device && (rc = cube_fit_host_arguments(who, nl, nstar, npsf, psf_index, origin, shift, layer_shift, scale0)))
        return rc;
    const size_t work = cube_free_workspace_bytes(ny, nx, nstar, nl);
    if (work > MPSFR_CUBE_FREE_WORK_BYTES)
        return fail(MPSFR_E_INVALID, "%s: %zu bytes of work memory for %d layers, above the budget of %zu: take the "
                                     "positions from fewer layers", who, work, nl, (size_t)MPSFR_CUBE_FREE_WORK_BYTES);
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ensure(c, c->cubefit, work))) return rc;
    const size_t L = (size_t)nl, npix = (size_t)ny * nx;
    Staged st(c, on_device);
    auto cu = st.in(cube, L * npix), va = st.in(var, L * npix), ps = st.in(psf, npsf * L * kStampPix);
    auto sh = st.in(shift, (size_t)2 * nstar), ls = st.in(layer_shift, 2 * L), s0 = st.in(scale0, L * nstar);
    auto og = st.in(origin, (size_t)2 * nstar), pi = st.in(psf_index, (size_t)nstar);
    auto rows = st.out(star_out, L * nstar * MPSFR_NFRAMEFIT), head = st.out(head_out, L * MPSFR_NFRAMEFIT);
    auto po = st.out(pos_out, (size_t)nstar * MPSFR_NCUBEFREE_POS), so = st.out(shift_out, (size_t)2 * nstar);
    auto call = st.out(call_out, MPSFR_NCUBEFREE_CALL), res = st.out(resid_out, L * npix);
    return st.run([&](hipStream_t s) {
        launch_fit_cube_free(s, ny, nx, nl, cu, va, StarList{nstar, npsf, ps, pi, og, sh, ls, nl}, s0, radius,
                             (flags & MPSFR_FIT_BACKGROUND) != 0, max_iter, tol, max_outer, pos_tol, max_step, max_move,
                             min_snr, rows, head, po, so, call, res, c->cubefit.p);
    });
}

}  // extern "C"
