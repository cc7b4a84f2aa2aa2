// Stand-alone check of muse_psfr_amd/csrc/stage_layout.h (tests/test_stage_layout_host.py compiles and runs it with the
// address and undefined-behaviour sanitizers).  It declares the arrays of every call of stamp_calls.cpp in the order the
// entry point declares them, at small counts, with every subset of the optional arrays absent, and compares the offsets
// and the total of StageLayout with the rule of DESIGN.md ("The entry layer") restated here without a loop over passes:
// an array lies behind everything of an earlier class -- inputs of 8-byte elements, then outputs, then narrower inputs --
// and behind what was declared before it in its own class; an output takes its bytes rounded up to 8, an absent array
// takes nothing.  mpsfr_fit_rows, the seventeenth function of that file, stages nothing.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stage_layout.h"

using mpsfr::host::StageLayout;

namespace {

struct Spec {
    const char* name;
    bool output;
    size_t elem, count;
    bool optional;
};
struct Call {
    const char* name;
    std::vector<Spec> arrays;
};
struct Sizes {
    size_t nstar, npsf, nl, ny, nx, nsrc, max_stars, max_groups, stride, nmet, box, nb;
};

Spec D(const char* n, size_t count, bool opt = false) { return {n, false, sizeof(double), count, opt}; }
Spec I(const char* n, size_t count, bool opt = false) { return {n, false, sizeof(int32_t), count, opt}; }
Spec OD(const char* n, size_t count, bool opt = false) { return {n, true, sizeof(double), count, opt}; }
Spec OI(const char* n, size_t count, bool opt = false) { return {n, true, sizeof(int32_t), count, opt}; }

std::vector<Call> calls(const Sizes& z) {
    const size_t S = 1600, n = z.nstar, P = z.npsf, L = z.nl, npix = z.ny * z.nx, B = z.nb;
    const size_t ncell = L * ((z.ny + z.box - 1) / z.box) * ((z.nx + z.box - 1) / z.box);
    const bool opt = true;
    return {
        {"fit_stamps", {D("stamps", n * S), OD("fit", n * 16)}},
        {"fit_stamps_elliptical", {D("stamps", n * S), OD("fit", n * 24)}},
        {"fit_stamps_observed", {D("stamps", n * S), D("var", n * S, opt), OD("fit", n * 24)}},
        {"fit_stamps_psf",
         {D("stamps", n * S), D("var", n * S, opt), D("psf", P * S), D("shift", 2 * n, opt), I("psf_index", n, opt),
          OD("fit", n * 16)}},
        {"fit_groups_psf",
         {D("stamps", n * S), D("var", n * S, opt), D("psf", P * S), D("shift", 2 * z.nsrc * n), I("psf_index", n, opt),
          OD("fit", n * 48)}},
        {"fit_spectra_psf",
         {D("cubes", n * L * S), D("var", n * L * S, opt), D("psf", P * L * S), D("shift", 2 * n, opt),
          I("psf_index", n, opt), OD("fit", n * (16 + 10 * L))}},
        {"stamp_metrics", {D("stamps", n * S), D("centers", 2 * n, opt), OD("out", n * (8 + z.nmet))}},
        {"cut_stamps",
         {D("image", npix), D("var", npix, opt), I("origin", 2 * n), OD("stamps_out", n * S), OD("var_out", n * S, opt)}},
        {"render_stars",
         {D("image_in", npix, opt), D("psf", P * S), D("shift", 2 * n, opt), D("scale", n), I("origin", 2 * n),
          I("psf_index", n, opt), OD("image_out", npix), OD("star_out", n * 4, opt)}},
        {"find_stars",
         {D("image", npix), D("var", npix, opt), D("psf", S), OD("star_out", z.max_stars * 8), OD("map_out", npix, opt),
          OI("origin_out", 2 * z.max_stars, opt), OI("count_out", 1)}},
        {"frame_background",
         {D("image", L * npix), D("var", L * npix, opt), D("apply_to", L * npix, opt), OD("mesh_out", ncell * 8),
          OD("head_out", L * 4), OD("map_out", L * npix, opt), OD("rms_out", L * npix, opt),
          OD("applied_out", L * npix, opt)}},
        {"group_stars",
         {D("pos", n * z.stride), OD("shift_out", z.max_groups * 8, opt), OI("label_out", n),
          OI("group_out", z.max_groups * 8), OI("origin_out", 2 * z.max_groups, opt), OI("count_out", 6)}},
        {"fit_frame_psf",
         {D("image", npix), D("var", npix, opt), D("psf", P * S), D("shift", 2 * n, opt), D("scale0", n, opt),
          I("origin", 2 * n), I("psf_index", n, opt), OD("star_out", n * 8), OD("head_out", 8), OD("resid_out", npix, opt)}},
        {"fit_frame_psf_free",
         {D("image", npix), D("var", npix, opt), D("psf", P * S), D("shift", 2 * n, opt), D("scale0", n, opt),
          I("origin", 2 * n), I("psf_index", n, opt), OD("star_out", n * 16), OD("shift_out", 2 * n), OD("head_out", 12),
          OD("resid_out", npix, opt)}},
        // the host form: what the call stages once, then a batch of nb layers
        {"fit_cube_psf",
         {D("shift", 2 * n, opt), D("layer_shift", 2 * L, opt), I("origin", 2 * n), I("psf_index", n, opt),
          D("cube", B * npix), D("var", B * npix, opt), D("psf", P * B * S), D("scale0", B * n, opt),
          OD("star_out", B * n * 8), OD("head_out", B * 8), OD("resid_out", B * npix, opt)}},
        {"fit_cube_psf_free",
         {D("cube", L * npix), D("var", L * npix, opt), D("psf", P * L * S), D("shift", 2 * n, opt),
          D("layer_shift", 2 * L, opt), D("scale0", L * n, opt), I("origin", 2 * n), I("psf_index", n, opt),
          OD("star_out", L * n * 8), OD("head_out", L * 8), OD("pos_out", n * 8), OD("shift_out", 2 * n),
          OD("call_out", 8), OD("resid_out", L * npix, opt)}},
    };
}

int failures = 0;

#define CHECK(cond, ...)                \
    do {                                \
        if (!(cond)) {                  \
            std::printf("FAIL: ");      \
            std::printf(__VA_ARGS__);   \
            std::printf("\n");          \
            ++failures;                 \
        }                               \
    } while (0)

int klass(const Spec& s) { return s.output ? 1 : s.elem < 8 ? 2 : 0; }
size_t taken(const Spec& s) { return s.output ? (s.elem * s.count + 7) / 8 * 8 : s.elem * s.count; }

// one case: the optional arrays whose bit in `absent` is set (in the order of the optionals) are NULL
void walk(const Call& call, unsigned absent) {
    const size_t na = call.arrays.size();
    std::vector<bool> present(na, true);
    unsigned bit = 0;
    for (size_t i = 0; i < na; ++i)
        if (call.arrays[i].optional) present[i] = !((absent >> bit++) & 1u);
    StageLayout lay;
    std::vector<int> idx(na);
    for (size_t i = 0; i < na; ++i) {
        const Spec& s = call.arrays[i];
        idx[i] = lay.add(present[i], s.count, s.elem, s.output);
        CHECK(idx[i] == (int)i, "%s: %s got the index %d, not %zu", call.name, s.name, idx[i], i);
    }
    const size_t total = lay.place();
    size_t want_total = 0;
    for (size_t i = 0; i < na; ++i) {
        if (!present[i]) continue;
        const Spec& s = call.arrays[i];
        want_total += taken(s);
        size_t want = 0;
        for (size_t j = 0; j < na; ++j)
            if (present[j] && (klass(call.arrays[j]) < klass(s) || (klass(call.arrays[j]) == klass(s) && j < i)))
                want += taken(call.arrays[j]);
        const size_t off = lay.a[i].offset, bytes = s.elem * s.count;
        CHECK(off == want, "%s (absent %#x): %s at %zu, the rule says %zu", call.name, absent, s.name, off, want);
        CHECK(lay.a[i].bytes == bytes, "%s: %s has %zu bytes, not %zu", call.name, s.name, lay.a[i].bytes, bytes);
        CHECK(off % s.elem == 0, "%s (absent %#x): %s at %zu is not aligned to %zu", call.name, absent, s.name, off, s.elem);
        CHECK(off + bytes <= total, "%s (absent %#x): %s ends beyond the total %zu", call.name, absent, s.name, total);
        for (size_t j = 0; j < i; ++j)
            if (present[j]) {
                const size_t o2 = lay.a[j].offset, b2 = call.arrays[j].elem * call.arrays[j].count;
                CHECK(off + bytes <= o2 || o2 + b2 <= off, "%s (absent %#x): %s and %s overlap", call.name, absent, s.name,
                      call.arrays[j].name);
            }
    }
    CHECK(total == want_total, "%s (absent %#x): total %zu, the rule says %zu", call.name, absent, total, want_total);
}

}  // namespace

int main() {
    // odd counts of int32 (nstar = 1 and 3, one count word), a 5 x 7 frame, one and three layers, batches of 1 and 2
    const Sizes sizes[] = {{1, 1, 1, 5, 7, 2, 1, 1, 2, 1, 4, 1}, {3, 2, 3, 5, 7, 3, 3, 3, 5, 5, 4, 2}};
    long cases = 0, with_absent = 0;
    const size_t ncall = calls(sizes[0]).size();
    for (size_t k = 0; k < ncall; ++k) {
        long call_cases = 0, call_absent = 0;
        for (const Sizes& z : sizes) {
            const Call call = calls(z)[k];
            unsigned nopt = 0;
            for (const Spec& s : call.arrays) nopt += s.optional;
            for (unsigned absent = 0; absent < (1u << nopt); ++absent) {
                walk(call, absent);
                ++call_cases;
                call_absent += absent != 0;
            }
        }
        std::printf("call %s %ld %ld\n", calls(sizes[0])[k].name, call_cases, call_absent);
        cases += call_cases;
        with_absent += call_absent;
    }
    std::printf("cases %ld absent %ld failures %d\n", cases, with_absent, failures);
    return failures ? 1 : 0;
}
