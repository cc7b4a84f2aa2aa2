// What the host files of libmpsfr share: the context, its grow-only device buffers, the error string, the wait for the
// pipeline lanes and the profiling scope.  Private to csrc/: mpsfr_api.cpp (the pipeline) and stamp_calls.cpp.
#pragma once

#include "../../include/mpsfr.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "kernels.h"

// mpsfr::host is internal to libmpsfr.so (hidden): nothing in it is exported, and calls between the host files are direct
namespace mpsfr {
namespace host __attribute__((visibility("hidden"))) {

// the text behind mpsfr_last_error
inline thread_local std::string g_err;

// log2 of the smallest OTF element (relative to OTF[0][0] = 1) that still has a normal fp16 high half
// (mf_common.h: kShift = 15), with a margin for the fp32 rounding of the bound
constexpr float kMfFloorLog2 = -29.01f;

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(MPSFR_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

constexpr size_t kStampPix = (size_t)NS * NS;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct Pending {
    int id;
    hipEvent_t a, b;
};

}  // namespace host
}  // namespace mpsfr

struct mpsfr_ctx {
    using DevBuf = mpsfr::host::DevBuf;
    int device = 0, N = 0, dimpsf = 0, prec = 0, ncu = 256;
    // CUs the two persistent grids leave free (K_OTF_MFMA2 / K_DPHI_SERIES launch ncu - R workgroups, no CU
    // masks): the other lane's latency-bound kernels find room beside them (VERDICT r5 #1a)
    // -1 (default): ncu / 8 while the context's other lane has work in flight, 0 for a call that runs alone
    int reserve_mf = -1, reserve_a = -1;
    // the tip-tilt kernel spectra ride in the second launch of the patch (series form of stage A)
    bool head_fusion = true;
    // stage A (series form) skips what lies outside the support of the telescope OTF
    bool support_skip = true;
    double pixscale = 0.2;
    bool f64 = false;
    hipStream_t stream = nullptr;
    // options
    int chunk_tasks = 0;   // 0 = automatic
    bool fast_exp = true;    // mixed mode: exp(x) = v_exp_f32(x log2 e)
    bool profile = false;
    int prof_only = -1;          // >= 0: time only this kernel id
    int prof_every = 1;          // time every n-th launch of a slot (a timed launch stops its queue twice)
    unsigned prof_count[64] = {};
    bool fft_conv = true;   // mixed mode: convolutions through 64-point FFTs
    int prune_fixed = 0;         // experiments: transform exactly this many lines (wrong results)
    double prune_eps = 1.0e-9;   // mixed mode: line pruning of the per-wavelength stage (0 = off)
    double prune_eps_f64 = 1.0e-13;  // f64 mode: the same, far below what its 1e-11 stamps resolve
    bool otf_mfma = true;        // mixed mode: per-wavelength stage on the matrix cores (otf_mfma.hip)
    bool mf_floor = true;        // matrix-core stage: skip blocks below the fp16 representation floor
    int mf_kernel = 2;           // 2: thin-wave kernel with precision tiers (otf_mfma2.hip, one direction); 1: otf_mfma.hip
    int mf_permax = 6;           // wavelengths per workgroup of the thin-wave kernel (6: 12 waves, 7: 14 waves)
    double mf_mid_log2 = -18.01; // blocks below 2^this need no low half of the OTF (see otf_mfma2.hip)
    double mf_floor_log2 = mpsfr::host::kMfFloorLog2;   // blocks below 2^this are dropped
    double tier_eps = 4.0e-6;    // budget of the two precision tiers, of the PSF peak (0: no tiers; inf: no budget)
    bool mf_clock = false;       // experiments: phase time stamps of the matrix-core kernel
    int stage_a = 1;             // stage A: 1 = automatic (the series + patch form of stage_a2.hip from 512^2 on, and at
                                 // 256^2 with several directions; the full-size transforms otherwise: one direction at
                                 // 256^2 19.2 against 18.3 M PSFs/s, nine directions 7.9 against 8.8), 0 = full-size
                                 // transforms, 2 = series + patch form on every grid
    DevBuf mfclk;
    // constant tables
    DevBuf tw64, tel, rows, tlmax, tl2, tlb, scoef, stwk, ssup;
    // per-call tables
    DevBuf aotab, samp_p, samp_a, G, kmuse, xtab, etab, gtab;
    // Pipeline lanes: each lane owns a HIP stream and a set of chunk workspaces.  Consecutive
    // chunks -- of one call or of consecutive asynchronous calls -- go to successive lanes, so one
    // chunk's low-occupancy tail (convolutions, fit) overlaps the next chunk's transforms.
    // `stream` is only the join stream: it waits for the lanes at the end of every call.
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;       // after the lane's last chunk of the most recent call (calls that join)
        hipEvent_t done_ev = nullptr;    // the event that marks the end of the lane's most recent call: `done`, or
                                         // the slot event of a call that queued a single marker (see "lean" below)
        bool busy = false;               // the lane has run a call
        bool marked = false;             // `done_ev` marks the end of the lane's most recent call (else: no marker was
                                         // queued for it -- lane_end() records one when somebody needs it)
        int ncu = 0;                     // CUs the lane's stream may use (0: all of them)
        DevBuf C, s00, D0t, Tq, pre, fin, dmin, dblk, vkeep, dminb, order, mown, muni, msched, mpart;
        DevBuf pP, pT, psp, dlin;        // series form of stage A: patch, its row transforms, its sum; line minima
        DevBuf thrf;                     // [tasks] floor of the kernel for several directions (K_PEAK_FLOOR)
        DevBuf band;                     // [tasks][nband][40][40] band stamps of a band call (K_BAND_REDUCE)
        // What D0t holds outside the part the series form of stage A writes (the pieces of a line outside the support
        // of the telescope OTF, the 16 padding lines, the lines of tasks beyond the chunk): 0 = zero or values the
        // series form left there itself; 1 = finite values of a call that wrote whole lines (the full-size form, the
        // series form with "support_skip" off); 2 = anything, non-finite included (a caller's PSD, mpsfr_psf_from_psd).
        // The next call that writes D0t clears the buffer first when it would otherwise read what is there: a series
        // call with the support skip at 1 or 2, every call at 2 ("Call-order independence").
        int d0t_stale = 0;
        // device outputs of its most recent calls: `done` is recorded behind every call of the lane,
        // so waiting for it covers all of them (a caller that rotates more buffer sets than lanes
        // must still get the calls that share a buffer in order)
        static constexpr int NHIST = 8;
        const void* outs[NHIST][3] = {};
        unsigned nouts = 0;
    };
    static constexpr int MAX_LANES = 4;
    Lane lane[MAX_LANES];
    int nlanes = 0;              // 0 = automatic (two lanes)
    int cu_partition = 0;        // 1: every lane's stream owns 1/lanes of the CUs (hipExtStreamCreateWithCUMask)
    bool param_copy_kernel = true;   // the parameter blob of a call is fetched by a kernel (else hipMemcpyAsync)
    bool stream_exported = false;    // mpsfr_stream() has been called: every call joins its lanes into `stream`
    hipEvent_t stream_tail = nullptr;    // created once a call has queued work on `stream` (mpsfr_stream_wait)
    bool pipeline_calls = true;  // successive asynchronous calls rotate over the lanes
    unsigned lane_rr = 0;        // lane of the next chunk
    hipEvent_t tables_ready = nullptr;
    hipEvent_t cache_ready = nullptr;    // cached per-wavelength / geometry tables are complete
    bool cache_ready_valid = false;
    hipEvent_t lsum_done = nullptr;      // the per-lane partial stamp sums have been consumed
    bool lsum_busy = false;
    hipEvent_t wait_next = nullptr;      // caller's event the next call must wait for
    // Stagger of the lanes at a cold start (see mpsfr_reconstruct)
    int cold_stagger = 0;                // 0: off; 1: behind the column transforms; 2: behind the preparation of the
                                         // per-wavelength stage
    hipEvent_t stagger_ev = nullptr;     // behind the column transforms of the first chunk after a cold start
    bool stagger_armed = false;
    int stagger_lane = -1;
    DevBuf specx;                      // [nl] the abscissa of mpsfr_fit_spectra_psf's drift
    DevBuf render;                     // work lists of mpsfr_render_stars (render_workspace_bytes)
    DevBuf find;                       // core, map, masks and counts of mpsfr_find_stars (find_workspace_bytes)
    DevBuf group;                      // cells, union-find and row lists of mpsfr_group_stars (group_workspace_bytes)
    DevBuf framefit;                   // lists, frames, vectors and scalars of mpsfr_fit_frame_psf (frame_fit_workspace_bytes)
    DevBuf cubefit;                    // the same for a batch of layers of mpsfr_fit_cube_psf (cube_fit_workspace_bytes)
    DevBuf fit, sum, stage, lsum;      // lsum: [lanes][nl][40][40] per-lane partial stamp sums
    // mpsfr_psd_to_psf: a stream and workspaces of its own, so that it never waits for nor touches the lanes
    struct P2P {
        hipStream_t stream = nullptr;
        int twm_len = 0;                 // length of the twiddle table in `twm`
        DevBuf twm, psd, cm, d0t, pup, phase, lbda, cl, t1, q, otf, g, out;
    } p2p;
    // Small per-call parameters: one pinned host blob -> one device blob, no stream sync.  A ring
    // of NSTAGE slots (pinned blob, device blob, tip-tilt kernel spectra): the host may queue
    // NSTAGE calls ahead of the GPU, and calls in flight on different lanes never share a slot.
    static constexpr int NSTAGE = 4;
    struct Slot {
        void* host = nullptr;
        size_t host_cap = 0;
        hipEvent_t staged = nullptr;     // after the H2D copy (the pinned blob may be refilled)
        hipEvent_t staged_ev = nullptr;  // what the host waits for before it refills the blob: `staged` or `call_done`
        bool staged_pending = false;
        hipEvent_t call_done = nullptr;  // after the call that used the slot (join stream, or the call's lane)
        bool call_pending = false;
        int last_lane = -1;              // lane of a lean call (stream order covers the slot's reuse there)
        bool has_event = true;           // `call_done` was recorded for the slot's last call
        unsigned long long seq = 0;      // staged_mode 2: the value the parameter-copy kernel writes into seq_host[slot]
        int staged_mode = 0;             // what frees the pinned blob: 0 `staged`, 1 `call_done`, 2 the kernel's flag
        DevBuf params, ktt;
    };
    Slot slot[NSTAGE];
    unsigned stage_next = 0;
    // Pinned host words the parameter-copy kernels write when they have read their blob (one per slot): the host
    // polls them instead of waiting for an event, so that a lean call queues no marker packet at all.
    unsigned long long* seq_host = nullptr;
    unsigned long long seq_next = 0;
    // Asynchronous host outputs (on_device = 2): a ring of result sets -- device buffers the call
    // writes, a pinned host mirror the join stream copies them to -- and the caller's arrays, filled
    // when the ticket is waited for.  The host queues up to NTICKET such calls ahead of the GPU and the
    // calls rotate over the lanes like device-output calls do.
    struct Ticket {
        long id = -1;
        bool pending = false;
        hipEvent_t done = nullptr;
        DevBuf dpsf, dsum, dfit;
        void* host = nullptr;
        size_t host_cap = 0;
        double *u_psf = nullptr, *u_sum = nullptr, *u_fit = nullptr;
        size_t n_psf = 0, n_sum = 0, n_fit = 0;
    };
    static constexpr int NTICKET = 4;
    Ticket ticket[NTICKET];
    // mpsfr_reconstruct_multi_async (held by ctxs[0]): the shards' stamp sums until mpsfr_wait_multi adds them
    struct Multi {
        bool pending = false;
        int nctx = 0;
        size_t n = 0;                    // nl * 1600
        std::vector<double> sums;        // [nctx][n]
        std::vector<long> tickets;       // per context (-1: no shard)
        double* user_sum = nullptr;
    } multi;
    long ticket_next = 0;                // id of the next asynchronous host-output call
    long d0t_clears = 0;                 // lane D0t buffers cleared because of what an earlier call left (d0t_stale)
    double host_seconds = 0.0;           // wall time spent inside mpsfr_reconstruct
    long host_calls = 0;
    // caches of the per-call tables that only depend on (lbda) / (geometry, masks)
    std::vector<double> cache_lbda;
    int cache_lbda_mode = -1;
    const void* cache_G_ptr = nullptr;
    const void* cache_kmuse_ptr = nullptr;
    const void* cache_xtab_ptr = nullptr;
    bool cache_xtab_valid = false;
    const void* cache_etab_ptr = nullptr;
    const void* cache_gtab_ptr = nullptr;
    bool cache_mf_valid = false;
    std::vector<unsigned char> cache_geom;
    const void* cache_ao_ptr = nullptr;
    // bookkeeping for debug_fetch
    int last_ndir = 0, last_nl = 0, last_chunk_tasks = 0, last_lane = 0;
    int last_ntab = 2;                   // layer tables per direction of the current AO tables (2: a legacy call)
    int last_gpp = 1;                    // stamp groups per task of the last call: npos of a field call, else 1
    bool last_mf = false, last_pruned = false, last_mf2 = false, last_dlin = false;
    float last_thr_blk = 0.f;
    bool last_floor_per_task = false;
    std::vector<double> last_lpc;        // c of every wavelength of the last call
    // thr_eps, thr_floor, thr_mid, tier_half, thr_blk, thr_sum, c2min of the last call ("mf_par")
    float last_thr[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // profiling
    double prof_ms[mpsfr::K_COUNT] = {0};
    long prof_n[mpsfr::K_COUNT] = {0};
    std::vector<mpsfr::host::Pending> pending;
    std::vector<hipEvent_t> pool;
};

namespace mpsfr {
namespace host __attribute__((visibility("hidden"))) {

inline size_t rsize(const mpsfr_ctx* c) { return c->f64 ? sizeof(double) : sizeof(float); }

inline int ensure(mpsfr_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return MPSFR_OK;
    if (b.p) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = bytes + bytes / 8;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        b.p = nullptr;
        return fail(MPSFR_E_NOMEM, "hipMalloc of %zu bytes failed", want);
    }
    b.cap = want;
    return MPSFR_OK;
}

inline void release(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// The event behind the lane's most recent call; a lean call queued none, so it is recorded here, at the lane's
// present tail (at or behind the end of that call: conservative), when somebody needs to wait for the lane.
inline hipEvent_t lane_end(mpsfr_ctx* c, mpsfr_ctx::Lane& ln) {
    // (a lane whose stream has been dropped -- "streams" / "cu_partition" reset -- has drained: nothing to record,
    // and recording on the NULL stream would synchronise with every blocking stream)
    if (!ln.marked && ln.stream != nullptr) {
        if (!ln.done) (void)hipEventCreateWithFlags(&ln.done, hipEventDisableTiming);
        (void)hipEventRecord(ln.done, ln.stream);
        ln.done_ev = ln.done;
        ln.marked = true;
    }
    return ln.done_ev;
}

inline hipEvent_t get_event(mpsfr_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int resolve_profile(mpsfr_ctx* c);      // (mpsfr_api.cpp)

struct ProfScope {
    mpsfr_ctx* c;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    bool on = false;
    bool markers;              // false: the launch itself carries the events (hipExtLaunchKernelGGL)
    ProfScope(mpsfr_ctx* ctx, int kid, hipStream_t stream = nullptr, bool use_markers = true)
        : c(ctx), id(kid), st(stream ? stream : ctx->stream), markers(use_markers) {
        on = c->profile && (c->prof_only < 0 || c->prof_only == kid);
        if (on && c->prof_every > 1 && kid >= 0 && kid < 64) on = (c->prof_count[kid]++ % (unsigned)c->prof_every) == 0;
        if (on) {
            a = get_event(c);
            b = get_event(c);
            if (!a || !b) {          // out of events: this launch goes untimed
                if (a) c->pool.push_back(a);
                if (b) c->pool.push_back(b);
                a = b = nullptr;
                on = false;
            } else if (markers) {
                (void)hipEventRecord(a, st);
            }
        }
    }
    ~ProfScope() {
        if (on) {
            if (markers) (void)hipEventRecord(b, st);
            c->pending.push_back({id, a, b});
            // a caller that never reads the profile must not grow the event list without bound
            if (c->pending.size() >= 8192) (void)resolve_profile(c);
        }
    }
};

// The calls queued so far run on the pipeline lanes: stream s waits for them on the GPU, so that device stamps written
// by a device-output reconstruct of this context are complete when a kernel on s reads them.
inline int wait_for_lanes(mpsfr_ctx* c, hipStream_t s) {
    for (int k = 0; k < mpsfr_ctx::MAX_LANES; ++k)
        if (c->lane[k].busy && c->lane[k].stream != s) HIPCHK(hipStreamWaitEvent(s, lane_end(c, c->lane[k]), 0));
    return MPSFR_OK;
}

}  // namespace host
}  // namespace mpsfr
