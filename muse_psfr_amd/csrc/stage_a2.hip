// Stage A in its "series + patch" form (round 4): the structure function D_phi0 of a task without any
// full-size transform.  Reference: simul_psd_wfm (psfrec.py:36-151), psd_fit (:616-626) and the
// structure function of psd_to_psf (:717-722).
//
// The residual PSD of a task is  PSD = F + P  with
//   F = the fitting term  cfit r0^(-5/3) (f^2 + 1/L0^2)^(-11/6) [f >= fc]  on the whole half-pixel
//       grid (psfrec.py:616-626), and
//   P = max(F, AO) - F >= 0, which lives in the 80 x 80 corrected zone only (psfrec.py:148-149).
// The transform is linear, so  D = D_F + D_P.
//
//  * D_F.  With eps = 1/L0^2, eps0 = 1/128 and delta = eps - eps0 (|delta| <= 0.0126 for L0 >= 7 m,
//    against f^2 + eps0 >= 2.2578 on the support of F),
//        (f^2 + eps)^(-11/6) = sum_k binom(-11/6, k) delta^k (f^2 + eps0)^(-11/6 - k)
//    converges by a factor <= 0.0056 per term.  The structure functions Hd_k of the terms depend on the
//    grid alone: they are computed ONCE PER CONTEXT with the full-size fp64 transforms of stage_a.hip
//    ("basis" tasks), and a task's D_F = r0^(-5/3) sum_k delta^k Hd_k is a polynomial per pixel.  D_F is
//    1-2 % of D (the fitting error saturates at small separations), and every term is a structure
//    function of a non-negative PSD -- no cancellation is left at run time -- so the mixed mode
//    evaluates it in fp32 from fp32 tables (4 terms: truncation 4e-9 of D_F); the f64 mode keeps 8
//    fp64 terms (6e-18).
//  * D_P = 2 scale (sum P - Re FFT2(P)) in fp64, as a PRUNED transform: 80 x 80 inputs, (N/2+1) x N
//    outputs.  Row pass (K_PATCH_ROWS): T[su][y] = sum_sv P[su][sv] W^(sv y).  Column pass
//    (K_DPHI_SERIES): with x = 64 k1 + k2, Q = N / 64 and su = r + Q j,
//        X[64 k1 + k2] = sum_r W_Q^(r k1) S_r[k2],   S_r[k2] = W_N^(r k2) sum_j T[r + Q j] W_64^(j k2):
//    a lane (k2) folds the inputs of a line into sums per class r and runs a Q-point transform in its own
//    registers; its Q outputs are x = k2, 64 + k2, ...: for every k1 the 64 lanes store one 256-byte piece of
//    the line.  No LDS pass, no barrier, no workspace of N^2 size.
//    Only Re X is used, so only the Hermitian half of a line travels (hfold_valid below): the row pass
//    stores 41 values U[su] = T[su] + conj(T[-su]) per line instead of 80, the column pass forms the classes
//    r = 0 .. Q/2 from 41 complex multiply-adds (S_(Q-r) = conj(S_r)) and its transform is complex-to-real.
//    The 7 MB per task of row transforms (1280^2) become 0.4 MB, and the kernel is bound by its fp64
//    multiply-adds (~17 per pixel).
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "device_common.h"
#include "conv_frames.h"
#include "dpp_groups.h"
#include "psd_model.h"

namespace mpsfr {

namespace {

constexpr double kEps0 = 1.0 / 128.0;      // expansion point of 1/L0^2 (L0 = 11.3 m)

// W_Q^m = exp(-2 pi i m / Q), m < Q: the constant twiddles of the in-lane transforms
template <int Q> struct WQ;
template <> struct WQ<4> {
    static constexpr double c[4] = {1.0, 0.0, -1.0, 0.0};
    static constexpr double s[4] = {0.0, -1.0, 0.0, 1.0};
};
template <> struct WQ<8> {
    static constexpr double c[8] = {1.0, 0.70710678118654752440, 0.0, -0.70710678118654752440, -1.0,
                                    -0.70710678118654752440, 0.0, 0.70710678118654752440};
    static constexpr double s[8] = {0.0, -0.70710678118654752440, -1.0, -0.70710678118654752440, 0.0,
                                    0.70710678118654752440, 1.0, 0.70710678118654752440};
};
template <> struct WQ<16> {
    static constexpr double c[16] = {1.0, 0.92387953251128675613, 0.70710678118654752440, 0.38268343236508977173,
                                     0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613,
                                     -1.0, -0.92387953251128675613, -0.70710678118654752440,
                                     -0.38268343236508977173, 0.0, 0.38268343236508977173, 0.70710678118654752440,
                                     0.92387953251128675613};
    static constexpr double s[16] = {0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613,
                                     -1.0, -0.92387953251128675613, -0.70710678118654752440,
                                     -0.38268343236508977173, 0.0, 0.38268343236508977173, 0.70710678118654752440,
                                     0.92387953251128675613, 1.0, 0.92387953251128675613, 0.70710678118654752440,
                                     0.38268343236508977173};
};
template <> struct WQ<20> {
    static constexpr double c[20] = {1.0, 0.95105651629515357212, 0.80901699437494742410, 0.58778525229247312917,
                                     0.30901699437494742410, 0.0, -0.30901699437494742410, -0.58778525229247312917,
                                     -0.80901699437494742410, -0.95105651629515357212, -1.0,
                                     -0.95105651629515357212, -0.80901699437494742410, -0.58778525229247312917,
                                     -0.30901699437494742410, 0.0, 0.30901699437494742410, 0.58778525229247312917,
                                     0.80901699437494742410, 0.95105651629515357212};
    static constexpr double s[20] = {0.0, -0.30901699437494742410, -0.58778525229247312917, -0.80901699437494742410,
                                     -0.95105651629515357212, -1.0, -0.95105651629515357212,
                                     -0.80901699437494742410, -0.58778525229247312917, -0.30901699437494742410, 0.0,
                                     0.30901699437494742410, 0.58778525229247312917, 0.80901699437494742410,
                                     0.95105651629515357212, 1.0, 0.95105651629515357212, 0.80901699437494742410,
                                     0.58778525229247312917, 0.30901699437494742410};
};

template <int M>
__device__ __forceinline__ void dftm(cx<double>* v) {
    if constexpr (M == 2) dft2(v[0], v[1]);
    if constexpr (M == 4) dft4(v[0], v[1], v[2], v[3]);
    if constexpr (M == 5) dft5(v);
}

// terms of the fold: su = r + Q j in [-40, 40)
template <int Q> constexpr int fold_jmin() { return -((NAO / 2 + Q - 1) / Q); }
template <int Q> constexpr int fold_jmax() { return (NAO / 2 + Q - 1) / Q; }      // exclusive
template <int Q> constexpr int fold_nj() { return fold_jmax<Q>() - fold_jmin<Q>(); }
constexpr bool fold_valid(int Q, int r, int j) { return r + Q * j >= -NAO / 2 && r + Q * j < NAO / 2; }

// The Hermitian half of a line (K_PATCH_ROWS stores it, K_DPHI_SERIES folds it).  Only the real part of the column
// transform is used, and with Th[su] = (T[su] + conj(T[-su])) / 2
//     Re sum_su T[su] W^(su x) = sum_su Th[su] W^(su x),   Th[-su] = conj(Th[su]),   su in [-40, 40]
// for any patch.  The edge row su = -40 has no partner inside the patch and is its own pair: Th[-40] = T[-40] / 2,
// Th[40] = conj(T[-40]) / 2.  A line is the kNH = 41 values (kernels.h) U[su] = c Th[su], su = 0 .. 40, with c = 1 for su = 0
// and c = 2 otherwise: a pair counts twice, and the doubling is exact.  For the fold su = r + Q j the symmetry reads
// S_(Q - r) = conj(S_r): the classes r = 0 .. Q/2 are formed,
//     r = 0:        S_0 = U[0] + sum_(j < 0) Re(conj(U[-Q j]) W_L^(j k2))           (real; the pairs through su < 0)
//     r = Q/2:      S_(Q/2) = Re(W_N^(r k2) sum_(j >= 0) U[r + Q j] W_L^(j k2))      (real; the pairs through su > 0)
//     0 < r < Q/2:  S'_r = 2 S_r = W_N^(r k2) sum_j Uh[r + Q j] W_L^(j k2),  Uh[su] = U[su], Uh[-su] = conj(U[su]),
// and X[k1] = S_0 + (-1)^k1 S_(Q/2) + sum_(0 < r < Q/2) Re(S'_r W_Q^(r k1)).  su = +-40 falls in class Q/2 (Q = 16) or
// 0 (Q = 2, 4, 8, 20), never in a general one.
constexpr bool hfold_valid(int Q, int r, int j) {
    const int su = r + Q * j;
    return su >= -NAO / 2 && su <= NAO / 2 && (2 * r != Q || j >= 0);
}

template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// Re(W_Q^m z), and acc + Re(W_Q^m z); the trivial factors are resolved at compile time
template <int Q, int MM>
__device__ __forceinline__ double re_w(const cx<double>& z) {
    constexpr int m = ((MM % Q) + Q) % Q;
    constexpr double c = WQ<Q>::c[m], s = WQ<Q>::s[m];
    if constexpr (c == 1.0) return z.x;
    else if constexpr (c == -1.0) return -z.x;
    else if constexpr (s == 1.0) return -z.y;
    else if constexpr (s == -1.0) return z.y;
    else return fma(-s, z.y, c * z.x);
}
template <int Q, int MM>
__device__ __forceinline__ double add_re_w(double acc, const cx<double>& z) {
    constexpr int m = ((MM % Q) + Q) % Q;
    constexpr double c = WQ<Q>::c[m], s = WQ<Q>::s[m];
    if constexpr (c == 1.0) return acc + z.x;
    else if constexpr (c == -1.0) return acc - z.x;
    else if constexpr (s == 1.0) return acc - z.y;
    else if constexpr (s == -1.0) return acc + z.y;
    else return fma(-s, z.y, fma(c, z.x, acc));
}

// X[k1] = sum_(r < Q) S_r W_Q^(r k1), k1 = 0 .. Q-1, for a Hermitian sequence S_(Q - r) = conj(S_r): a complex-to-real
// transform.  Q = 4 M: r = 4 r2 + r1, k1 = M a + b, and with V_r1[b] = sum_r2 S_(4 r2 + r1) W_Q^((4 r2 + r1) b)
//     X[M a + b] = V_0[b] + (-1)^a V_2[b] + 2 Re((-i)^a V_1[b]):
// V_0 and V_2 are real (their classes are conjugate pairs within themselves) and V_3 = conj(V_1), which is never
// formed; V_1 is the one complex M-point transform left, over the odd classes 1, 3, .. Q/2 - 1 and the conjugates of
// the same in reverse.  s0 = S_0; EV(v) fills v[i] = S'_(2 + 2 i), i < M, of which the last is the real S_(Q/2) (in
// .x); OD(v) fills v[i] = S'_(1 + 2 i), i < M (S' = 2 S: see above).  The caller produces the sums of one group at a
// time, so that at Q = 20 only 5 of them are alive beside the partial results.
template <int Q, typename FE, typename FO>
__device__ __forceinline__ void dftq_herm_real_out(double s0, FE&& EV, FO&& OD, double* out) {
    static_assert(Q % 4 == 0, "Q = 2 is handled by the caller");
    constexpr int M = Q / 4;
    double t0[M], t1[M], t2[M], t3[M];
    {
        cx<double> e[M];
        EV(e);
        const double sh = e[M - 1].x;
        static_for<0, M>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            const double shb = b % 2 ? -sh : sh;                   // (-1)^b S_(Q/2)
            double v0, v2;
            if constexpr (M % 2 == 0) {                            // Q/2 = 0 mod 4; class 2 is a general one
                v0 = s0 + shb;
                v2 = re_w<Q, 2 * b>(e[0]);
            } else {                                               // Q/2 = 2 mod 4
                v0 = s0;
                v2 = shb;
            }
            static_for<(M % 2 == 0 ? 1 : 0), M - 1>([&](auto ic) {
                constexpr int r = 2 + 2 * decltype(ic)::value;
                if constexpr (r % 4 == 0) v0 = add_re_w<Q, r * b>(v0, e[decltype(ic)::value]);
                else v2 = add_re_w<Q, r * b>(v2, e[decltype(ic)::value]);
            });
            t0[b] = v0 + v2;
            t1[b] = v0 - v2;
        });
    }
    {
        cx<double> o[M], v[M];
        OD(o);
#pragma unroll
        for (int r2 = 0; r2 < M; ++r2) {
            const int r = 4 * r2 + 1;
            if (2 * r < Q) v[r2] = o[(r - 1) / 2];
            else v[r2] = {o[(Q - r - 1) / 2].x, -o[(Q - r - 1) / 2].y};
        }
        dftm<M>(v);
#pragma unroll
        for (int b = 0; b < M; ++b) {
            if (b == 0) {
                t2[b] = v[b].x;
                t3[b] = v[b].y;
            } else {
                t2[b] = v[b].x * WQ<Q>::c[b] - v[b].y * WQ<Q>::s[b];
                t3[b] = v[b].x * WQ<Q>::s[b] + v[b].y * WQ<Q>::c[b];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < M; ++b) {
        out[b] = t0[b] + t2[b];
        out[2 * M + b] = t0[b] - t2[b];
        out[M + b] = t1[b] + t3[b];
        out[3 * M + b] = t1[b] - t3[b];
    }
}

// 16-point transform in registers (natural order): 4 x 4
__device__ __forceinline__ void dft16(cx<double>* v) {
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) dft4(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
#pragma unroll
    for (int k1 = 1; k1 < 4; ++k1)
#pragma unroll
        for (int n2 = 1; n2 < 4; ++n2) {
            const cx<double> w = {WQ<16>::c[n2 * k1], WQ<16>::s[n2 * k1]};
            v[4 * k1 + n2] = cmul(v[4 * k1 + n2], w);
        }
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) dft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
    cx<double> o[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) o[k1 + 4 * k2] = v[4 * k1 + k2];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = o[i];
}

template <int Q>
__device__ __forceinline__ void dftq(cx<double>* v) {
    if constexpr (Q == 16) dft16(v);
    else dftr<double, Q>(v);
}

// ------------------------------------------------------------------------------------------
// Broadcast operands.  Every lane of a wave needs the same inputs of a fold (80 real ones in K_PATCH_ROWS, 41
// complex ones in K_DPHI_SERIES), each multiplied by the lane's own twiddle.  They travel in 5 (3) register pairs
// per component -- lane l holds input 16 a + (l mod 16) in pair a, the same in all four rows of 16 lanes -- and the
// multiply-add picks its
// lane with the DPP control row_newbcast (the one DPP control gfx90a+ has for 64-bit operations):
// no LDS read, no scalar load, no extra instruction per operand.  (Through the scalar cache, the
// first form of this kernel, the 1280 bytes per line and task were 26 s_load per 440 vector
// instructions and the waves waited 68 % of their cycles for them.)
// hipcc does not pad the wait states of an instruction inside an asm statement: a VGPR written by a
// vector instruction must not be read through DPP within 2 wait states.  The operands below come out
// of global loads; tools/isa_lint.py (R6) checks every DPP instruction of the build.
// ------------------------------------------------------------------------------------------
template <int LANE>
__device__ __forceinline__ double mov_bc(double x) {                             // x[LANE]
    double d;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(x), "n"(LANE));
    return d;
}

template <int LANE>
__device__ __forceinline__ void fmac_bc(double& acc, double x, double w) {       // acc += x[LANE] * w
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(w), "n"(LANE));
}

constexpr int kNX = NAO / 16;        // register pairs of the 80 real inputs of a fold of K_PATCH_ROWS
constexpr int kNXH = (kNH + 15) / 16;  // register pairs per component of the 41 complex inputs of a line

// The sums of a group of CNT residues r_i = R0 + RS i:  acc[i] = sum_j in[r_i + Q j] W_64^(j k2)
// (the factor W_N^(r k2) is the caller's), wj[j - JMIN] = W_64^(j k2).  HERM = false: the 80 real inputs of
// K_PATCH_ROWS, xr = broadcast operands with index su + 40 (xi unused).  HERM = true: the Hermitian half of a line,
// xr / xi with index |su|, conjugated where su < 0 (all of a term's residues are on one side: r < Q) and the terms of
// hfold_valid.  Term by term over j, all residues of the group in one multiply-add block (dpp_groups.h): the
// accumulators of the group are the independent chains that cover the latency of the fp64 DPP multiply-add.
template <int Q, bool HERM, int R0, int RS, int CNT, int J>
struct FoldValid {
    int n = 0, idx[CNT > 0 ? CNT : 1] = {};
    constexpr FoldValid() {
        for (int i = 0; i < CNT; ++i)
            if (HERM ? hfold_valid(Q, R0 + RS * i, J) : fold_valid(Q, R0 + RS * i, J)) idx[n++] = i;
    }
};

template <int Q, bool HERM, int R0, int RS, int CNT, int J = fold_jmin<Q>()>
__device__ __forceinline__ void fold_group(cx<double>* acc, const double* xr, const double* xi,
                                           const cx<double>* wj) {
    if constexpr (J < fold_jmax<Q>()) {
        constexpr FoldValid<Q, HERM, R0, RS, CNT, J> V;
#define MPSFR_FSU(k) (R0 + RS * V.idx[k] + Q * J)                /* su of the k-th valid residue */
#define MPSFR_FN(k) (HERM ? (MPSFR_FSU(k) < 0 ? -MPSFR_FSU(k) : MPSFR_FSU(k)) : MPSFR_FSU(k) + NAO / 2)   /* input index */
#define MPSFR_FA(k) acc[V.idx[k]]
#define MPSFR_FX(k) xr[MPSFR_FN(k) / 16], xi[MPSFR_FN(k) / 16]
#define MPSFR_FR(k) xr[MPSFR_FN(k) / 16]
#define MPSFR_FL(k) MPSFR_FN(k) % 16
#define MPSFR_FGROUPS(mac, X)                                                                                  \
    if constexpr (n == 5)                                                                                      \
        mac##_group5<MPSFR_FL(0), MPSFR_FL(1), MPSFR_FL(2), MPSFR_FL(3), MPSFR_FL(4)>(                         \
            MPSFR_FA(0), MPSFR_FA(1), MPSFR_FA(2), MPSFR_FA(3), MPSFR_FA(4), X(0), X(1), X(2), X(3), X(4), w); \
    if constexpr (n == 4)                                                                                      \
        mac##_group4<MPSFR_FL(0), MPSFR_FL(1), MPSFR_FL(2), MPSFR_FL(3)>(                                      \
            MPSFR_FA(0), MPSFR_FA(1), MPSFR_FA(2), MPSFR_FA(3), X(0), X(1), X(2), X(3), w);                    \
    if constexpr (n == 2 || n == 3)                                                                            \
        mac##_group2<MPSFR_FL(0), MPSFR_FL(1)>(MPSFR_FA(0), MPSFR_FA(1), X(0), X(1), w);                       \
    if constexpr (n == 3) mac##_group1<MPSFR_FL(2)>(MPSFR_FA(2), X(2), w);                                     \
    if constexpr (n == 1) mac##_group1<MPSFR_FL(0)>(MPSFR_FA(0), X(0), w);
        if constexpr (J == 0) {          // the twiddle is 1 (and su = r >= 0)
            static_for<0, V.n>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                acc[V.idx[k]].x += mov_bc<MPSFR_FL(k)>(xr[MPSFR_FN(k) / 16]);
                if constexpr (HERM) acc[V.idx[k]].y += mov_bc<MPSFR_FL(k)>(xi[MPSFR_FN(k) / 16]);
            });
        } else {
            const cx<double> w = wj[J - fold_jmin<Q>()];
            constexpr int n = V.n;
            static_assert(n <= 5, "group sizes up to 5");
            if constexpr (!HERM) {
                MPSFR_FGROUPS(rmac, MPSFR_FR)
            } else if constexpr (J < 0) {
                MPSFR_FGROUPS(cmacc, MPSFR_FX)
            } else {
                MPSFR_FGROUPS(cmac, MPSFR_FX)
            }
        }
#undef MPSFR_FGROUPS
#undef MPSFR_FSU
#undef MPSFR_FN
#undef MPSFR_FA
#undef MPSFR_FX
#undef MPSFR_FR
#undef MPSFR_FL
        fold_group<Q, HERM, R0, RS, CNT, J + 1>(acc, xr, xi, wj);
    }
}

// v[i] = S_r (HERM: S'_r) for r = R0 + RS i, i < CNT, the factor W_N^(r k2) = wrf(r) included.  The class Q/2 of a
// Hermitian line is real: only v[i].x = Re(W_N^(r k2) sum) is formed, one multiply-add pair.
template <int Q, bool HERM, int R0, int RS, int CNT, typename WR>
__device__ __forceinline__ void fold_sums(cx<double>* v, const double* xr, const double* xi,
                                          const cx<double>* wj, WR&& wrf) {
#pragma unroll
    for (int i = 0; i < CNT; ++i) v[i] = {0.0, 0.0};
    fold_group<Q, HERM, R0, RS, CNT>(v, xr, xi, wj);
#pragma unroll
    for (int i = 0; i < CNT; ++i) {
        const int r = R0 + RS * i;
        if (HERM && 2 * r == Q) {
            const cx<double> w = wrf(r);
            v[i] = {fma(-v[i].y, w.y, v[i].x * w.x), 0.0};
        } else if (r > 0) {
            v[i] = cmul(v[i], wrf(r));
        }
    }
}

// S_0 of a Hermitian line without its term U[0]: sum_(j < 0) Re(conj(U[-Q j]) W_L^(j k2)), in two chains
template <int Q, int J = fold_jmin<Q>()>
__device__ __forceinline__ void fold_class0(double& a, double& b, const double* xr, const double* xi,
                                            const cx<double>* wj) {
    if constexpr (J < 0) {
        if constexpr (Q * J >= -NAO / 2) {
            constexpr int n = -Q * J;
            const cx<double> w = wj[J - fold_jmin<Q>()];
            fmac_bc<n % 16>(a, xr[n / 16], w.x);
            fmac_bc<n % 16>(b, xi[n / 16], w.y);
        }
        fold_class0<Q, J + 1>(a, b, xr, xi, wj);
    }
}

// ------------------------------------------------------------------------------------------
// The twiddles of a lane, laid out per lane: twk[j - JMIN][k2] = W_64^(j k2) for the NJ fold terms,
// then twk[NJ + r][k2] = W_N^(r k2) for r < Q.  Built once per context: a wave reads a row of the
// table as 1 KB of consecutive bytes, where twg[(r k2) mod N] straight from the table of N-th roots
// is a gather of 64 cache lines per instruction -- the 16 such gathers at the head of every wave of
// K_PATCH_ROWS kept its vector-memory pipe full and the waves at 40 cycles per instruction.
// ------------------------------------------------------------------------------------------
// L: lanes per line (64 in K_PATCH_ROWS; series_lanes<N>() in K_DPHI_SERIES), Q = N / L
template <int N, int L>
__global__ void __launch_bounds__(64) k_series_twiddles(const cx<double>* __restrict__ twg,
                                                        cx<double>* __restrict__ twk) {
    constexpr int Q = N / L, NJ = fold_nj<Q>(), JMIN = fold_jmin<Q>();
    const int row = blockIdx.x, k2 = threadIdx.x;
    if (k2 >= L) return;
    if (row < NJ) twk[row * L + k2] = twg[(((Q * (row + JMIN) * k2) % N) + N) % N];
    else twk[row * L + k2] = twg[((row - NJ) * k2) % N];
}

// Lanes per line of K_DPHI_SERIES.  A wave carries 64 / L lines (the same y, consecutive tasks): the
// fold costs 320 multiply-adds per WAVE whatever L is -- each row of 16 lanes holds its own line's
// inputs as broadcast operands -- while the in-lane transform grows with Q = N / L.  Q = 16 wherever
// the grid allows it (512^2: two lines per wave, 560 -> 330 instructions per line; 256^2: four).
template <int N>
constexpr int series_lanes() { return N <= 256 ? 16 : (N == 512 ? 32 : 64); }
template <int N, int L>
constexpr size_t twiddle_entries() { return (size_t)(fold_nj<N / L>() + N / L) * L; }

// ------------------------------------------------------------------------------------------
// K_PATCH_GEN: P[td][su + 40][sv + 40] = max(F, AO) - F on the corrected zone (psfrec.py:148-149;
// F and AO exactly as K_PSD_ROWFFT evaluates them).  A thread is (task, pixel) and walks the task's
// directions: the fitting term and the von Karman factor of the pixel -- two x^(-11/6), nearly all of
// the arithmetic -- do not depend on the direction, only the tables do (nine directions: 21.6 -> us).
// ------------------------------------------------------------------------------------------
// Mix: empty (a legacy call, the kernel as it was before profiles existed) or (const double* w, int ntab): a profile
// call, the row's weights w[task][ntab] and ntab + 1 tables per direction
template <bool F64, typename... Mix>
__global__ void __launch_bounds__(256) k_patch_gen(int ndir, const TaskPar* __restrict__ tp,
                                                   const double* __restrict__ aotab, double cfit,
                                                   double* __restrict__ P, Mix... mix) {
    constexpr int NEWTON = F64 ? 2 : 1;
    const int task = blockIdx.y;
    const TaskPar p = tp[task];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= NAO * NAO) return;
    const int su = pix / NAO - NAO / 2, sv = pix % NAO - NAO / 2;
    const double fit = psd_fit_value<NEWTON>(su, sv, p, cfit);
    const int ia = su < 0 ? su + NAO : su, ib = sv < 0 ? sv + NAO : sv;
    const double g2 = (double)(su * su + sv * sv) * (1.0 / 256.0);
    const double vk = 0.0229 * p.r0m53 * pow_m11_6<NEWTON>(g2 + p.inv_l0sq);        // :569-571
    const int o = ia * NAO + ib;
    if constexpr (sizeof...(Mix) > 0) {
        const double* w;
        int ntab;
        mix_args(w, ntab, mix...);
        w += (size_t)task * ntab;
        for (int d = 0; d < ndir; ++d) {
            const double* tb = aotab + ((size_t)(p.geom * ndir + d) * (ntab + 1)) * (NAO * NAO);
            // (the first two terms taken are the legacy expression: a two-layer profile gives the legacy bits)
            const double ao = vk * ao_mix_sum(tb, o, w, ntab) + tb[ntab * NAO * NAO + o];
            P[((size_t)task * ndir + d) * (NAO * NAO) + pix] = fmax(fit, ao) - fit;          // :149
        }
        return;
    }
    if (ndir == 1) {
        const double* tb = aotab + ((size_t)p.geom * 3) * (NAO * NAO);
        const double ao = vk * (p.cn2_0 * tb[o] + p.cn2_1 * tb[NAO * NAO + o]) + tb[2 * NAO * NAO + o];
        P[(size_t)task * (NAO * NAO) + pix] = fmax(fit, ao) - fit;                           // :149
        return;
    }
    // (nine directions at a time with their table loads in flight together: one at a time, the loop was
    // nine memory latencies long)
    for (int d0 = 0; d0 < ndir; d0 += 9) {
        double t0[9], t1[9], t2[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int d = min(d0 + i, ndir - 1);
            const double* tb = aotab + ((size_t)(p.geom * ndir + d) * 3) * (NAO * NAO);
            t0[i] = tb[o];
            t1[i] = tb[NAO * NAO + o];
            t2[i] = tb[2 * NAO * NAO + o];
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            if (d0 + i >= ndir) break;
            const double ao = vk * (p.cn2_0 * t0[i] + p.cn2_1 * t1[i]) + t2[i];
            P[((size_t)task * ndir + d0 + i) * (NAO * NAO) + pix] = fmax(fit, ao) - fit;     // :149
        }
    }
}

// ------------------------------------------------------------------------------------------
// K_PATCH_ROWS: the row transforms Trow[su][y] = sum_sv P[su][sv] exp(-2 pi i sv y / N), y in [0, N/2], stored as
// the Hermitian half of a line (above): T[td][y][su] = U[su] = Trow[su] + conj(Trow[-su]) for su = 1 .. 39,
// U[0] = Re Trow[0], U[40] = conj(Trow[-40]); and sp[td] = sum P.  A wave takes one, two or four adjacent rows su at
// a time: lane k2 folds a row's 80 values (broadcast operands) into Q sums with its own twiddles, transforms them in
// registers and owns y = k2, 64 + k2, ...  K_DPHI_SERIES reads the 41 values of one (td, y) as 656 contiguous bytes
// (with T[td][su][y] every line of it gathered 80 cache lines: 12 of its 50 us at 512^2).
// ------------------------------------------------------------------------------------------
// L = series_lanes<N>() lanes per row, R = 64 / L rows per wave and pass (one per group of L lanes),
// Q = N / L: the same fold and in-lane transform as K_DPHI_SERIES, with a real input and a complex
// output of which y <= N/2 is kept.  A workgroup takes `qb` groups of 4 R rows of one td, one group per pass, a row
// set per wave: the 2 R adjacent rows su = -40 + 2 R g + s (s < 2 R) and their partners -su, so that every pair
// meets in the pass's LDS tile [y][4 R rows] (the partner slot of su = -40, which has none, carries su = 0).  The
// pairs are combined in fp64 on the way out, U = Trow[-su'] + conj(Trow[su']) for su' < 0, and leave as pieces of
// 2 R x 16 bytes (32 bytes at 1280^2, 128 at 256^2): a lane storing its own y values wrote 16-byte pieces a line
// apart, and at 1280^2 that alone took 25 of the kernel's 45 us.
template <int N>
constexpr size_t patch_rows_smem() { return (size_t)(N / 2 + 1) * (4 * (64 / series_lanes<N>()) + 1) * sizeof(cx<double>); }

// Round 6: the workgroups with blockIdx.y >= ntd are not rows of the patch: they compute the spectra of the chunk's
// tip-tilt Moffat kernels (the body of K_KHAT, conv_frames.h; KR = float / double, void: none) -- a kernel of its
// own at the head of every call until now (8 us alone, 16-48 us parked behind the other lane's K_OTF_MFMA2 in the
// pipelined run) whose LDS footprint is this kernel's.
template <int N, typename KR>
constexpr size_t patch_rows_smem_all() {
    if constexpr (std::is_void<KR>::value) return patch_rows_smem<N>();
    else return patch_rows_smem<N>() > conv_smem_bytes<KR>(true) ? patch_rows_smem<N>() : conv_smem_bytes<KR>(true);
}

template <int N, typename KR>
__global__ void __launch_bounds__(256) k_patch_rows(const double* __restrict__ P,
                                                    const cx<double>* __restrict__ twk,
                                                    cx<double>* __restrict__ T, double* __restrict__ sp, int qb,
                                                    int ntd, PatchKhat kh) {
    constexpr int L = series_lanes<N>(), R = 64 / L, Q = N / L, H1 = N / 2 + 1, NJ = fold_nj<Q>();
    if constexpr (!std::is_void<KR>::value) {
        if ((int)blockIdx.y >= ntd) {
            extern __shared__ __align__(16) unsigned char smem_k[];
            const int kid = ((int)blockIdx.y - ntd) * (int)gridDim.x + (int)blockIdx.x;
            if (kid < kh.n) khat_body<KR>(kh.gam, kh.alp, (cx<KR>*)kh.out, smem_k, kid);
            return;
        }
    }
    constexpr bool WJREG = NJ <= 10;
    constexpr int NY = Q / 2 + 1;                        // values y = L k1 + k2 <= N/2 of a lane
    constexpr int RG = 4 * R, RS = RG + 1;               // rows per pass of the workgroup; padded tile row
    constexpr int RH = RG / 2;                           // pairs per pass: slots [0, RH) su < 0, [RH, RG) the partners
    constexpr int NG = NAO / RG;                         // passes per td
    extern __shared__ __align__(16) unsigned char smem[];
    cx<double>* tile = reinterpret_cast<cx<double>*>(smem);          // [H1][RS]
    __shared__ double sred[256];
    const int td = blockIdx.y;
    const double* Pg = P + (size_t)td * (NAO * NAO);
    const int lane = threadIdx.x & 63, rho = lane / L, k2 = lane & (L - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g_end = min(NG, ((int)blockIdx.x + 1) * qb);
    int g = blockIdx.x * qb;
    double xa[kNX], xb[kNX];
    auto fetch = [&](int gg, double* xr) {
        const int q = R * wave + rho, i = RH * gg + (q < RH ? q : q - RH);       // i = 40 - |su| of the slot's pair
        const int row = q < RH ? i : (i == 0 ? NAO / 2 : NAO - i);
#pragma unroll
        for (int a = 0; a < kNX; ++a) xr[a] = Pg[row * NAO + 16 * a + (lane & 15)];
    };
    if (g < g_end) fetch(g, xa);
    if (blockIdx.x == 0) {      // sum of the patch, in an order fixed by the launch geometry
        double a = 0.0;
        for (int i = threadIdx.x; i < NAO * NAO; i += 256) a += Pg[i];
        sred[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x < 64) {
            double b = (sred[threadIdx.x] + sred[threadIdx.x + 64]) + (sred[threadIdx.x + 128] + sred[threadIdx.x + 192]);
            b = wave_sum(b);
            if (threadIdx.x == 0) sp[td] = b;
        }
    }
    cx<double> wjr[WJREG ? NJ : 1], wr[Q];
    if constexpr (WJREG) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) wjr[j] = twk[j * L + k2];
    }
#pragma unroll
    for (int r = 1; r < Q; ++r) wr[r] = twk[(NJ + r) * L + k2];
    auto pass = [&](int gg, const double* xr) {
        cx<double> S[Q];
        {
            constexpr int GC = Q % 5 == 0 ? 5 : (Q < 4 ? Q : 4);
            cx<double> wl[WJREG ? 1 : NJ];
            if constexpr (!WJREG) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) wl[j] = twk[j * L + k2];
            }
            const cx<double>* wjp = WJREG ? wjr : wl;
            static_for<0, Q / GC>([&](auto gc) {
                constexpr int R0 = decltype(gc)::value * GC;
                fold_sums<Q, false, R0, 1, GC>(S + R0, xr, xr, wjp, [&](int r) { return wr[r]; });
            });
        }
        dftq<Q>(S);
#pragma unroll
        for (int k1 = 0; k1 < NY; ++k1)
            if (L * k1 + k2 <= N / 2) tile[(L * k1 + k2) * RS + R * wave + rho] = S[k1];
        __syncthreads();
        cx<double>* Tt = T + (size_t)td * H1 * kNH;
        for (int e = threadIdx.x; e < H1 * RH; e += 256) {
            const int y = e / RH, sl = e % RH, i = RH * gg + sl;
            const cx<double> vn = tile[y * RS + sl], vp = tile[y * RS + RH + sl];
            if (i == 0) {       // su = -40 alone, and su = 0 in its partner's slot
                Tt[(size_t)y * kNH + NAO / 2] = {vn.x, -vn.y};
                Tt[(size_t)y * kNH] = {vp.x, 0.0};
            } else {
                Tt[(size_t)y * kNH + NAO / 2 - i] = {vp.x + vn.x, vp.y - vn.y};
            }
        }
        __syncthreads();
    };
    while (g < g_end) {
        if (g + 1 < g_end) fetch(g + 1, xb);
        pass(g, xa);
        g += 1;
        if (g >= g_end) break;
        if (g + 1 < g_end) fetch(g + 1, xa);
        pass(g, xb);
        g += 1;
    }
}

// ------------------------------------------------------------------------------------------
// K_DPHI_SERIES: D0t[td][y][x] = r0^(-5/3) sum_k delta^k Hd_k[y][x] + scale2 (sp - Re X[x]) with
// Re X[x] = Re sum_su Trow[su] exp(-2 pi i su x / N) from the Hermitian half T[td][y][0 .. 40] of the line.  A wave
// takes one (td, y) at a time ("a line"): the 41 complex inputs are broadcast operands (above), lane k2 owns
// x = k2, 64 + k2, ...
//   coef: [y][x][K] (K fp32 / fp64 terms of pixel (y, x) side by side), staged in LDS per line y.
// ------------------------------------------------------------------------------------------
template <typename RO> struct SeriesCfg;
template <> struct SeriesCfg<float> { static constexpr int K = 4; };
template <> struct SeriesCfg<double> { static constexpr int K = 8; };

// Minima over each row of 16 lanes of NV values at once (NV a power of two <= 16), transposed: at a step that pairs the
// lanes l and l ^ B (in the order row_mirror, row_half_mirror, quad_perm [2,3,0,1], [1,0,3,2] every partner agrees with
// the lane in the bits already used), the lanes with bit B clear go on with the first half of the values and the others
// with the second: two selects and one DPP minimum per PAIR of values, and lane l ends with the row's minimum of value
// l % NV -- the lane that stores it.  With fewer values than 2 B a step is a plain minimum of every value.  16 values:
// 46 instructions with the step over the two rows of a line, where five v_min_f32_dpp steps per value and a compare
// and a select to pick each value's lane were 112.  The DPP operand is the builtin's: hipcc folds the move into
// v_min_i32_dpp and pads its wait states itself (tools/isa_lint.py R6 still checks them).
template <int CTRL>
__device__ __forceinline__ float min_dpp(float mine, float sent) {
    // (no value is below -0 or a NaN: the order of the bit patterns as signed integers is the order of the values, and
    // an integer minimum needs no canonical operands, so the DPP move folds into it)
    const int a = __float_as_int(mine);
    const int b = __builtin_amdgcn_update_dpp(0, __float_as_int(sent), CTRL, 0xf, 0xf, true);
    return __int_as_float(a < b ? a : b);
}
template <int NV, int B = 8>
__device__ __forceinline__ void rowmin_transposed(float* v, int lane) {
    constexpr int CTRL = B == 8 ? 0x140 : (B == 4 ? 0x141 : (B == 2 ? 0x4E : 0xB1));
    if constexpr (NV > B) {
        static_assert(NV == 2 * B, "a power of two");
        const bool hi = (lane & B) != 0;
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const float a = v[j], b = v[j + B];
            v[j] = min_dpp<CTRL>(hi ? b : a, hi ? a : b);
        }
        if constexpr (B > 1) rowmin_transposed<B, B / 2>(v, lane);
    } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = min_dpp<CTRL>(v[j], v[j]);
        if constexpr (B > 1) rowmin_transposed<NV, B / 2>(v, lane);
    }
}

// The lines of a wave: xv = their inputs (lane l holds input min(16 a + l % 16, 40) of ITS line in xv[a]),
// wjp[j - JMIN] = W_L^(j k2) of the lane, swr[r * L + k2] = W_N^(r k2) (LDS), scoef = the coefficients
// of line y (LDS, [x][K]); r0m53, delta, spv, dst, dlin: the lane's line (td); k2 = lane % L.
template <int N, typename RO, int L>
__device__ __forceinline__ void series_line(const cx<double>* xv, const cx<double>* wjp,
                                            const cx<double>* swr, const RO* scoef, double r0m53,
                                            double delta, double spv, double scale2, RO* dst, float* dlin,
                                            bool valid, int lane, unsigned kmask) {
    // kmask (wave-uniform): bit k1 set = some column x in [L k1, L k1 + L) of this line lies inside the support of
    // the telescope OTF (K_SERIES_SUPPORT).  Outside it the OTF is identically zero whatever the structure function
    // (psfrec.py:784-797): the polynomial, the store and the minimum of such a piece are skipped -- 21 % of the half
    // plane; what the per-wavelength stage reads there is the zero the buffer was allocated with.
    constexpr int Q = N / L, K = SeriesCfg<RO>::K;
    constexpr float kSkipped = 3.0e38f;
    const int k2 = lane & (L - 1);
    double xr[kNXH], xi[kNXH];
#pragma unroll
    for (int a = 0; a < kNXH; ++a) {
        xr[a] = xv[a].x;
        xi[a] = xv[a].y;
    }
    double out[Q];
    // A branch hipcc cannot fold (the flag comes out of an asm statement and is always 1): the join
    // behind it pins `out` in registers and keeps the fold and the transform apart from the
    // polynomial phase.  As one basic block the 1280^2 kernel with the 80-input fold was allocated 256 registers
    // + 124 bytes of scratch instead of 238 + 0 and took 246 us instead of 180; scheduling fences alone
    // (__builtin_amdgcn_sched_barrier) do not change that.  With the Hermitian fold the kernel needs 144: without
    // the branch it has 16-20 fewer 64-bit moves per unit, the same time within 0.1 us at 512^2, 161 registers at
    // 1280^2 -- and hipcc contracts the multiply-adds of the transform differently, so that the f64-mode structure
    // function changes in its last bit.  The branch stays.
    int always;
    asm volatile("s_mov_b32 %0, 1" : "=s"(always));
    if (!always) {
#pragma unroll
        for (int k1 = 0; k1 < Q; ++k1) out[k1] = xr[k1 % kNXH];
    } else {
        auto wrf = [&](int r) { return swr[r * L + k2]; };
        static_assert((NAO / 2) % Q == 0 || (NAO / 2) % Q == Q / 2, "su = +-40 falls in a self-conjugate class");
        double s0 = mov_bc<0>(xr[0]), s0b = 0.0;
        fold_class0<Q>(s0, s0b, xr, xi, wjp);
        s0 += s0b;
        if constexpr (Q == 2) {
            cx<double> S[1];
            fold_sums<Q, true, 1, 2, 1>(S, xr, xi, wjp, wrf);
            out[0] = s0 + S[0].x;
            out[1] = s0 - S[0].x;
        } else {
            // the even classes 2 .. Q/2, then the odd ones: Q / 4 = 4 or 5 independent accumulator pairs each
            dftq_herm_real_out<Q>(
                s0, [&](cx<double>* v) { fold_sums<Q, true, 2, 2, Q / 4>(v, xr, xi, wjp, wrf); },
                [&](cx<double>* v) { fold_sums<Q, true, 1, 2, Q / 4>(v, xr, xi, wjp, wrf); }, out);
        }
    }
    // Block minima for the pruning of the per-wavelength stage, while the values are in registers
    // (K_DMIN read all of D back for them: 12 us at 512^2, 69 us at 1280^2): the minimum of max(D, 0)
    // over the 32 columns [32 kb, 32 kb + 32) of the line goes to dlin[kb]; K_DMIN16 takes the minima
    // over 16 lines.  A lane's values are x = L k1 + k2:
    //   L = 64: kb = 2 k1 + (lane >= 32): the rows of 16 lanes (rowmin_transposed), then rows 1 and 3 take the minimum
    //           with the row before them; lane 16 + k1 % 16 (48 + k1 % 16) holds the result of k1;
    //   L = 32: kb = k1, the 32 lanes of a line; the same, lanes 16-31 / 48-63 are the two lines;
    //   L = 16: kb = k1 / 2: the two values of a lane first, then the row of 16 lanes; lane kb % 16 of the line's
    //           row holds kb.
    constexpr int NB = L == 16 ? Q / 2 : Q;              // values per lane that go into the lane minima
    float keep[(NB + 15) / 16], dq[Q];
#pragma unroll
    for (int i = 0; i < (NB + 15) / 16; ++i) keep[i] = 0.f;
    // The pieces of a line in groups of G: one wave-uniform test skips a group with no piece inside the support;
    // otherwise the coefficients of all G pieces are read together (the whole line is in LDS: reading a skipped
    // piece's is harmless) and their polynomials run side by side -- one LDS wait and G independent chains per
    // basic block instead of a branch, a read and a wait per piece.  A piece outside the support is still never
    // stored and its dq is the sentinel; a group that lies wholly inside (most) tests no piece.
    constexpr int G = sizeof(RO) == 4 ? (Q < 4 ? Q : 4) : 2;
    constexpr unsigned kFull = (1u << G) - 1u;
    static_assert(Q % G == 0, "whole groups");
    auto lane_min = [](RO d) {      // (f64: rounded down, the bound stays a bound)
        if constexpr (sizeof(RO) == 4) return fmaxf(d, 0.f);
        else return fmaxf(__double2float_rd(d), 0.f);
    };
    auto finish_group = [&](int k0, unsigned gm, const RO* d) {
        if (sizeof(RO) == 4 && gm == kFull) {
#pragma unroll
            for (int i = 0; i < G; ++i) dq[k0 + i] = lane_min(d[i]);
            if (valid) {
#pragma unroll
                for (int i = 0; i < G; ++i) dst[L * (k0 + i)] = d[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < G; ++i) dq[k0 + i] = ((gm >> i) & 1u) ? lane_min(d[i]) : kSkipped;
            if (valid) {
#pragma unroll
                for (int i = 0; i < G; ++i)
                    if ((gm >> i) & 1u) dst[L * (k0 + i)] = d[i];
            }
        }
    };
    const float df = (float)delta, rf = (float)r0m53;
#pragma unroll
    for (int k0 = 0; k0 < Q; k0 += G) {
        const unsigned gm = (kmask >> k0) & kFull;
        if (gm == 0u) {
#pragma unroll
            for (int i = 0; i < G; ++i) dq[k0 + i] = kSkipped;
            continue;
        }
        RO d[G];
        if constexpr (sizeof(RO) == 4) {
            float4 h[G];
#pragma unroll
            for (int i = 0; i < G; ++i) h[i] = *reinterpret_cast<const float4*>(scoef + (size_t)(L * (k0 + i) + k2) * K);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const float dF = rf * fmaf(fmaf(fmaf(h[i].w, df, h[i].z), df, h[i].y), df, h[i].x);
                d[i] = (float)(fma(scale2, spv - out[k0 + i], (double)dF));
            }
        } else {
            double a[G];
#pragma unroll
            for (int i = 0; i < G; ++i) a[i] = scoef[(size_t)(L * (k0 + i) + k2) * K + K - 1];
#pragma unroll
            for (int k = K - 2; k >= 0; --k) {
#pragma unroll
                for (int i = 0; i < G; ++i) a[i] = fma(a[i], delta, scoef[(size_t)(L * (k0 + i) + k2) * K + k]);
            }
#pragma unroll
            for (int i = 0; i < G; ++i) d[i] = fma(scale2, spv - out[k0 + i], r0m53 * a[i]);
        }
        finish_group(k0, gm, d);
    }
    if (dlin != nullptr) {
        // values 16 i .. 16 i + 15 (or what is left of them, a power of two) at a time: lane 16 i + l % 16 of a row of
        // lanes ends with the row's minimum of value 16 i + l % 16
        if constexpr (L == 16) {
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) dq[kb] = fminf(dq[2 * kb], dq[2 * kb + 1]);
        }
        static_for<0, (NB + 15) / 16>([&](auto ic) {
            constexpr int i = decltype(ic)::value, NV = NB - 16 * i < 16 ? NB - 16 * i : 16;
            rowmin_transposed<NV>(dq + 16 * i, lane);
            keep[i] = dq[16 * i];
            // (L >= 32: rows 1 and 3 take the minimum with the row before them -- lanes 0-31 and 32-63)
            if constexpr (L != 16) keep[i] = fminf(keep[i], __shfl_up(keep[i], 16));
        });
        if (valid && (L == 16 || (lane & 16))) {
#pragma unroll
            for (int i = 0; i < (NB + 15) / 16; ++i) {
                const int kb = 16 * i + (lane & 15);
                if (kb < NB) dlin[L == 64 ? 2 * kb + (lane >> 5) : kb] = keep[i];
            }
        }
    }
}

// Persistent form: one workgroup per CU (12 waves, three per SIMD: with the 144-146 registers of the Hermitian fold a
// third wave fits, 8 -> 12 waves took 1.4 us off 25.8 at 512^2 and 2.8 off 34.4 at 1280^2 x 20 rows; a fourth needs
// 128 registers, which hipcc only reaches with 28-84 bytes of scratch), the C = (N/2+1) ntd lines in y-major order cut into equal
// contiguous shares; the waves of a workgroup take the lines of its share in turn (wave w: lines
// c0 + w, c0 + w + NW, ...), so every wave of the launch does the same number of lines +- 1 and the
// set-up (twiddles, first coefficients) is paid once.  At any time the waves of a workgroup are within
// NW lines of each other, i.e. in at most two consecutive y: the coefficients of y_lo and y_lo + 1 sit
// in two LDS slots, and when wave 0 moves on to a new y_lo the workgroup meets at a barrier and loads
// the next line's into the slot that fell free (a share is 1 - 3 lines y long: a handful of barriers
// per launch).  [first form: one workgroup per (y, group of tasks) -- 2056 workgroups at 512^2, whose
// set-up and +-1 task imbalance cost 20 of its 50 us]
#ifndef MPSFR_SERIES_THREADS
#define MPSFR_SERIES_THREADS 768
#endif
template <int N, typename RO>
constexpr int series_threads() { return N <= 128 ? 256 : MPSFR_SERIES_THREADS; }
template <int N, typename RO>
constexpr size_t series_smem() {
    return 2 * (size_t)N * SeriesCfg<RO>::K * sizeof(RO) + (size_t)N * sizeof(cx<double>);
}
template <int N, typename RO>
constexpr bool series_fits() { return series_smem<N, RO>() <= 160 * 1024; }

// A "unit" is what a wave takes at a time: the R = 64 / L lines (y; td = R q + rho, rho < R) of one y
// and R consecutive tasks; units in y-major order, c = y nq + q with nq = ceil(ntd / R).
template <int N, typename RO>
__global__ void __launch_bounds__((series_threads<N, RO>()), (512 / series_threads<N, RO>() > 1 ? 2 : 1))
k_dphi_series(const cx<double>* __restrict__ T, const double* __restrict__ sp,
              const TaskPar* __restrict__ tp, int ndir, int ntd, const RO* __restrict__ coef,
              const cx<double>* __restrict__ twk, double scale2, RO* __restrict__ D0t,
              float* __restrict__ dlin, int* __restrict__ zero17, const unsigned* __restrict__ support) {
    constexpr int L = series_lanes<N>(), R = 64 / L, Q = N / L, H1 = N / 2 + 1, K = SeriesCfg<RO>::K;
    constexpr int THREADS = series_threads<N, RO>(), NW = THREADS / 64, NJ = fold_nj<Q>();
    constexpr bool WJREG = NJ <= 10;         // the twiddles W_L^(j k2) of a lane in registers
    constexpr int LINE = N * K;              // coefficients of a line
    extern __shared__ __align__(16) unsigned char smem[];
    RO* scoef = reinterpret_cast<RO*>(smem);                                       // [2][N][K]
    cx<double>* swr = reinterpret_cast<cx<double>*>(smem + 2 * (size_t)LINE * sizeof(RO));   // [Q][L]
    const int lane = threadIdx.x & 63, rho = lane / L, k2 = lane & (L - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nq = (ntd + R - 1) / R;
    const long C = (long)H1 * nq;
    const int c0 = (int)(C * blockIdx.x / gridDim.x), c1 = (int)(C * (blockIdx.x + 1) / gridDim.x);
    if (zero17 != nullptr && blockIdx.x == 0 && threadIdx.x < kMfSchedInts) zero17[threadIdx.x] = 0;
    if (c0 >= c1) return;
    // (two register sets: the inputs of a unit are requested a whole unit ahead)
    cx<double> xva[kNXH], xvb[kNXH];
    auto fetch = [&](int c, cx<double>* xv) {
        const int y = c / nq, td = min(R * (c - y * nq) + rho, ntd - 1);
        const cx<double>* src = T + ((size_t)td * H1 + y) * kNH;
#pragma unroll
        for (int a = 0; a < kNXH; ++a) xv[a] = src[min(16 * a + (lane & 15), kNH - 1)];
    };
    const int nwe = min(NW, nq);
    const bool active = wave < nwe;
    if (active && c0 + wave < c1) fetch(c0 + wave, xva);
    using V4 = typename std::conditional<sizeof(RO) == 4, float4, double2>::type;
    constexpr int NV = (int)((size_t)LINE * sizeof(RO) / 16);
    auto load_line = [&](int y) {          // (all threads) coefficients of line y -> slot y & 1
        if (y > N / 2) return;
        const V4* src = reinterpret_cast<const V4*>(coef + (size_t)y * LINE);
        V4* dst = reinterpret_cast<V4*>(scoef + (size_t)(y & 1) * LINE);
        for (int i = threadIdx.x; i < NV; i += THREADS) dst[i] = src[i];
    };
    int ylo = c0 / nq;
    load_line(ylo);
    load_line(ylo + 1);
    for (int i = threadIdx.x; i < Q * L; i += THREADS) swr[i] = twk[NJ * L + i];
    cx<double> wjr[WJREG ? NJ : 1];
    if constexpr (WJREG) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) wjr[j] = twk[j * L + k2];
    }
    __syncthreads();
    auto unit = [&](int c, const cx<double>* xv) {
        const int y = c / nq, tdr = R * (c - y * nq) + rho;
        const bool valid = tdr < ntd;
        const int td = valid ? tdr : ntd - 1;
        const int task = td / ndir;
        const double r0m53 = tp[task].r0m53, delta = tp[task].inv_l0sq - kEps0;
        const double spv = sp[td];
        cx<double> wl[WJREG ? 1 : NJ];
        if constexpr (!WJREG) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) wl[j] = twk[j * L + k2];
        }
        const unsigned kmask = support != nullptr ? (unsigned)__builtin_amdgcn_readfirstlane((int)support[y]) : 0xffffffffu;
        series_line<N, RO, L>(xv, WJREG ? wjr : wl, swr, scoef + (size_t)(y & 1) * LINE, r0m53, delta, spv, scale2,
                              D0t + ((size_t)td * H1 + y) * N + k2,
                              dlin != nullptr ? dlin + ((size_t)td * H1 + y) * (N / 32) : nullptr, valid, lane, kmask);
    };
    // every wave runs the same number of rounds (the barriers below are met by all of them); a round
    // is one unit per active wave: c = cb + wave.  (With fewer units per y than waves a round would
    // span more than two y: only nq waves work then.)
    auto new_y = [&](int cb) {
        const int yb = cb / nq;                  // the y of wave 0's unit: uniform over the workgroup
        if (yb != ylo) {                         // (yb = ylo + 1: a round is at most nq units long)
            __syncthreads();                     // nobody reads line ylo any more
            for (int yy = ylo + 2; yy <= yb + 1; ++yy) load_line(yy);
            ylo = yb;
            __syncthreads();
        }
    };
    for (int cb = c0; cb < c1; cb += 2 * nwe) {
        new_y(cb);
        {
            const int c = cb + wave;
            if (active && c + nwe < c1) fetch(c + nwe, xvb);
            if (active && c < c1) unit(c, xva);
        }
        if (cb + nwe < c1) {
            new_y(cb + nwe);
            const int c = cb + nwe + wave;
            if (active && c + nwe < c1) fetch(c + nwe, xva);
            if (active && c < c1) unit(c, xvb);
        }
    }
}

// The first form, kept for what does not fit two coefficient slots in LDS (f64 mode at 1280^2):
// workgroup = (line y, group of tasks), the coefficients of the line in LDS once, every wave then walks
// its tasks alone.
template <int N, typename RO>
constexpr size_t series1_smem() {
    return (size_t)N * SeriesCfg<RO>::K * sizeof(RO) + (size_t)(N / 64) * 64 * sizeof(cx<double>);
}

template <int N, typename RO>
__global__ void __launch_bounds__(256)
k_dphi_series1(const cx<double>* __restrict__ T, const double* __restrict__ sp,
               const TaskPar* __restrict__ tp, int ndir, int ntd, int tg, const RO* __restrict__ coef,
               const cx<double>* __restrict__ twk, double scale2, RO* __restrict__ D0t,
               float* __restrict__ dlin, int* __restrict__ zero17, const unsigned* __restrict__ support) {
    constexpr int Q = N / 64, H1 = N / 2 + 1, K = SeriesCfg<RO>::K, THREADS = 256;
    constexpr int NJ = fold_nj<Q>(), JMIN = fold_jmin<Q>();
    constexpr bool WJREG = NJ <= 10;
    extern __shared__ __align__(16) unsigned char smem[];
    RO* scoef = reinterpret_cast<RO*>(smem);                                   // [N][K]
    cx<double>* swr = reinterpret_cast<cx<double>*>(smem + (size_t)N * K * sizeof(RO));   // [Q][64]
    const int y = blockIdx.x, g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int td_end = min(ntd, (g + 1) * tg);
    int td = g * tg + wave;
    cx<double> xva[kNXH], xvb[kNXH];
    auto fetch = [&](int t, cx<double>* xv) {
        const cx<double>* src = T + ((size_t)t * H1 + y) * kNH;
#pragma unroll
        for (int a = 0; a < kNXH; ++a) xv[a] = src[min(16 * a + (lane & 15), kNH - 1)];
    };
    if (td < td_end) fetch(td, xva);
    {
        using V4 = typename std::conditional<sizeof(RO) == 4, float4, double2>::type;
        constexpr int NV = (int)((size_t)N * K * sizeof(RO) / 16);
        const V4* src = reinterpret_cast<const V4*>(coef + (size_t)y * N * K);
        V4* dst = reinterpret_cast<V4*>(scoef);
        for (int i = threadIdx.x; i < NV; i += THREADS) dst[i] = src[i];
        for (int i = threadIdx.x; i < Q * 64; i += THREADS) swr[i] = twk[NJ * 64 + i];
    }
    if (zero17 != nullptr && y == 0 && g == 0 && threadIdx.x < kMfSchedInts) zero17[threadIdx.x] = 0;
    cx<double> wjr[WJREG ? NJ : 1];
    if constexpr (WJREG) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) wjr[j] = twk[j * 64 + lane];
    }
    __syncthreads();
    const unsigned kmask = support != nullptr ? (unsigned)__builtin_amdgcn_readfirstlane((int)support[y]) : 0xffffffffu;
    auto line = [&](int td, const cx<double>* xv) {
        const int task = td / ndir;
        const double r0m53 = tp[task].r0m53, delta = tp[task].inv_l0sq - kEps0;
        const double spv = sp[td];
        cx<double> wl[WJREG ? 1 : NJ];
        if constexpr (!WJREG) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) wl[j] = twk[j * 64 + lane];
        }
        series_line<N, RO, 64>(xv, WJREG ? wjr : wl, swr, scoef, r0m53, delta, spv, scale2,
                               D0t + ((size_t)td * H1 + y) * N + lane,
                               dlin != nullptr ? dlin + ((size_t)td * H1 + y) * (N / 32) : nullptr, true, lane, kmask);
    };
    constexpr int STEP = THREADS / 64;
    while (td < td_end) {
        if (td + STEP < td_end) fetch(td + STEP, xvb);
        line(td, xva);
        td += STEP;
        if (td >= td_end) break;
        if (td + STEP < td_end) fetch(td + STEP, xva);
        line(td, xvb);
        td += STEP;
    }
}

// K_SERIES_SUPPORT: support[y] bit k1 = some column x in [L k1, L k1 + L) of line y has a non-zero telescope OTF
// (L = series_lanes<N>(): the pieces a lane of K_DPHI_SERIES owns).  Once per context.
template <int N, typename RT>
__global__ void __launch_bounds__(64) k_series_support(const RT* __restrict__ tel, unsigned* __restrict__ support) {
    constexpr int L = series_lanes<N>(), Q = N / L;
    const int y = blockIdx.x, lane = threadIdx.x;
    unsigned m = 0;
    for (int k1 = 0; k1 < Q; ++k1) {
        bool any = false;
        for (int x = L * k1 + lane; x < L * k1 + L; x += 64) any = any || tel[(size_t)y * N + x] > (RT)0;
        if (__ballot(any) != 0ull) m |= 1u << k1;
    }
    if (lane == 0) support[y] = m;
}

// Hd planes [K][H1][N] (fp64, the output of K_COLFFT_DPHI for the basis tasks) -> coef[y][x][K]
template <typename RO>
__global__ void __launch_bounds__(256) k_series_coef(int n, int K, const double* __restrict__ planes,
                                                     RO* __restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < K; ++k) coef[(size_t)i * K + k] = (RO)planes[(size_t)k * n + i];
}

// K_DMIN16: dlin[td][y][kb] (the per-line block minima of K_DPHI_SERIES) -> dblk[td][y / 16][kb], the
// minima over the blocks of 16 lines x 32 columns, and dline[td][y], the minima per line (what K_DMIN
// computes from D itself).
__global__ void __launch_bounds__(128) k_dmin16(int H1, int nks, const float* __restrict__ dlin,
                                                float* __restrict__ dline, float* __restrict__ dblk) {
    const int mt = blockIdx.x, td = blockIdx.y, nmt = gridDim.x;
    const int nline = min(16, H1 - 16 * mt);
    const float* src = dlin + ((size_t)td * H1 + 16 * mt) * nks;
    if ((int)threadIdx.x < nks) {
        float m = __builtin_inff();
        for (int i = 0; i < nline; ++i) m = fminf(m, src[i * nks + threadIdx.x]);
        dblk[((size_t)td * nmt + mt) * nks + threadIdx.x] = m;
    } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + nline) {
        const int i = threadIdx.x - 64;
        float m = __builtin_inff();
        for (int kb = 0; kb < nks; ++kb) m = fminf(m, src[i * nks + kb]);
        dline[(size_t)td * H1 + 16 * mt + i] = m;
    }
}

}  // namespace

void launch_dmin16(hipStream_t s, int N, int ntd, const float* d_dlin, float* d_dline, float* d_dblk) {
    const int H1 = N / 2 + 1;
    hipLaunchKernelGGL(k_dmin16, dim3((H1 + 15) / 16, ntd), dim3(128), 0, s, H1, N / 32, d_dlin, d_dline, d_dblk);
}

// the twiddle buffer: the table for 64 lanes per line (K_PATCH_ROWS, K_DPHI_SERIES1), then the one for
// series_lanes<N>() lanes per line (K_DPHI_SERIES)
size_t series_twiddle_bytes(int N) {
    size_t n = 0;
    DISPATCH_N(N, { n = (twiddle_entries<NN, 64>() + twiddle_entries<NN, series_lanes<NN>()>()) * sizeof(cx<double>); })
    return n;
}

void launch_series_twiddles(hipStream_t s, int N, const void* d_tw64, void* d_twk) {
    DISPATCH_N(N, {
        constexpr int L = series_lanes<NN>();
        hipLaunchKernelGGL((k_series_twiddles<NN, 64>), dim3(fold_nj<NN / 64>() + NN / 64), dim3(64), 0, s,
                           (const cx<double>*)d_tw64, (cx<double>*)d_twk);
        hipLaunchKernelGGL((k_series_twiddles<NN, L>), dim3(fold_nj<NN / L>() + NN / L), dim3(64), 0, s,
                           (const cx<double>*)d_tw64, (cx<double>*)d_twk + twiddle_entries<NN, 64>());
    })
}

int series_terms(bool f64) { return f64 ? SeriesCfg<double>::K : SeriesCfg<float>::K; }
double series_eps0() { return kEps0; }

void launch_series_support(hipStream_t s, int N, const void* d_tel, bool f64, unsigned* d_support) {
    DISPATCH_N(N, {
        if (f64)
            hipLaunchKernelGGL((k_series_support<NN, double>), dim3(NN / 2 + 1), dim3(64), 0, s, (const double*)d_tel, d_support);
        else
            hipLaunchKernelGGL((k_series_support<NN, float>), dim3(NN / 2 + 1), dim3(64), 0, s, (const float*)d_tel, d_support);
    })
}

void launch_series_coef(hipStream_t s, int N, const double* d_planes, void* d_coef, bool f64) {
    const int n = (N / 2 + 1) * N;
    if (f64)
        hipLaunchKernelGGL(k_series_coef<double>, dim3((n + 255) / 256), dim3(256), 0, s, n,
                           SeriesCfg<double>::K, d_planes, (double*)d_coef);
    else
        hipLaunchKernelGGL(k_series_coef<float>, dim3((n + 255) / 256), dim3(256), 0, s, n,
                           SeriesCfg<float>::K, d_planes, (float*)d_coef);
}

void launch_patch(hipStream_t s, int N, int ntd, int ndir, const TaskPar* d_tp, const double* d_aotab,
                  double cfit, const void* d_twk, double* d_P, void* d_T, double* d_sp, bool f64,
                  const PatchKhat& kh, const LayerMix& mix) {
    const dim3 ggrid((NAO * NAO + 255) / 256, ntd / ndir);
    if (mix.w != nullptr) {
        if (f64)
            hipLaunchKernelGGL((k_patch_gen<true, const double*, int>), ggrid, dim3(256), 0, s, ndir, d_tp, d_aotab, cfit, d_P,
                               mix.w, mix.ntab);
        else
            hipLaunchKernelGGL((k_patch_gen<false, const double*, int>), ggrid, dim3(256), 0, s, ndir, d_tp, d_aotab, cfit, d_P,
                               mix.w, mix.ntab);
    } else if (f64)
        hipLaunchKernelGGL(k_patch_gen<true>, ggrid, dim3(256), 0, s, ndir, d_tp, d_aotab, cfit, d_P);
    else
        hipLaunchKernelGGL(k_patch_gen<false>, ggrid, dim3(256), 0, s, ndir, d_tp, d_aotab, cfit, d_P);
    DISPATCH_N(N, {
        constexpr int NG = NAO * series_lanes<NN>() / 256;       // passes (of 4 x 64 / L rows) per td
        // passes per workgroup: around 512 workgroups in all (1024: +2 us at 512^2, +4 at 1280^2; 256: +2)
        int nb = (512 + ntd - 1) / ntd;
        if (nb > NG) nb = NG;
        if (nb < 1) nb = 1;
        const int qb = (NG + nb - 1) / nb;
        nb = (NG + qb - 1) / qb;
        const int ky = kh.n > 0 ? (kh.n + nb - 1) / nb : 0;       // rows of workgroups for the kernel spectra
        if (kh.n <= 0) {
            constexpr size_t sm = patch_rows_smem_all<NN, void>();
            allow_smem((k_patch_rows<NN, void>), sm);
            hipLaunchKernelGGL((k_patch_rows<NN, void>), dim3(nb, ntd), dim3(256), sm, s, (const double*)d_P,
                               (const cx<double>*)d_twk + twiddle_entries<NN, 64>(), (cx<double>*)d_T, d_sp, qb, ntd, kh);
        } else if (kh.f64) {
            constexpr size_t sm = patch_rows_smem_all<NN, double>();
            allow_smem((k_patch_rows<NN, double>), sm);
            hipLaunchKernelGGL((k_patch_rows<NN, double>), dim3(nb, ntd + ky), dim3(256), sm, s, (const double*)d_P,
                               (const cx<double>*)d_twk + twiddle_entries<NN, 64>(), (cx<double>*)d_T, d_sp, qb, ntd, kh);
        } else {
            constexpr size_t sm = patch_rows_smem_all<NN, float>();
            allow_smem((k_patch_rows<NN, float>), sm);
            hipLaunchKernelGGL((k_patch_rows<NN, float>), dim3(nb, ntd + ky), dim3(256), sm, s, (const double*)d_P,
                               (const cx<double>*)d_twk + twiddle_entries<NN, 64>(), (cx<double>*)d_T, d_sp, qb, ntd, kh);
        }
    })
}

void launch_dphi_series(hipStream_t s, int N, int ntd, int ndir, const TaskPar* d_tp, const void* d_T,
                        const double* d_sp, const void* d_coef, const void* d_twk, double scale2,
                        void* d_D0t, float* d_dlin, bool f64out, int* d_zero, int ncu, const unsigned* d_support) {
    const int H1 = N / 2 + 1;
    auto first_form = [&](auto kernel, size_t sm) {
        // task groups: enough workgroups to fill the GPU several times over, every workgroup's table load
        // shared by as many tasks as that allows, every wave of a workgroup the same number of lines
        const int waves = 4;
        int ngr = (2048 + H1 - 1) / H1;
        if (ngr * waves > ntd) ngr = (ntd + waves - 1) / waves;
        if (ngr < 1) ngr = 1;
        int tg = (ntd + ngr - 1) / ngr;
        tg = (tg + waves - 1) / waves * waves;
        ngr = (ntd + tg - 1) / tg;
        return std::make_pair(dim3(H1, ngr), tg);
    };
    DISPATCH_N(N, {
        if (f64out) {
            if constexpr (series_fits<NN, double>()) {
                constexpr size_t sm = series_smem<NN, double>();
                allow_smem((k_dphi_series<NN, double>), sm);
                hipLaunchKernelGGL((k_dphi_series<NN, double>), dim3(ncu), dim3(series_threads<NN, double>()), sm, s,
                                   (const cx<double>*)d_T, d_sp, d_tp, ndir, ntd, (const double*)d_coef,
                                   (const cx<double>*)d_twk + twiddle_entries<NN, 64>(), scale2, (double*)d_D0t, d_dlin, d_zero, d_support);
            } else {
                constexpr size_t sm = series1_smem<NN, double>();
                allow_smem((k_dphi_series1<NN, double>), sm);
                const auto gt = first_form(0, sm);
                hipLaunchKernelGGL((k_dphi_series1<NN, double>), gt.first, dim3(256), sm, s,
                                   (const cx<double>*)d_T, d_sp, d_tp, ndir, ntd, gt.second, (const double*)d_coef,
                                   (const cx<double>*)d_twk, scale2, (double*)d_D0t, d_dlin, d_zero, d_support);
            }
        } else {
            constexpr size_t sm = series_smem<NN, float>();
            allow_smem((k_dphi_series<NN, float>), sm);
            hipLaunchKernelGGL((k_dphi_series<NN, float>), dim3(ncu), dim3(series_threads<NN, float>()), sm, s,
                               (const cx<double>*)d_T, d_sp, d_tp, ndir, ntd, (const float*)d_coef,
                               (const cx<double>*)d_twk + twiddle_entries<NN, 64>(), scale2, (float*)d_D0t, d_dlin, d_zero, d_support);
        }
    })
}

}  // namespace mpsfr
