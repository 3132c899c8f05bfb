// implicit_foldin.hip — the exact user step on implicit feedback in one launch on gfx950 (include/mfcd.h:
// mfcd_implicit_fold_in_users).  Row r has observed columns (pos list) and barred columns (excl list), both strictly
// ascending; P = observed \ barred, N = [0, m) \ (observed u barred).  With V [m][d] fixed its vector u minimises
//     f(u) = coef_r * sum over i in P, j in N of softplus(a_j - a_i) + (l2 / 2) |u|^2,   a_c = u . v~_c,
// mfcd/implicit_exact.py's _UserProblem, which implicit_user_step solves for all rows in lockstep through
// population._newton, a chain of small launches per iteration.  Here one workgroup of 256 threads owns one row and runs
// that iteration (solver "direct": the d x d Hessian and a Cholesky factor in LDS) from start to finish;
// tests/implicit_foldin_model.py restates it in numpy.
//
// The fixed iteration, mfcd_ratings_fold_in_users':
//   1. u = U_init[r] or 0, t = 1, iterations = 0.
//   2. g = grad f(u).  |g|_2 <= gtol l2 |u|_inf: status 0.  Otherwise iterations == max_newton: status 1.
//   3. If u moved since the direction was formed, or there is none yet: H = coef H_risk + l2 I, p = -H^{-1} g by
//      Cholesky (foldin_common.h: fold_cholesky_solve); a pivot that is not positive: p = -g / mean(diag H).
//   4. f_t = f(u + t p), iterations += 1.  f_t <= f + 1e-4 t (g . p) (a NaN f_t fails): u += t p, t = min(2 t, 1).
//      Otherwise t /= 2, the direction is kept, and t < 2^-12 ends the row with status 1.  Back to 2.
//      The inequality is taken on the two values of f first; only when that fails the decrease f(u + t p) - f(u) is
//      summed pair by pair (softplus(a + h) - softplus(a) = log1p(sigmoid(a) expm1(h)) for |h| < 1) and tested too
//      (fold_armijo_accepts: either evaluation accepts).  It decides where the fp32 part of f, coef times the risk,
//      outweighs the f64 ridge part: f's rounding then exceeds the decrease of the last steps.  Measured with this file
//      compiled under -DMFCD_IF_VALUES_ONLY (tests/test_implicit_foldin.py: VALUES_ONLY_STOPPED): at coef = 1e-7,
//      l2 = 1e-5 and at coef = 1, l2 = 3e-2 the values alone leave rows at the iteration cap that are certified here; at
//      the tests' l2 = 3e-2 under a table's coef (ridge-dominated f) the values alone decide the same.
//
// v~_c is V[c] minus the f64 mean of the rows of V that P names, rounded to fp32 once: everything depends on
// differences of the v_c only.  It is never stored, and neither are the scores: a_c is re-formed from V in every pass
// (an f64 chain over d rounded to fp32 once), m d multiply-adds against |P| |N| pairs, so there is no workspace and
// no split between resident and streamed rows.  What stays in LDS for the whole row is, per admissible positive, its
// column, its score and one f64 sum: 16 bytes.
//
// Threads own columns; the positives are broadcast reads from LDS.  With w_ij = sigmoid'(a_i - a_j),
// g_j = sum_i sigmoid(a_j - a_i), G_i = sum_j sigmoid(a_j - a_i), D_j = sum_i w_ij, D_i = sum_j w_ij, y_j = sum_i w_ij v~_i:
//     grad   = coef (sum_j g_j v~_j - sum_i G_i v~_i) + l2 u
//     H_risk = (T + T^T) / 2,   T = sum_i v~_i (D_i v~_i)^T + sum_j v~_j (D_j v~_j - 2 y_j)^T
// (the bipartite Laplacian's cross terms sum_ij w_ij (v~_i v~_j^T + v~_j v~_i^T) equal sum_j (y_j v~_j^T + v~_j y_j^T)),
// so only the scalars G_i and D_i cross threads: once per (positive, column stage), an xor butterfly inside a wave in
// f64, then the waves in index order.  The passes, in stages of kImpChunk columns classified from the two sorted lists
// (implicit_common.h: implicit_mark):
//   value and gradient   a thread owns 8 columns of a stage; per positive it adds softplus and sigmoid over them (fp32,
//                        8 terms, widened to f64), g_j in fp32 runs of 64 positives.  A column that is no negative
//                        carries score -inf: its terms are exactly 0 without a class branch.  The two d-vector sums
//                        of the gradient are column sums in f64: thread (k, slice) adds its slice, the slices are
//                        added in order.
//   decrease             the same loop with the pair's decrease term alone; taken only after a failed test on f.
//   Hessian              first D_i, a scalar pass as above.  Then y_j at DK multiply-adds per pair on the fp32 vector
//                        pipe: a thread owns one column at a time, the positives' v~_i go through LDS in slabs of 64,
//                        z_j = D_j v~_j - 2 y_j is rounded to fp32 once, and T is added in f64 from LDS slabs of 64
//                        columns, thread (bi, bj) owning a 4 x 4 block (ratings_fold_in_kernel's scheme; T is not
//                        symmetric, so all blocks are formed).  (T + T^T) / 2 is bit-symmetric.
// No atomics, no allocation, no host wait, no scratch; every sum has one owner and a fixed order that depends on the
// row alone; every loop is bounded by max_newton, the list lengths, m and d.
//
// Caps.  kIfMaxPos = 4608: 16 bytes of LDS per positive beside the 73 KiB the d = 64 form needs otherwise, 145 KiB of
// the compute unit's 160.  kIfMaxPairs = 11 x 2^20: one workgroup takes a whole row, and a row at the cap should stay
// under a second at max_newton = 20.  Measured on one MI355X (profiles/implicit_fold_in.txt, one row of 1024 observed
// items among 8192, d = 64, a call with max_newton = 0, launch and host time included): a value-and-gradient pass runs at
// 2.28 G pairs/s on its compute unit and a Hessian pass at 0.270 G pairs/s, 4.15 ns per pair for an iteration of one
// pass each; 11 534 336 pairs x 20 x 4.15 ns = 0.96 s (2^24 pairs would take 1.39 s).  The cap started at 2^23, from
// the ratings kernel's 4.9 ns.  It is not a tuning knob.  The cap bounds the pair work only: every pass also re-forms
// m scores of width d and reads the row's columns of V (about five times per iteration), which no cap bounds, so
// a short row in a very large catalogue is not held under a second by it (measured: 10 observed items of 65 536 at
// d = 64, 129 ms for 256 rows side by side, nearly all of it scoring; m = 4 194 304 would be 64 times that per row).
#include <cmath>
#include <type_traits>

#include "foldin_common.h"
#include "implicit_common.h"
#include "pairs_common.h"

namespace {

constexpr int kIfMaxD = 64;
constexpr int kIfMaxPos = 4608;
constexpr int64_t kIfMaxPairs = (int64_t)11 << 20;      // see above: from the measured pass rates at d = 64
constexpr int kIfThreads = kImpThreads;                // implicit_mark strides by it
constexpr int kIfChunk = kImpChunk;                    // columns per stage
constexpr int kIfOwn = kIfChunk / kIfThreads;          // columns a thread owns in a scalar pass
constexpr int kIfTile = 256;                           // positives per hand-over of the cross-thread sums
constexpr int kIfSlab = 64;                            // rows per LDS slab = terms per fp32 run
constexpr int kIfWaves = kIfThreads / MFCD_WAVE;
constexpr double kIfMinStep = 1.0 / 4096.0;            // population.MIN_STEP
static_assert(kIfThreads == 256 && kIfOwn == 8 && kIfMaxPos % kIfTile == 0, "the passes' geometry");

struct IfArgs {
    const float *V;
    int m, d;
    const int64_t *pos_off;
    const int32_t *pos_items;
    int64_t entries;
    const int64_t *excl_off;
    const int32_t *excl_items;
    int64_t excl_entries;
    int r0;
    const double *coef;
    double l2;
    const float *U_init;
    int max_newton;
    double gtol;
    float *U_out;
    double *objective, *grad_ratio;
    int32_t *iters_status;
    double *info;
};

// The scalar passes' stage of g_j (fp32 [kIfChunk]) and hand-over of the waves' sums (f64 [kIfWaves][kIfTile]) share
// the bytes of the Hessian pass's two slabs.
constexpr size_t if_slab_bytes(int DK)
{
    const size_t slabs = sizeof(float) * ((size_t)kIfSlab * DK + (size_t)kIfSlab * (DK + 1));
    const size_t scalar = sizeof(double) * kIfWaves * kIfTile + sizeof(float) * kIfChunk;
    return ((slabs > scalar ? slabs : scalar) + 15) & ~(size_t)15;
}

// bytes of LDS a workgroup of the DK form takes
constexpr size_t if_lds_bytes(int DK)
{
    return sizeof(double) * ((size_t)DK * (DK + 1) + 8 * (size_t)DK + kIfThreads + 32 + kIfMaxPos) + if_slab_bytes(DK) +
           sizeof(float) * (size_t)kIfMaxPos + sizeof(int32_t) * ((size_t)kIfMaxPos + 8) + kIfChunk;
}
static_assert(if_lds_bytes(64) <= 160 * 1024, "the compute unit's LDS");

// softplus(v) = max(v, 0) + ln 2 * this: log2(1 + exp(-|v|)), from the exp pair_sigmoid(v) takes (pairs_common.h: the same
// expression, so a pair that needs both pays one v_exp_f32); ln 2 is applied once, in f64, where the parts are summed.
__device__ __forceinline__ float if_softplus_log2(float v)
{
    return __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(v)));
}

// softplus(da) - softplus(da - h) of one pair, da the score difference at the trial point and h the step's share of it
// (ratings_foldin.hip's term without a label part).  h = 0, or da = -inf, gives exactly 0.
__device__ __forceinline__ float if_decrease_term(float da, float h)
{
    const float d0 = da - h;
    if (fabsf(h) < 1.0f) return log1pf(pair_sigmoid(d0) * expm1f(h));
    const float s1 = fmaxf(da, 0.0f) + 0.6931471805599453f * if_softplus_log2(da);
    const float s0 = fmaxf(d0, 0.0f) + 0.6931471805599453f * if_softplus_log2(d0);
    return s1 - s0;
}

// Statuses 2 and 3, and the closed form of a row without a pair (status 0).
__device__ __forceinline__ void if_constant_row(const IfArgs &g, int r, int tid, bool nan, int status, double f_start)
{
    const int d = g.d;
    const float rowv = nan ? __uint_as_float(0x7fc00000u) : 0.0f;
    const double dv = nan ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    for (int k = tid; k < d; k += kIfThreads) g.U_out[(int64_t)r * d + k] = rowv;
    if (g.info)
        for (int q = tid; q < d * d; q += kIfThreads) g.info[(int64_t)r * d * d + q] = dv;
    if (tid == 0) {
        if (g.objective) {
            g.objective[2 * (int64_t)r] = nan ? dv : f_start;
            g.objective[2 * (int64_t)r + 1] = dv;
        }
        if (g.grad_ratio) g.grad_ratio[r] = dv;
        g.iters_status[2 * (int64_t)r] = 0;
        g.iters_status[2 * (int64_t)r + 1] = status;
    }
}

template <int DK>
__global__ __launch_bounds__(kIfThreads) void implicit_fold_in_kernel(const IfArgs g)
{
    constexpr int NT = kIfThreads, LD = DK + 1, ZLD = DK + 1, NB = DK / 4, GR = 16;
    using Value = std::integral_constant<int, 0>;
    using Decrease = std::integral_constant<int, 1>;
    using Degree = std::integral_constant<int, 2>;
    extern __shared__ double if_lds[];
    double *H = if_lds, *u = H + DK * LD, *gv = u + DK, *gt = gv + DK, *p = gt + DK, *ut = p + DK, *mean = ut + DK;
    double *sol = mean + DK, *diag = sol + DK, *part = diag + DK, *scal = part + NT, *Gacc = scal + 32;
    double *red = Gacc + kIfMaxPos;                    // the scalar passes' view of the slab bytes ...
    float *GS = (float *)(red + kIfWaves * kIfTile);
    float *S = (float *)red, *Zs = S + kIfSlab * DK;   // ... and the Hessian pass's
    float *PA = (float *)((char *)red + if_slab_bytes(DK));
    float *PH = (float *)Gacc;                         // the decrease pass's h_i: Gacc holds nothing then
    int32_t *PC = (int32_t *)(PA + kIfMaxPos), *wl = PC + kIfMaxPos;
    unsigned char *cls = (unsigned char *)(wl + 8);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = g.d, m = g.m;
    const int r = g.r0 + blockIdx.x;
    const float *__restrict__ V = g.V;

    // ---- validation: offsets and lengths, then every item of both lists, the coefficient, the start row ----
    const int64_t pb = g.pos_off[r], pe = g.pos_off[r + 1];
    const int64_t eb = g.excl_off ? g.excl_off[r] : 0, ee = g.excl_off ? g.excl_off[r + 1] : 0;
    if (!(pb >= 0 && pe >= pb && pe <= g.entries && eb >= 0 && ee >= eb && ee <= g.excl_entries) || pe - pb > m || ee - eb > m) {
        if_constant_row(g, r, tid, true, 2, 0.0);      // a strictly ascending list of [0, m) has at most m items
        return;
    }
    const int Lp = (int)(pe - pb), Le = (int)(ee - eb);
    // From the lengths alone: at least Lp - Le admissible positives and m - Lp - Le negatives.  Without a barred list
    // these are the counts themselves.
    if (Lp - Le > kIfMaxPos || (Lp - Le > 0 && m - Lp - Le > 0 && (int64_t)(Lp - Le) * (m - Lp - Le) > kIfMaxPairs)) {
        if_constant_row(g, r, tid, true, 3, 0.0);
        return;
    }
    const float *start = g.U_init ? g.U_init + (int64_t)r * d : nullptr;
    const double coef = g.coef ? g.coef[r] : 1.0;
    int bad = (int)!(coef > 0.0 && coef <= 1.7976931348623157e308);
    for (int q = tid; q < Lp; q += NT) {
        const int v = g.pos_items[pb + q];
        bad |= (int)((unsigned)v >= (unsigned)m);
        if (q > 0) bad |= (int)(g.pos_items[pb + q - 1] >= v);
    }
    for (int q = tid; q < Le; q += NT) {
        const int v = g.excl_items[eb + q];
        bad |= (int)((unsigned)v >= (unsigned)m);
        if (q > 0) bad |= (int)(g.excl_items[eb + q - 1] >= v);
    }
    if (start)
        for (int k = tid; k < d; k += NT) bad |= (int)is_nonfinite_bits(start[k]);
    if (__syncthreads_or(bad)) {
        if_constant_row(g, r, tid, true, 2, 0.0);
        return;
    }

    // ---- the admissible positives, in list order: PC[0, np) (the first kIfMaxPos of them) ----
    int np = 0;
    for (int q0 = 0; q0 < Lp; q0 += NT) {
        const int q = q0 + tid;
        const int c = q < Lp ? g.pos_items[pb + q] : 0;
        const bool keep = q < Lp && !is_barred(g.excl_items, eb, ee, c);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wl[wave] = __popcll(mask);
        __syncthreads();
        int slot = np + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) slot += wl[w];
        if (keep && slot < kIfMaxPos) PC[slot] = c;
        np += (wl[0] + wl[1]) + (wl[2] + wl[3]);
        __syncthreads();
    }
    const int nn = m - Le - np;                        // |observed u barred| = Lp + Le - (Lp - np)
    if (np > kIfMaxPos || (int64_t)np * nn > kIfMaxPairs) {
        if_constant_row(g, r, tid, true, 3, 0.0);
        return;
    }
    if (np == 0 || nn == 0) {                          // no pair: the risk is identically 0
        double uu = 0.0;
        if (start)
            for (int k = 0; k < d; ++k) uu = fma((double)start[k], (double)start[k], uu);
        if_constant_row(g, r, tid, false, 0, 0.5 * g.l2 * uu);
        return;
    }

    // ---- geometry ----
    int lg = 0;
    while ((1 << lg) < d) ++lg;
    const int P2 = 1 << lg, ck = tid & (P2 - 1), csl = tid >> lg, nsl = NT >> lg;   // column sums: (column, slice)
    const bool hthread = tid < NB * NB;                // the 4 x 4 block (bi, bj) of T this thread owns
    const int bi = tid / NB, bj = tid - bi * NB;

    // One centred entry of V~.
    auto centred = [&](int c, int k) -> float { return (float)((double)V[(int64_t)c * d + k] - mean[k]); };

    // u . v~_c and p . v~_c: f64 chains over k; flags a non-finite entry of the row.
    auto dots = [&](int c, const double *uv, double &a, double &h, int &flag) {
        const float *vr = V + (int64_t)c * d;
        a = h = 0.0;
        for (int k = 0; k < d; ++k) {
            const float v = vr[k];
            flag |= (int)is_nonfinite_bits(v);
            const double vt = (double)(float)((double)v - mean[k]);
            a = fma(uv[k], vt, a);
            h = fma(p[k], vt, h);
        }
    };

    // part[] over the slices of column k in order → the thread's total (tid < DK).  A barrier precedes the call.
    auto slices = [&]() -> double {
        double tsum = 0.0;
        if (tid < d)
            for (int w = 0; w < nsl; ++w) tsum += part[w * P2 + tid];   // fixed order
        return tsum;
    };

    // cls[j] = 1 for the columns of [c0, c0 + len) that either list names.  Ends with a barrier.
    auto classify = [&](int c0, int len) {
        for (int j = tid; j < kIfChunk; j += NT) cls[j] = 0;
        __syncthreads();
        implicit_mark(cls, c0, len, g.pos_items, pb, pe, 1, tid);
        implicit_mark(cls, c0, len, g.excl_items, eb, ee, 1, tid);
        __syncthreads();
    };

    // PA[i] = a_i at uv, and with WITH_H PH[i] = tt p . v~_i.  Ends with a barrier.
    auto pos_scores = [&](const double *uv, double tt, bool with_h) -> int {
        int flag = 0;
        for (int i = tid; i < np; i += NT) {
            double a, h;
            dots(PC[i], uv, a, h, flag);
            PA[i] = (float)a;
            if (with_h) PH[i] = (float)(tt * h);
        }
        __syncthreads();
        return flag;
    };

    // One pass over the row's pairs with 8 columns per thread and stage.  Value: f(uv) → scal[0], the gradient → gout,
    // → whether a V row of the user is non-finite.  Decrease: f(uv) - f(u) summed pair by pair → scal[5], uv = u + tt p.
    // Degree: Gacc[i] = D_i at uv.
    auto scalar_pass = [&](auto mode, const double *uv, double *gout, double tt) -> int {
        constexpr int MODE = decltype(mode)::value;
        int flag = 0;
        if (MODE != Decrease::value)
            for (int i = tid; i < np; i += NT) Gacc[i] = 0.0;
        flag |= pos_scores(uv, tt, MODE == Decrease::value);
        double fa = 0.0, fb = 0.0, gsum = 0.0;         // log2 parts and linear parts (or decreases); the slice's sum
        for (int c0 = 0; c0 < m; c0 += kIfChunk) {
            const int len = m - c0 < kIfChunk ? m - c0 : kIfChunk, nown = (len + NT - 1) / NT;
            classify(c0, len);
            float aj[kIfOwn], hj[kIfOwn], grun[kIfOwn];
            double gacc[kIfOwn];
            bool any = false;
#pragma unroll
            for (int c = 0; c < kIfOwn; ++c) {
                const int j = tid + NT * c;
                aj[c] = -INFINITY;
                hj[c] = grun[c] = 0.0f;
                gacc[c] = 0.0;
                if (j < len && cls[j] == 0) {
                    double a, h;
                    dots(c0 + j, uv, a, h, flag);
                    aj[c] = (float)a;
                    hj[c] = (float)(tt * h);
                    any = true;
                }
            }
            const bool live = __ballot(any) != 0ull;   // the wave holds a negative of this stage
            for (int t0 = 0; t0 < np; t0 += kIfTile) {
                const int nt = np - t0 < kIfTile ? np - t0 : kIfTile;
                if (live) {
                    for (int i = 0; i < nt; ++i) {
                        const float ai = PA[t0 + i];
                        float s8 = 0.0f, x8 = 0.0f, y8 = 0.0f;     // at most kIfOwn terms each
                        if (MODE == Decrease::value) {
                            const float hi = PH[t0 + i];
#pragma unroll
                            for (int c = 0; c < kIfOwn; ++c)
                                if (c < nown) x8 += if_decrease_term(aj[c] - ai, hj[c] - hi);
                            fb += (double)x8;
                        } else if (MODE == Degree::value) {
#pragma unroll
                            for (int c = 0; c < kIfOwn; ++c)
                                if (c < nown) s8 += pair_curvature(aj[c] - ai);
                        } else {
#pragma unroll
                            for (int c = 0; c < kIfOwn; ++c)
                                if (c < nown) {
                                    const float da = aj[c] - ai;
                                    const float sg = pair_sigmoid(da);
                                    x8 += if_softplus_log2(da);
                                    y8 += fmaxf(da, 0.0f);
                                    s8 += sg;
                                    grun[c] += sg;
                                }
                            fa += (double)x8;
                            fb += (double)y8;
                            if ((i & 63) == 63 || i + 1 == nt) {   // a column's run: at most 64 positives
#pragma unroll
                                for (int c = 0; c < kIfOwn; ++c) {
                                    gacc[c] += (double)grun[c];
                                    grun[c] = 0.0f;
                                }
                            }
                        }
                        if (MODE != Decrease::value) {
                            const double s = wave_sum_xor((double)s8);
                            if (lane == 0) red[wave * kIfTile + i] = s;
                        }
                    }
                } else if (MODE != Decrease::value) {
                    for (int i = lane; i < nt; i += MFCD_WAVE) red[wave * kIfTile + i] = 0.0;
                }
                if (MODE != Decrease::value) {
                    __syncthreads();
                    if (tid < nt) {
                        double s = red[tid];
                        for (int w = 1; w < kIfWaves; ++w) s += red[w * kIfTile + tid];   // the waves in index order
                        Gacc[t0 + tid] += s;
                    }
                    __syncthreads();
                }
            }
            if (MODE == Value::value) {
#pragma unroll
                for (int c = 0; c < kIfOwn; ++c) GS[tid + NT * c] = (float)gacc[c];   // rounded to fp32 once; 0 for no negative
                __syncthreads();
                if (ck < d)
                    for (int e = csl; e < len; e += nsl)
                        if (cls[e] == 0) gsum = fma((double)GS[e], (double)centred(c0 + e, ck), gsum);
            }
            __syncthreads();                           // the stage's readers of cls and GS are done
        }
        if (MODE == Degree::value) return 0;
        if (MODE == Value::value) {
            if (ck < d)
                for (int i = csl; i < np; i += nsl) gsum = fma(-Gacc[i], (double)centred(PC[i], ck), gsum);
            part[tid] = gsum;
        }
        fa = wave_sum_xor(fa);
        fb = wave_sum_xor(fb);
        if (lane == 0) {
            scal[16 + 2 * wave] = fa;
            scal[17 + 2 * wave] = fb;
        }
        flag = __syncthreads_or(flag);
        if (MODE == Value::value && tid < DK) gout[tid] = tid < d ? fma(coef, slices(), g.l2 * uv[tid]) : 0.0;
        if (tid == 0) {
            double sa = 0.0, sb = 0.0, uu = 0.0, up = 0.0, pp = 0.0;
            for (int w = 0; w < kIfWaves; ++w) {
                sa += scal[16 + 2 * w];
                sb += scal[17 + 2 * w];
            }
            for (int k = 0; k < d; ++k) {
                uu = fma(uv[k], uv[k], uu);
                up = fma(u[k], p[k], up);
                pp = fma(p[k], p[k], pp);
            }
            if (MODE == Value::value) scal[0] = coef * (0.6931471805599453 * sa + sb) + 0.5 * g.l2 * uu;
            else scal[5] = coef * sb + g.l2 * (tt * up + 0.5 * tt * tt * pp);
        }
        __syncthreads();
        return flag;
    };

    // T += S^T Zs over the first tn rows of the two slabs.
    double hacc[4][4];
    auto gram = [&](int tn) {
        if (!hthread) return;
        for (int t = 0; t < tn; ++t) {
            const float *sr = S + t * DK + 4 * bi, *zr = Zs + t * ZLD + 4 * bj;
            double va[4], zc[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                va[a] = (double)sr[a];
                zc[a] = (double)zr[a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) hacc[a][c] = fma(va[a], zc[c], hacc[a][c]);
        }
    };

    // H_risk at u: coef times it plus the ridge into H (padding rows and columns carry an identity block), or the sum
    // itself into info[r].
    auto hessian = [&](bool to_info) {
        scalar_pass(Degree{}, u, nullptr, 0.0);        // PA and Gacc = D_i at u
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) hacc[a][c] = 0.0;
        int flag = 0;
        for (int c0 = 0; c0 < m; c0 += kIfChunk) {
            const int len = m - c0 < kIfChunk ? m - c0 : kIfChunk, nown = (len + NT - 1) / NT;
            classify(c0, len);
            for (int sub = 0; sub < nown; ++sub) {
                const int j = sub * NT + tid;
                const bool neg = j < len && cls[j] == 0;
                float aown = -INFINITY;
                if (neg) {
                    double a, h;
                    dots(c0 + j, u, a, h, flag);
                    aown = (float)a;
                }
                const bool live = __ballot(neg) != 0ull;
                if (lane == 0) wl[wave] = (int)live;
                double zacc[DK], dacc = 0.0;
#pragma unroll
                for (int k = 0; k < DK; ++k) zacc[k] = 0.0;
                for (int i0 = 0; i0 < np; i0 += kIfSlab) {
                    const int ln = np - i0 < kIfSlab ? np - i0 : kIfSlab;
                    __syncthreads();                   // the previous readers of S are done
                    for (int q = tid; q < kIfSlab * DK; q += NT) {
                        const int t = q / DK, k = q - t * DK;
                        S[q] = (t < ln && k < d) ? centred(PC[i0 + t], k) : 0.0f;
                    }
                    __syncthreads();
                    if (!live) continue;               // the wave only helps to stage
                    float acc[DK], dg = 0.0f;          // at most kIfSlab terms each
#pragma unroll
                    for (int k = 0; k < DK; ++k) acc[k] = 0.0f;
                    for (int t = 0; t < ln; ++t) {
                        const float w = pair_curvature(aown - PA[i0 + t]);
                        dg += w;
                        const float *sr = S + t * DK;
#pragma unroll
                        for (int k = 0; k < DK; ++k) acc[k] = fmaf(w, sr[k], acc[k]);
                    }
                    dacc += (double)dg;
#pragma unroll
                    for (int k = 0; k < DK; ++k) zacc[k] += (double)acc[k];
                }
                // T += V~^T Z over the negatives of this sub-stage, one wave's 64 columns at a time
                for (int w = 0; w < kIfWaves; ++w) {
                    const int e0 = sub * NT + kIfSlab * w;
                    if (e0 >= len) break;
                    if (!wl[w]) continue;              // written before the barriers of the positives' loop (np >= 1)
                    __syncthreads();                   // the previous readers of S and Zs are done
                    if (wave == w) {
#pragma unroll
                        for (int k = 0; k < DK; ++k) {
                            float z = 0.0f;
                            if (neg && k < d) z = (float)(dacc * (double)centred(c0 + j, k) - 2.0 * zacc[k]);   // rounded to fp32 once
                            Zs[lane * ZLD + k] = z;
                        }
                    }
                    for (int q = tid; q < kIfSlab * DK; q += NT) {
                        const int t = q / DK, k = q - t * DK;
                        S[q] = (e0 + t < len && cls[e0 + t] == 0 && k < d) ? centred(c0 + e0 + t, k) : 0.0f;
                    }
                    __syncthreads();
                    gram(len - e0 < kIfSlab ? len - e0 : kIfSlab);
                }
                __syncthreads();                       // the readers of wl are done
            }
            __syncthreads();                           // the stage's readers of cls are done
        }
        // T += sum_i v~_i (D_i v~_i)^T
        for (int i0 = 0; i0 < np; i0 += kIfSlab) {
            const int ln = np - i0 < kIfSlab ? np - i0 : kIfSlab;
            __syncthreads();
            for (int q = tid; q < kIfSlab * DK; q += NT) {
                const int t = q / DK, k = q - t * DK;
                const bool in = t < ln && k < d;
                const float v = in ? centred(PC[i0 + t], k) : 0.0f;
                S[q] = v;
                Zs[t * ZLD + k] = in ? (float)(Gacc[i0 + t] * (double)v) : 0.0f;
            }
            __syncthreads();
            gram(ln);
        }
        __syncthreads();
        if (hthread) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) H[(4 * bi + a) * LD + 4 * bj + c] = hacc[a][c];
        }
        __syncthreads();
        for (int q = tid; q < DK * DK; q += NT) {      // (T + T^T) / 2: the thread of (hi, hj), hi >= hj, owns both entries
            const int hi = q / DK, hj = q - hi * DK;
            if (hi < hj) continue;
            const double s = 0.5 * (H[hi * LD + hj] + H[hj * LD + hi]);
            if (to_info) {
                if (hi < d) {
                    double *out = g.info + (int64_t)r * d * d;
                    out[hi * d + hj] = s;
                    out[hj * d + hi] = s;
                }
            } else {
                const double h = hi < d ? fma(coef, s, hi == hj ? g.l2 : 0.0) : (hi == hj ? 1.0 : 0.0);
                H[hi * LD + hj] = h;
                H[hj * LD + hi] = h;
            }
        }
        __syncthreads();
    };

    // p = -H^{-1} gv by Cholesky; a pivot that is not positive: p = -gv / mean(diag H).
    auto direction = [&]() {
        if (tid == 0) {
            double tr = 0.0;
            for (int k = 0; k < d; ++k) tr += H[k * LD + k];
            scal[3] = tr / (double)d;
        }
        if (!fold_cholesky_solve<NT, GR>(H, LD, DK, diag, sol, gv, p, tid)) {
            __syncthreads();
            if (tid < DK) p[tid] = tid < d ? -gv[tid] / scal[3] : 0.0;
        }
        __syncthreads();
    };

    // ---- the row's centre (and the check of its positives' V rows), the start ----
    if (tid < DK) {
        u[tid] = (start && tid < d) ? (double)start[tid] : 0.0;
        mean[tid] = 0.0;
        p[tid] = 0.0;
    }
    {
        double s = 0.0;
        int badv = 0;
        if (ck < d)
            for (int i = csl; i < np; i += nsl) {
                const float v = V[(int64_t)PC[i] * d + ck];
                badv |= (int)is_nonfinite_bits(v);
                s += (double)v;
            }
        part[tid] = s;
        badv = __syncthreads_or(badv);
        if (badv) {
            if_constant_row(g, r, tid, true, 2, 0.0);
            return;
        }
        if (tid < DK) mean[tid] = tid < d ? slices() / (double)np : 0.0;
        __syncthreads();
    }

    if (scalar_pass(Value{}, u, gv, 0.0)) {            // a V row of a negative holds an inf or a NaN
        if_constant_row(g, r, tid, true, 2, 0.0);
        return;
    }
    double f = scal[0];
    const double f_start = f;
    int it = 0, status = 1;
    double t = 1.0;
    bool have = false, moved = true;
    for (;;) {                                         // gv and f belong to u
        if (tid == 0) {
            double gg = 0.0, um = 0.0;
            for (int k = 0; k < d; ++k) {
                gg = fma(gv[k], gv[k], gg);
                um = fmax(um, fabs(u[k]));
            }
            scal[1] = sqrt(gg);
            scal[2] = um;
        }
        __syncthreads();
        if (scal[1] <= g.gtol * (g.l2 * scal[2])) {
            status = 0;
            break;
        }
        if (it == g.max_newton) break;
        if (moved || !have) {
            hessian(false);
            direction();
            have = true;
        }
        if (tid < DK) ut[tid] = fma(t, p[tid], u[tid]);
        if (tid == 0) {
            double gp = 0.0;
            for (int k = 0; k < d; ++k) gp = fma(gv[k], p[k], gp);
            scal[4] = gp;
        }
        __syncthreads();
        const double gp = scal[4];
        scalar_pass(Value{}, ut, gt, t);
        const double ft = scal[0];
        ++it;
        // the Armijo rule on the two values of f, then on the decrease summed pair by pair; a NaN trial is a rejected one
        double dec = INFINITY;
#ifndef MFCD_IF_VALUES_ONLY                            // the diagnostic twin (make exp): the test on the values of f alone
        if (!(ft <= f + kFoldArmijo * t * gp)) {
            scalar_pass(Decrease{}, ut, nullptr, t);
            dec = scal[5];
        }
#endif
        if (fold_armijo_accepts(dec, ft, f, t, gp)) {
            if (tid < DK) {
                u[tid] = ut[tid];
                gv[tid] = gt[tid];
            }
            f = ft;
            t = fmin(2.0 * t, 1.0);
            moved = true;
        } else {
            t *= 0.5;
            moved = false;
            if (t < kIfMinStep) break;
        }
        __syncthreads();
    }
    __syncthreads();

    if (g.info) hessian(true);
    for (int k = tid; k < d; k += NT) g.U_out[(int64_t)r * d + k] = (float)u[k];
    if (tid == 0) {
        if (g.objective) {
            g.objective[2 * (int64_t)r] = f_start;
            g.objective[2 * (int64_t)r + 1] = f;
        }
        if (g.grad_ratio) g.grad_ratio[r] = scal[1] / (g.l2 * scal[2]);
        g.iters_status[2 * (int64_t)r] = it;
        g.iters_status[2 * (int64_t)r + 1] = status;
    }
}

template <int DK>
int if_launch(IfArgs g, int rows, hipStream_t st)
{
    constexpr size_t lds = if_lds_bytes(DK);
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)implicit_fold_in_kernel<DK>, lds, allowed));
    return pair_chunks(rows, (int)kPairMaxBlocks, [&](int r0, int nr) {
        g.r0 = r0;
        hipLaunchKernelGGL((implicit_fold_in_kernel<DK>), dim3((unsigned)nr), dim3(kIfThreads), lds, st, g);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" int mfcd_implicit_fold_in_max_d(void) { return kIfMaxD; }

extern "C" int mfcd_implicit_fold_in_max_pos(void) { return kIfMaxPos; }

extern "C" int64_t mfcd_implicit_fold_in_max_pairs(void) { return kIfMaxPairs; }

extern "C" int mfcd_implicit_fold_in_chunk(void) { return kIfChunk; }

extern "C" size_t mfcd_implicit_fold_in_workspace_bytes(int rows, int m, int d)
{
    if (rows < 0 || m < 1 || m > kTopkMaxM || d < 1 || d > kIfMaxD) return 0;
    return 256;                                        // nothing is staged in HBM: the scores are re-formed from V in every pass
}

extern "C" int mfcd_implicit_fold_in_users(const float *V, int m, int d, const int64_t *pos_off, const int32_t *pos_items,
                                           int64_t entries, const int64_t *excl_off, const int32_t *excl_items,
                                           int64_t excl_entries, int rows, const double *coef, double l2, const float *U_init,
                                           int max_newton, double gtol, float *U_out, double *objective, double *grad_ratio,
                                           int32_t *iters_status, double *info, void *workspace, size_t workspace_bytes,
                                           void *stream)
{
    if (!V || !pos_off || !U_out || !iters_status || m < 1 || m > kTopkMaxM || d < 1 || d > kIfMaxD || rows < 0 || entries < 0)
        return MFCD_EINVAL;
    if ((entries > 0 && !pos_items) || (excl_off == nullptr) != (excl_items == nullptr)) return MFCD_EINVAL;
    if (excl_off ? excl_entries < 0 : excl_entries != 0) return MFCD_EINVAL;
    if (!std::isfinite(l2) || !(l2 > 0.0) || !std::isfinite(gtol) || gtol < 0.0 || max_newton < 0 || max_newton > 1000)
        return MFCD_EINVAL;
    const size_t row_bytes = (size_t)rows * d * sizeof(float), info_bytes = (size_t)rows * d * d * sizeof(double);
    const size_t off_bytes = ((size_t)rows + 1) * sizeof(int64_t);
    const struct {
        const void *p;
        size_t n;
    } inputs[] = {{V, (size_t)m * d * sizeof(float)},
                  {pos_off, off_bytes},
                  {pos_items, (size_t)entries * sizeof(int32_t)},
                  {excl_off, off_bytes},
                  {excl_items, (size_t)excl_entries * sizeof(int32_t)},
                  {coef, (size_t)rows * sizeof(double)},
                  {U_init, row_bytes}};
    const struct {
        const void *p;
        size_t n;
    } outputs[] = {{U_out, row_bytes},
                   {info, info_bytes},
                   {objective, (size_t)rows * 2 * sizeof(double)},
                   {grad_ratio, (size_t)rows * sizeof(double)},
                   {iters_status, (size_t)rows * 2 * sizeof(int32_t)}};
    for (const auto &out : outputs) {
        if (!out.p) continue;
        for (const auto &in : inputs)
            if (in.p && (out.p == in.p || fold_overlap(out.p, out.n, in.p, in.n))) return MFCD_EINVAL;
        for (const auto &other : outputs)
            if (other.p && &other != &out && (out.p == other.p || fold_overlap(out.p, out.n, other.p, other.n)))
                return MFCD_EINVAL;
    }
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_implicit_fold_in_workspace_bytes(rows, m, d)) return MFCD_EWORKSPACE;
    IfArgs g{V,    m,  d,      pos_off,    pos_items, entries, excl_off,  excl_items, excl_entries, 0,
             coef, l2, U_init, max_newton, gtol,      U_out,   objective, grad_ratio, iters_status, info};
    hipStream_t st = (hipStream_t)stream;
    if (d <= 4) return if_launch<4>(g, rows, st);
    if (d <= 16) return if_launch<16>(g, rows, st);
    if (d <= 32) return if_launch<32>(g, rows, st);
    return if_launch<64>(g, rows, st);
}
