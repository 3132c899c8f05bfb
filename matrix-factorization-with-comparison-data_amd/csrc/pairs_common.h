// What the pair kernels of pairs.hip, pair_info.hip, pair_best.hip and pair_ragged.hip share: the limits of a call and the
// host loop over its launches, the opening argument check, the pair law's kernel arguments, its weight, its argument
// check and the dispatch over its three flags, the per-pair arithmetic of the statistics, gradient and Hessian-vector
// kernels, and the statistics' workgroup reduction and partial (DESIGN sections 3.10, 3.13, 3.14).
#pragma once
#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace {

constexpr int kPairMaxCols = 1 << 20;
constexpr int64_t kPairMaxBlocks = 1 << 20;            // (row, tile) workgroups per launch: bounds the workspace at 80 MiB

// Rows per launch of a kernel with T (row, tile) workgroups per row: long inputs go through in blocks of rows of at most
// kPairMaxBlocks workgroups and at most `cap` rows (what the kernel's per-row workspace allows).
inline int pair_chunk_rows(int rows, int T, int64_t cap = kPairMaxBlocks)
{
    int64_t R = kPairMaxBlocks / T;                    // >= 128
    if (R > cap) R = cap;
    return (int)(rows < R ? rows : R);
}

// The host loop of every entry: [0, n) in blocks of at most `step`, launch(i0, count) per block in stream order → the
// first non-zero status.  Rows (r0, nr) for the dense entries, tiles (t0, nb) for the ragged ones.
template <class I, class F>
int pair_chunks(I n, I step, F launch)
{
    for (I i0 = 0; i0 < n; i0 += step)
        if (int rc = launch(i0, n - i0 < step ? n - i0 : step)) return rc;
    return 0;
}

// The opening check of the dense entries → 0, or MFCD_EINVAL: the two inputs, the call's size, every leading dimension
// (those of absent arrays are passed as m), a scale that is finite in fp32 (entries without a scale pass 0).
inline int pair_args(const void *A, const void *B, int rows, int m, double scale, std::initializer_list<int64_t> lds)
{
    if (!A || !B || rows < 0 || m < 1 || m > kPairMaxCols) return MFCD_EINVAL;
    for (int64_t ld : lds)
        if (ld < m) return MFCD_EINVAL;
    return std::isfinite(scale) && std::isfinite((float)scale) ? 0 : MFCD_EINVAL;
}

// Every unordered pair {i, j} of a row carries a weight
//   w = (alpha_i beta_j + alpha_j beta_i   or 1)  *  [|x_i - x_j| <= margin]  *  [label_i != label_j],
// each factor present or not (template flags HW, HM, HL: an absent factor costs no load and no instruction).
struct LawArgs {
    const float *alpha, *beta;     // [m], both or neither
    const int32_t *labels;         // row r reads labels + r * label_stride
    int64_t label_stride;
    float margin;                  // floor32 of the caller's
};

template <bool HW, bool HM, bool HL>
__device__ __forceinline__ float law_weight(float dx, float ali, float bei, int li, float alj, float bej, int lj, float mg)
{
    float w = HW ? fmaf(ali, bej, __fmul_rn(alj, bei)) : 1.0f;   // a product of its own: never contracted
    if (HM) w = fabsf(dx) <= mg ? w : 0.0f;
    if (HL) w = li != lj ? w : 0.0f;
    return w;
}

// The largest fp32 <= margin (margin >= 0, not NaN).
inline float floor32(double margin)
{
    float f = (float)margin;
    if ((double)f > margin) f = std::nextafterf(f, -INFINITY);
    return f;
}

// The shared part of the law entries' argument check → 0, or MFCD_EINVAL; fills the kernels' LawArgs.
inline int law_args(const mfcd_pair_law *law, int m, LawArgs *out)
{
    if (!law || (law->alpha == nullptr) != (law->beta == nullptr)) return MFCD_EINVAL;
    if (law->use_margin && !(law->margin >= 0.0)) return MFCD_EINVAL;          // negative or NaN
    if (law->labels && law->label_stride != 0 && law->label_stride < m) return MFCD_EINVAL;
    out->alpha = law->alpha;
    out->beta = law->beta;
    out->labels = law->labels;
    out->label_stride = law->label_stride;
    out->margin = law->use_margin ? floor32(law->margin) : 0.0f;
    return 0;
}

// The law of rows r0, r0 + 1, ... of a call: the labels move with the rows.
inline LawArgs law_rows(LawArgs la, int64_t r0)
{
    if (la.labels) la.labels += r0 * la.label_stride;
    return la;
}

// f: a generic lambda that receives the law's three flags (alpha / beta, margin, labels) as std::bool_constant tags and
// launches the instantiation they name: hw() is a constant expression inside it.
template <class F>
void law_dispatch(const LawArgs &la, bool use_margin, F f)
{
    constexpr std::true_type y{};
    constexpr std::false_type n{};
    switch ((la.alpha ? 1 : 0) | (use_margin ? 2 : 0) | (la.labels ? 4 : 0)) {
    case 0: f(n, n, n); break;
    case 1: f(y, n, n); break;
    case 2: f(n, y, n); break;
    case 3: f(y, y, n); break;
    case 4: f(n, n, y); break;
    case 5: f(y, n, y); break;
    case 6: f(n, y, y); break;
    default: f(y, y, y); break;
    }
}

// ---- the per-pair arithmetic of the statistics and gradient kernels (pairs.hip, pair_ragged.hip) ----
// One pair.  f: the run's fp32 accumulators — log2(1 + e) and the linear part of the two risks apart (ln 2 is applied
// once, in f64), exp_acc, bayes_acc.
template <int WHAT, bool MASKED>
__device__ __forceinline__ void pair_term(float ai, float xi, float aj, float xj, bool valid, float scale,
                                          unsigned (&cnt)[4], float (&f)[6])
{
    const bool la = ai < aj, ga = ai > aj, lx = xi < xj, gx = xi > xj;
    const bool v = !MASKED || valid;
    if (WHAT & 1) {                                    // comparison masks combine on the scalar unit
        cnt[0] += (unsigned)(v && ((la && lx) || (ga && gx)));
        cnt[1] += (unsigned)(v && ((la && gx) || (ga && lx)));
        cnt[2] += (unsigned)(v && (la || ga));         // strictly ordered in a: Ta = n0 - this, in the finishing kernel
        cnt[3] += (unsigned)(v && (lx || gx));         // (a row with a NaN is voided there)
    }
    if (WHAT & 2) {
        const float da = ai - aj, t = scale * (xi - xj);
        const float ada = v ? fabsf(da) : 0.0f, at = v ? fabsf(t) : 0.0f;
        const float ea = __builtin_amdgcn_exp2f(-1.4426950408889634f * ada);       // exp(-|da|): v_exp_f32
        const float et = __builtin_amdgcn_exp2f(-1.4426950408889634f * at);
        const float l2a = __builtin_amdgcn_logf(1.0f + ea), l2t = __builtin_amdgcn_logf(1.0f + et);   // v_log_f32: log2
        const float qhi = __builtin_amdgcn_rcpf(1.0f + et), qlo = et * qhi;       // sigmoid(|t|), sigmoid(-|t|)
        // the scores order the pair against the side the label law leans to: then 1 - q (for da > 0) or q (da < 0) is
        // q_hi and the pair is right with probability q_lo; otherwise the other way round
        const bool against = ga != (t >= 0.0f);
        const float miss = against ? qhi : qlo, hit = against ? qlo : qhi;
        const float eacc = (ga || la) ? hit : 0.5f;
        f[0] += v ? l2a : 0.0f;
        f[1] = fmaf(ada, miss, f[1]);
        f[2] += v ? l2t : 0.0f;
        f[3] = fmaf(at, qlo, f[3]);
        f[4] += v ? eacc : 0.0f;
        f[5] += v ? qhi : 0.0f;
    }
}

// sigmoid(v) from exp of a non-positive argument only: sigmoid(|v|) = 1 / (1 + e), sigmoid(-|v|) = e / (1 + e), selected
// by the sign, never formed as 1 - sigmoid.  v = +-0 gives the same value for either sign.
__device__ __forceinline__ float pair_sigmoid(float v)
{
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(v));       // exp(-|v|) <= 1: v_exp_f32
    const float hi = __builtin_amdgcn_rcpf(1.0f + e);
    return v >= 0.0f ? hi : e * hi;
}

// sigmoid'(da) = e h h with e = exp(-|da|), h = 1 / (1 + e): symmetric in the sign of da, so nothing is selected and
// nothing cancels; one exp and one reciprocal.  The Hessian-vector kernels' pair (pairs.hip, pair_ragged.hip).
__device__ __forceinline__ float pair_curvature(float da)
{
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(da));   // exp(-|da|) <= 1
    const float h = __builtin_amdgcn_rcpf(1.0f + e);
    return e * h * h;
}

// ---- what the statistics kernels of pairs.hip and pair_ragged.hip share around the pair loops ----
// The sums of NC 64-bit counters and NS f64 sums over a workgroup of WAVES waves: an xor tree within each wave, then
// the waves in index order, by thread 0, which hands the totals to store(c, s).  Every thread of the workgroup calls it.
template <int WAVES, int NC, int NS, class F>
__device__ __forceinline__ void pair_block_sum(int tid, long long (&c)[NC], double (&s)[NS], F store)
{
    __shared__ long long red_c[WAVES][NC];
    __shared__ double red_s[WAVES][NS];
#pragma unroll
    for (int q = 0; q < NC; ++q) c[q] = wave_sum_xor(c[q]);
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = wave_sum_xor(s[q]);
    if ((tid & 63) == 0) {
        for (int q = 0; q < NC; ++q) red_c[tid >> 6][q] = c[q];
        for (int q = 0; q < NS; ++q) red_s[tid >> 6][q] = s[q];
    }
    __syncthreads();
    if (tid == 0) {
        long long ct[NC];
        double st[NS];
        for (int q = 0; q < NC; ++q) {
            ct[q] = 0;
            for (int w = 0; w < WAVES; ++w) ct[q] += red_c[w][q];
        }
        for (int q = 0; q < NS; ++q) {
            st[q] = 0.0;
            for (int w = 0; w < WAVES; ++w) st[q] += red_s[w][q];   // fixed order
        }
        store(ct, st);
    }
}

// What one workgroup of a statistics kernel leaves in the workspace: one per (row, tile I), dense or ragged.
struct PairPartial {
    long long c[4];     // C, D, pairs strictly ordered in a, in x, of this tile
    long long bad[2];   // NaN entries, non-finite entries (NaN included) among the tile's own elements
    double s[4];        // risk, bayes_risk, exp_acc, bayes_acc
};
static_assert(sizeof(PairPartial) == 80, "workspace layout");

}  // namespace
