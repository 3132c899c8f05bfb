// What the pair kernels of pairs.hip and pair_info.hip share: the limits of a call, the pair law's kernel arguments, its
// weight, its argument check and the dispatch over its three flags.
#pragma once
#include <cmath>

#include "common.h"

namespace {

constexpr int kPairMaxCols = 1 << 20;
constexpr int64_t kPairMaxBlocks = 1 << 20;            // (row, tile) workgroups per launch: bounds the workspace at 80 MiB

// Rows per launch of a kernel with T (row, tile) workgroups per row: long inputs go through in blocks of rows of at most
// kPairMaxBlocks workgroups and at most `cap` rows (what the kernel's per-row workspace allows).
inline int pair_chunk_rows(int rows, int T, int64_t cap)
{
    int64_t R = kPairMaxBlocks / T;                    // >= 128
    if (R > cap) R = cap;
    return (int)(rows < R ? rows : R);
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

// F: a functor template over the three flags; picks the instantiation the law needs.
template <template <bool, bool, bool> class F, class... Args>
void law_dispatch(bool hw, bool hm, bool hl, Args... args)
{
    switch ((hw ? 1 : 0) | (hm ? 2 : 0) | (hl ? 4 : 0)) {
    case 0: F<false, false, false>::go(args...); break;
    case 1: F<true, false, false>::go(args...); break;
    case 2: F<false, true, false>::go(args...); break;
    case 3: F<true, true, false>::go(args...); break;
    case 4: F<false, false, true>::go(args...); break;
    case 5: F<true, false, true>::go(args...); break;
    case 6: F<false, true, true>::go(args...); break;
    default: F<true, true, true>::go(args...); break;
    }
}

}  // namespace
