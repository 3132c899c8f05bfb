// pairs.hip — exact all-pairs statistics of a score row against a ground-truth row on gfx950.
//
// For row r of A (model scores a) and row r of X (ground truth x), over the n0 = m (m - 1) / 2 unordered pairs i < j:
//   counts  C, D, Ta, Tx — concordant, discordant, tied in a, tied in x — as exact integers: every decision is a plain
//           comparison of the two values themselves (never the sign of a difference or of a product), every sum an
//           integer sum.  Kendall's tau-b and the pairwise accuracy are functions of these four numbers.
//   sums    of the BTL population risk softplus(da) - q da, its Bayes floor softplus(t) - q t, the expected accuracy and
//           its Bayes ceiling, with da = a_i - a_j, t = scale (x_i - x_j), q = sigmoid(t).  Per-pair arithmetic is fp32;
//           a thread adds at most 64 terms in fp32 before it widens to f64 (a run of equal terms, which a row of few
//           levels produces, rounds the same way every time: the bound on that drift is 64 half-ulps, 2e-6 relative).
// There is no sort and no shortcut: the risk is not a function of the ranks, so all pairs are visited, and the counts
// ride in the same pass.
//
// One workgroup of 256 threads per (row, tile I) of kPairTile = 1024 columns.  Tile I sits in registers, four (a, x)
// elements per thread (element k of thread t is column 1024 I + 256 k + t: coalesced loads); the tiles J >= I stream
// through 8 KiB of LDS and every lane reads the same (a_j, x_j) — a broadcast, conflict-free.  Tiles J > I need no
// mask.  The diagonal tile is walked in four runs of 256 columns: in run c the elements k < c of every thread pair
// with all of the run, element k == c is masked to i < j, elements k > c are skipped (6 + 4/2 of 16 sub-blocks do work
// that counts, instead of all 16 under a mask).
//
// Per pair the sums take five transcendentals — exp(-|da|), exp(-|t|), two logs of 1 + e, one reciprocal — and are
// written so that nothing cancels: with e = exp(-|t|), q_hi = 1 / (1 + e) and q_lo = e q_hi are sigmoid(|t|) and
// sigmoid(-|t|), so q and 1 - q are both selected, never subtracted, and
//   softplus(da) - q da = log1p(exp(-|da|)) + |da| (da > 0 ? 1 - q : q),   softplus(t) - q t = log1p(e) + |t| q_lo.
// Which of q_hi, q_lo is selected depends on one bit, whether the scores order the pair against the side the label
// law leans to.  The logs are taken in base 2 (the hardware's) and summed apart from the linear parts; ln 2 is applied
// once per workgroup, in f64.  Only exp of a non-positive argument is taken, so no row range overflows and there is
// no second formulation.
//
// Counters: a thread meets at most 4 m <= 2^22 pairs in a launch, so 32-bit per-thread counters cannot wrap; they are
// widened to 64 bits once, for the workgroup's sum.  No floating-point atomics: every workgroup writes one fixed-size
// partial per (row, tile I) into the workspace, and a one-wave finishing kernel per row adds the partials in a fixed
// order.  Two calls are therefore bit-equal, and the counts-only and sums-only kernels execute the same operations in
// the same order as the matching half of the combined kernel.
#include <cmath>

#include "common.h"
#include "pairs_common.h"

namespace {

constexpr int kPairThreads = 256;
constexpr int kPairIpt = 4;                            // elements of tile I per thread
constexpr int kPairTile = kPairThreads * kPairIpt;     // 1024 columns (mfcd/pairs.py: TILE)
constexpr int kPairFlush = 16;                         // columns between two widenings of the fp32 sums to f64

inline int pair_tiles(int m) { return (m + kPairTile - 1) / kPairTile; }

// Columns [j0, j1) of the LDS tile against this thread's elements: k < KFULL unmasked, k == KMASK (the run of the
// diagonal tile that holds element k itself, first column j0) only where the element's column is below j.
template <int WHAT, int KFULL, int KMASK>
__device__ __forceinline__ void pair_run(const float2 *tile, int j0, int j1, const float (&ai)[kPairIpt],
                                         const float (&xi)[kPairIpt], int tid, float scale, unsigned (&cnt)[4],
                                         double (&acc)[6])
{
    for (int jb = j0; jb < j1; jb += kPairFlush) {
        const int je = jb + kPairFlush < j1 ? jb + kPairFlush : j1;
        float f[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // at most kPairFlush columns x 4 elements = 64 terms each
#pragma unroll 4
        for (int j = jb; j < je; ++j) {
            const float2 v = tile[j];
#pragma unroll
            for (int k = 0; k < kPairIpt; ++k) {
                if (k < KFULL) pair_term<WHAT, false>(ai[k], xi[k], v.x, v.y, true, scale, cnt, f);
                else if (k == KMASK) pair_term<WHAT, true>(ai[k], xi[k], v.x, v.y, tid < j - j0, scale, cnt, f);
            }
        }
        if (WHAT & 2) {
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += (double)f[q];
        }
    }
}

template <int WHAT>
__global__ __launch_bounds__(kPairThreads) void pair_tiles_kernel(const float *__restrict__ A, int64_t lda,
                                                                  const float *__restrict__ X, int64_t ldx, int m, int T,
                                                                  float scale, PairPartial *__restrict__ part)
{
    __shared__ float2 tile[kPairTile];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x / T;
    const int I = (int)(blockIdx.x - r * T);
    const float *a = A + r * lda, *x = X + r * ldx;

    float ai[kPairIpt], xi[kPairIpt];
    unsigned n_nan = 0, n_inf = 0;
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        ai[k] = 0.0f;
        xi[k] = 0.0f;
        if (p < m) {
            ai[k] = a[p];
            xi[k] = x[p];
            n_nan += (unsigned)(ai[k] != ai[k] || xi[k] != xi[k]);
            n_inf += (unsigned)(is_nonfinite_bits(ai[k]) || is_nonfinite_bits(xi[k]));
        }
    }

    unsigned cnt[4] = {0u, 0u, 0u, 0u};                // <= 4 m <= 2^22 pairs per thread
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int J = I; J < T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < kPairIpt; ++k) {
            const int e = k * kPairThreads + tid, p = J * kPairTile + e;
            float2 v = make_float2(ai[k], xi[k]);      // J == I: the tile is this workgroup's own elements
            if (J != I) v = p < m ? make_float2(a[p], x[p]) : make_float2(0.0f, 0.0f);
            tile[e] = v;
        }
        __syncthreads();
        const int jn = m - J * kPairTile < kPairTile ? m - J * kPairTile : kPairTile;   // columns of tile J that exist
        const auto end = [jn](int j1) { return j1 < jn ? j1 : jn; };
        if (J != I) {
            for (int c = 0; c < kPairIpt; ++c)
                pair_run<WHAT, kPairIpt, kPairIpt>(tile, c * kPairThreads, end((c + 1) * kPairThreads), ai, xi, tid, scale,
                                                   cnt, acc);
        } else {                                       // an element past m only meets columns past m: j < jn bars both
            pair_run<WHAT, 0, 0>(tile, 0, end(256), ai, xi, tid, scale, cnt, acc);
            pair_run<WHAT, 1, 1>(tile, 256, end(512), ai, xi, tid, scale, cnt, acc);
            pair_run<WHAT, 2, 2>(tile, 512, end(768), ai, xi, tid, scale, cnt, acc);
            pair_run<WHAT, 3, 3>(tile, 768, end(1024), ai, xi, tid, scale, cnt, acc);
        }
    }

    long long c6[6] = {(long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3], (long long)n_nan,
                       (long long)n_inf};
    pair_block_sum<kPairThreads / 64>(tid, c6, acc, [&](const long long(&c)[6], const double(&s)[6]) {
        PairPartial out;
        for (int q = 0; q < 4; ++q) out.c[q] = c[q];
        out.bad[0] = c[4];
        out.bad[1] = c[5];
        out.s[0] = 0.6931471805599453 * s[0] + s[1];
        out.s[1] = 0.6931471805599453 * s[2] + s[3];
        out.s[2] = s[4];
        out.s[3] = s[5];
        part[blockIdx.x] = out;
    });
}

// One wave per row: lane l adds the partials of tiles l, l + 64, ... in order, then the lanes are added in a fixed tree.
__global__ __launch_bounds__(64) void pair_finish_kernel(const PairPartial *__restrict__ part, int T, long long n0, int what,
                                                         int64_t *__restrict__ counts, double *__restrict__ sums)
{
    const int64_t r = blockIdx.x;
    long long c6[6] = {0, 0, 0, 0, 0, 0};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int I = threadIdx.x; I < T; I += 64) {
        const PairPartial &p = part[r * T + I];
        for (int q = 0; q < 4; ++q) c6[q] += p.c[q];
        c6[4] += p.bad[0];
        c6[5] += p.bad[1];
        for (int q = 0; q < 4; ++q) s[q] += p.s[q];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) c6[q] = wave_sum_xor(c6[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = wave_sum_xor(s[q]);
    if (threadIdx.x == 0) {
        if (what & 1)
            for (int q = 0; q < 4; ++q) counts[r * 4 + q] = c6[4] ? -1 : q < 2 ? c6[q] : n0 - c6[q];
        if (what & 2)
            for (int q = 0; q < 4; ++q) sums[r * 4 + q] = c6[5] ? __longlong_as_double(0x7ff8000000000000ll) : s[q];
    }
}

// ---- the statistics under a pair law (second follow-on) ----
// Every unordered pair {i, j} of a row carries a weight
//   w = (alpha_i beta_j + alpha_j beta_i   or 1)  *  [|x_i - x_j| <= margin]  *  [label_i != label_j],
// each factor present or not (template flags HW, HM, HL: an absent factor costs no load and no instruction).  The sums
// become sums of w * term, W = sum of w rides along, and `support` counts the pairs with w > 0.  The decomposition is
// the unweighted kernels'; the LDS element grows to (a, x, alpha, beta) — still one broadcast read — plus the label:
// 20 KiB per workgroup.  Masks fold into w (0 where masked) and every accumulation is fma(w, term, f); all terms of the
// sums are non-negative, so w = 0 adds exactly +0.  The margin arrives rounded down to fp32: fabsf(dx) <= floor32(margin)
// decides as (double)fabsf(dx) <= margin does.
struct LawPartial {
    long long support, bad;   // pairs with w > 0; non-finite entries among tile I's elements
    double s[5];              // W, risk, bayes_risk, exp_acc, bayes_acc
};
static_assert(sizeof(LawPartial) == 56, "workspace layout");

template <bool HW> struct LawElem { typedef float2 type; };
template <> struct LawElem<true> { typedef float4 type; };

// One element of this thread against one column: f = log2 parts and linear parts of the two risks, exp_acc, bayes_acc, W.
template <bool HW, bool HM, bool HL, bool MASKED>
__device__ __forceinline__ void law_term(float ai, float xi, float ali, float bei, int li, float aj, float xj, float alj,
                                         float bej, int lj, bool valid, float scale, float mg, unsigned &support,
                                         float (&f)[7])
{
    const float da = ai - aj, dx = xi - xj, t = scale * dx;
    float w = law_weight<HW, HM, HL>(dx, ali, bei, li, alj, bej, lj, mg);
    if (MASKED) w = valid ? w : 0.0f;
    support += (unsigned)(w > 0.0f);
    const float ada = fabsf(da), at = fabsf(t);
    const float ea = __builtin_amdgcn_exp2f(-1.4426950408889634f * ada);
    const float et = __builtin_amdgcn_exp2f(-1.4426950408889634f * at);
    const float l2a = __builtin_amdgcn_logf(1.0f + ea), l2t = __builtin_amdgcn_logf(1.0f + et);
    const float qhi = __builtin_amdgcn_rcpf(1.0f + et), qlo = et * qhi;
    const bool ga = ai > aj, la = ai < aj;
    const bool against = ga != (t >= 0.0f);
    const float miss = against ? qhi : qlo, hit = against ? qlo : qhi;
    const float eacc = (ga || la) ? hit : 0.5f;
    f[0] = fmaf(w, l2a, f[0]);
    f[1] = fmaf(w, __fmul_rn(ada, miss), f[1]);      // rounded apart, so that w = 1 adds the same bits as a constant 1
    f[2] = fmaf(w, l2t, f[2]);
    f[3] = fmaf(w, __fmul_rn(at, qlo), f[3]);
    f[4] = fmaf(w, eacc, f[4]);
    f[5] = fmaf(w, qhi, f[5]);
    if (HW) f[6] += w;                                 // without alpha/beta W is the support itself
}

template <bool HW, bool HM, bool HL, int KFULL, int KMASK>
__device__ __forceinline__ void law_run(const typename LawElem<HW>::type *tile, const int *lab, int j0, int j1,
                                        const float (&ai)[kPairIpt], const float (&xi)[kPairIpt],
                                        const float (&ali)[kPairIpt], const float (&bei)[kPairIpt],
                                        const int (&li)[kPairIpt], int tid, float scale, float mg, unsigned &support,
                                        double (&acc)[7])
{
    for (int jb = j0; jb < j1; jb += kPairFlush) {
        const int je = jb + kPairFlush < j1 ? jb + kPairFlush : j1;
        float f[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // at most kPairFlush columns x 4 elements = 64 terms each
#pragma unroll 4
        for (int j = jb; j < je; ++j) {
            const typename LawElem<HW>::type v = tile[j];
            float alj = 0.0f, bej = 0.0f;
            if constexpr (HW) {
                alj = v.z;
                bej = v.w;
            }
            const int lj = HL ? lab[j] : 0;
#pragma unroll
            for (int k = 0; k < kPairIpt; ++k) {
                if (k < KFULL)
                    law_term<HW, HM, HL, false>(ai[k], xi[k], ali[k], bei[k], li[k], v.x, v.y, alj, bej, lj, true, scale, mg,
                                                support, f);
                else if (k == KMASK)
                    law_term<HW, HM, HL, true>(ai[k], xi[k], ali[k], bei[k], li[k], v.x, v.y, alj, bej, lj, tid < j - j0,
                                               scale, mg, support, f);
            }
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) acc[q] += (double)f[q];
    }
}

template <bool HW> __device__ __forceinline__ typename LawElem<HW>::type law_elem(float a, float x, float al, float be);
template <> __device__ __forceinline__ float2 law_elem<false>(float a, float x, float, float) { return make_float2(a, x); }
template <> __device__ __forceinline__ float4 law_elem<true>(float a, float x, float al, float be)
{
    return make_float4(a, x, al, be);
}

template <bool HW, bool HM, bool HL>
__global__ __launch_bounds__(kPairThreads) void pair_law_tiles_kernel(const float *__restrict__ A, int64_t lda,
                                                                      const float *__restrict__ X, int64_t ldx, LawArgs law,
                                                                      int m, int T, float scale,
                                                                      LawPartial *__restrict__ part)
{
    __shared__ typename LawElem<HW>::type tile[kPairTile];
    __shared__ int lab[HL ? kPairTile : 1];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x / T;
    const int I = (int)(blockIdx.x - r * T);
    const float *a = A + r * lda, *x = X + r * ldx;
    const int32_t *lb = HL ? law.labels + r * law.label_stride : nullptr;

    float ai[kPairIpt], xi[kPairIpt], ali[kPairIpt], bei[kPairIpt];
    int li[kPairIpt];
    unsigned n_inf = 0;
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        ai[k] = xi[k] = ali[k] = bei[k] = 0.0f;
        li[k] = 0;
        if (p < m) {
            ai[k] = a[p];
            xi[k] = x[p];
            if (HW) {
                ali[k] = law.alpha[p];
                bei[k] = law.beta[p];
            }
            if (HL) li[k] = lb[p];
            n_inf += (unsigned)(is_nonfinite_bits(ai[k]) || is_nonfinite_bits(xi[k]));
        }
    }

    unsigned support = 0u;                             // <= 4 m <= 2^22 pairs per thread
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int J = I; J < T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < kPairIpt; ++k) {
            const int e = k * kPairThreads + tid, p = J * kPairTile + e;
            if (J == I) {                              // the tile is this workgroup's own elements
                tile[e] = law_elem<HW>(ai[k], xi[k], ali[k], bei[k]);
                if (HL) lab[e] = li[k];
            } else {                                   // zero-filled pad columns: alpha = beta = 0, and jn bars them
                const bool in = p < m;
                tile[e] = law_elem<HW>(in ? a[p] : 0.0f, in ? x[p] : 0.0f, HW && in ? law.alpha[p] : 0.0f,
                                       HW && in ? law.beta[p] : 0.0f);
                if (HL) lab[e] = in ? lb[p] : 0;
            }
        }
        __syncthreads();
        const int jn = m - J * kPairTile < kPairTile ? m - J * kPairTile : kPairTile;   // columns of tile J that exist
        const auto end = [jn](int j1) { return j1 < jn ? j1 : jn; };
        if (J != I) {
            for (int c = 0; c < kPairIpt; ++c)
                law_run<HW, HM, HL, kPairIpt, kPairIpt>(tile, lab, c * kPairThreads, end((c + 1) * kPairThreads), ai, xi, ali,
                                                        bei, li, tid, scale, law.margin, support, acc);
        } else {                                       // an element past m only meets columns past m: j < jn bars both
            law_run<HW, HM, HL, 0, 0>(tile, lab, 0, end(256), ai, xi, ali, bei, li, tid, scale, law.margin, support, acc);
            law_run<HW, HM, HL, 1, 1>(tile, lab, 256, end(512), ai, xi, ali, bei, li, tid, scale, law.margin, support, acc);
            law_run<HW, HM, HL, 2, 2>(tile, lab, 512, end(768), ai, xi, ali, bei, li, tid, scale, law.margin, support, acc);
            law_run<HW, HM, HL, 3, 3>(tile, lab, 768, end(1024), ai, xi, ali, bei, li, tid, scale, law.margin, support, acc);
        }
    }

    long long c2[2] = {(long long)support, (long long)n_inf};
    pair_block_sum<kPairThreads / 64>(tid, c2, acc, [&](const long long(&c)[2], const double(&s)[7]) {
        LawPartial out;
        out.support = c[0];
        out.bad = c[1];
        out.s[0] = HW ? s[6] : (double)out.support;
        out.s[1] = 0.6931471805599453 * s[0] + s[1];
        out.s[2] = 0.6931471805599453 * s[2] + s[3];
        out.s[3] = s[4];
        out.s[4] = s[5];
        part[blockIdx.x] = out;
    });
}

// One wave per row, as pair_finish_kernel: a fixed order over the tiles, then a fixed tree over the lanes.
__global__ __launch_bounds__(64) void pair_law_finish_kernel(const LawPartial *__restrict__ part, int T,
                                                             int64_t *__restrict__ support, double *__restrict__ sums)
{
    const int64_t r = blockIdx.x;
    long long c2[2] = {0, 0};
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int I = threadIdx.x; I < T; I += 64) {
        const LawPartial &p = part[r * T + I];
        c2[0] += p.support;
        c2[1] += p.bad;
        for (int q = 0; q < 5; ++q) s[q] += p.s[q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) c2[q] = wave_sum_xor(c2[q]);
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] = wave_sum_xor(s[q]);
    if (threadIdx.x == 0) {
        support[r] = c2[0];
        for (int q = 0; q < 5; ++q) sums[r * 5 + q] = c2[1] ? __longlong_as_double(0x7ff8000000000000ll) : s[q];
    }
}

// ---- the gradient of a row's risk sum (follow-on) ----
// g_i = sum over j != i of w_ij (sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j))): the derivative of the `risk` sum above
// with respect to a_i.  Same decomposition as the statistics — one workgroup per (row, tile I), four elements per thread
// in registers, tiles streamed through LDS and read as a broadcast — but EVERY tile J is visited, so a thread owns its
// four sums completely and stores them itself: no scatter to the j side, no workspace, no finishing kernel, no atomics,
// at the price of visiting each unordered pair twice.  One template serves the plain entry (no flag, an empty LawArgs:
// w = 1, the accumulation a plain add) and the law entry.  The column j == i needs no mask: both differences are +-0
// there, both sigmoids run the same instructions on the same e, and the term is exactly +0 whatever its weight.
constexpr int kGradFlush = 64;                         // columns, = terms per accumulator, between two widenings to f64

template <bool HW, bool HM, bool HL>
__global__ __launch_bounds__(kPairThreads) void pair_grad_kernel(const float *__restrict__ A, int64_t lda,
                                                                 const float *__restrict__ X, int64_t ldx, LawArgs law,
                                                                 int m, int T, float scale, float *__restrict__ G,
                                                                 int64_t ldg)
{
    __shared__ typename LawElem<HW>::type tile[kPairTile];
    __shared__ int lab[HL ? kPairTile : 1];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x / T;
    const int I = (int)(blockIdx.x - r * T);
    const float *a = A + r * lda, *x = X + r * ldx;
    const int32_t *lb = HL ? law.labels + r * law.label_stride : nullptr;
    const float mg = law.margin;

    float ai[kPairIpt], xi[kPairIpt], ali[kPairIpt], bei[kPairIpt];
    int li[kPairIpt];
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        const bool in = p < m;                         // an element past m is computed and never stored
        ai[k] = in ? a[p] : 0.0f;
        xi[k] = in ? x[p] : 0.0f;
        ali[k] = HW && in ? law.alpha[p] : 0.0f;
        bei[k] = HW && in ? law.beta[p] : 0.0f;
        li[k] = HL && in ? lb[p] : 0;
    }

    int bad = 0;                                       // the workgroup stages the whole row: it sees every entry
    double acc[kPairIpt] = {0.0, 0.0, 0.0, 0.0};
    for (int J = 0; J < T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < kPairIpt; ++k) {
            const int e = k * kPairThreads + tid, p = J * kPairTile + e;
            const bool in = p < m;
            const float va = in ? a[p] : 0.0f, vx = in ? x[p] : 0.0f;
            bad |= (int)(is_nonfinite_bits(va) || is_nonfinite_bits(vx));
            tile[e] = law_elem<HW>(va, vx, HW && in ? law.alpha[p] : 0.0f, HW && in ? law.beta[p] : 0.0f);
            if (HL) lab[e] = in ? lb[p] : 0;
        }
        __syncthreads();
        // columns of tile J that exist: a zero-filled pad column would be a real term here
        const int jn = m - J * kPairTile < kPairTile ? m - J * kPairTile : kPairTile;
        for (int jb = 0; jb < jn; jb += kGradFlush) {
            const int je = jb + kGradFlush < jn ? jb + kGradFlush : jn;
            float f[kPairIpt] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
            for (int j = jb; j < je; ++j) {
                const typename LawElem<HW>::type v = tile[j];
                float alj = 0.0f, bej = 0.0f;
                if constexpr (HW) {
                    alj = v.z;
                    bej = v.w;
                }
                const int lj = HL ? lab[j] : 0;
#pragma unroll
                for (int k = 0; k < kPairIpt; ++k) {
                    const float dx = xi[k] - v.y;
                    const float term = pair_sigmoid(ai[k] - v.x) - pair_sigmoid(scale * dx);
                    if constexpr (HW || HM || HL)
                        f[k] = fmaf(law_weight<HW, HM, HL>(dx, ali[k], bei[k], li[k], alj, bej, lj, mg), term, f[k]);
                    else f[k] += term;
                }
            }
#pragma unroll
            for (int k = 0; k < kPairIpt; ++k) acc[k] += (double)f[k];
        }
    }

    bad = __syncthreads_or(bad);
    float *g = G + r * ldg;
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        if (p < m) g[p] = bad ? __uint_as_float(0x7fc00000u) : (float)acc[k];     // rounded to fp32 once
    }
}

// ---- the Hessian of a row's risk sum times a vector (third follow-on) ----
// q_i = sum over j != i of w_ij s_ij (y_i - y_j),  s_ij = sigmoid'(a_i - a_j),  and optionally deg_i = sum over j != i of
// w_ij s_ij: the weighted graph Laplacian L(a) applied to y, and its diagonal.  The decomposition is pair_grad_kernel's
// (every tile J visited, a thread owns its four sums and stores them itself); one template serves the plain entry
// (LAW = false: no x, w = 1) and the law entry, whose flags are pair_grad_kernel's.
//   s = e h h with e = exp(-|v|), h = 1 / (1 + e): symmetric in the sign of v, so nothing is selected and nothing
//   cancels; one exp and one reciprocal per ordered pair.  The term is s (y_i - y_j), the difference formed first.
// The column j == i adds exactly 0 to q (its difference is +0) but s = 1/4 to deg: with DEG the element that can meet its
// own column in a run of the diagonal tile (element c in run c, at column tid of the run) has s zeroed there.
template <bool DEG, int KMASK, bool HW, bool HM, bool HL>
__device__ __forceinline__ void hvp_run(const float2 *tile, const float *tx, const float2 *tab, const int *lab, int j0,
                                        int j1, const float (&ai)[kPairIpt], const float (&yi)[kPairIpt],
                                        const float (&xi)[kPairIpt], const float (&ali)[kPairIpt],
                                        const float (&bei)[kPairIpt], const int (&li)[kPairIpt], int tid, float mg,
                                        double (&acc)[kPairIpt], double (&dacc)[kPairIpt])
{
    for (int jb = j0; jb < j1; jb += kGradFlush) {
        const int je = jb + kGradFlush < j1 ? jb + kGradFlush : j1;
        float f[kPairIpt] = {0.0f, 0.0f, 0.0f, 0.0f}, g[kPairIpt] = {0.0f, 0.0f, 0.0f, 0.0f};   // <= 64 terms each
#pragma unroll 4
        for (int j = jb; j < je; ++j) {
            const float2 v = tile[j];
            const float xj = HM ? tx[j] : 0.0f;
            float alj = 0.0f, bej = 0.0f;
            if constexpr (HW) {
                alj = tab[j].x;
                bej = tab[j].y;
            }
            const int lj = HL ? lab[j] : 0;
#pragma unroll
            for (int k = 0; k < kPairIpt; ++k) {
                float s = pair_curvature(ai[k] - v.x);
                if (HW || HM || HL)
                    s = __fmul_rn(law_weight<HW, HM, HL>(HM ? xi[k] - xj : 0.0f, ali[k], bei[k], li[k], alj, bej, lj, mg), s);
                if (DEG && k == KMASK) s = j - j0 == tid ? 0.0f : s;
                f[k] = fmaf(s, yi[k] - v.y, f[k]);
                if (DEG) g[k] += s;
            }
        }
#pragma unroll
        for (int k = 0; k < kPairIpt; ++k) {
            acc[k] += (double)f[k];
            if (DEG) dacc[k] += (double)g[k];
        }
    }
}

template <bool LAW, bool HW, bool HM, bool HL, bool DEG>
__global__ __launch_bounds__(kPairThreads) void pair_hvp_kernel(const float *__restrict__ A, int64_t lda,
                                                                const float *__restrict__ X, int64_t ldx,
                                                                const float *__restrict__ Y, int64_t ldy, LawArgs law, int m,
                                                                int T, float *__restrict__ Q, int64_t ldq,
                                                                float *__restrict__ Dg, int64_t ldd)
{
    __shared__ float2 tile[kPairTile];                 // (a, y)
    __shared__ float tx[HM ? kPairTile : 1];
    __shared__ float2 tab[HW ? kPairTile : 1];         // (alpha, beta)
    __shared__ int lab[HL ? kPairTile : 1];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x / T;
    const int I = (int)(blockIdx.x - r * T);
    const float *a = A + r * lda, *y = Y + r * ldy, *x = LAW ? X + r * ldx : nullptr;
    const int32_t *lb = HL ? law.labels + r * law.label_stride : nullptr;

    float ai[kPairIpt], yi[kPairIpt], xi[kPairIpt], ali[kPairIpt], bei[kPairIpt];
    int li[kPairIpt];
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        const bool in = p < m;                         // an element past m is computed and never stored
        ai[k] = in ? a[p] : 0.0f;
        yi[k] = in ? y[p] : 0.0f;
        xi[k] = HM && in ? x[p] : 0.0f;
        ali[k] = HW && in ? law.alpha[p] : 0.0f;
        bei[k] = HW && in ? law.beta[p] : 0.0f;
        li[k] = HL && in ? lb[p] : 0;
    }

    int bad = 0;                                       // the workgroup stages the whole row: it sees every entry
    double acc[kPairIpt] = {0.0, 0.0, 0.0, 0.0}, dacc[kPairIpt] = {0.0, 0.0, 0.0, 0.0};
    for (int J = 0; J < T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < kPairIpt; ++k) {
            const int e = k * kPairThreads + tid, p = J * kPairTile + e;
            const bool in = p < m;
            const float va = in ? a[p] : 0.0f, vy = in ? y[p] : 0.0f, vx = LAW && in ? x[p] : 0.0f;
            bad |= (int)(is_nonfinite_bits(va) || is_nonfinite_bits(vy) || is_nonfinite_bits(vx));
            tile[e] = make_float2(va, vy);
            if (HM) tx[e] = vx;
            if (HW) tab[e] = make_float2(in ? law.alpha[p] : 0.0f, in ? law.beta[p] : 0.0f);
            if (HL) lab[e] = in ? lb[p] : 0;
        }
        __syncthreads();
        const int jn = m - J * kPairTile < kPairTile ? m - J * kPairTile : kPairTile;   // pad columns stay out
        if (DEG && J == I) {                           // run c holds element c's own column
            const auto end = [jn](int j1) { return j1 < jn ? j1 : jn; };
            hvp_run<DEG, 0, HW, HM, HL>(tile, tx, tab, lab, 0, end(256), ai, yi, xi, ali, bei, li, tid, law.margin, acc, dacc);
            hvp_run<DEG, 1, HW, HM, HL>(tile, tx, tab, lab, 256, end(512), ai, yi, xi, ali, bei, li, tid, law.margin, acc, dacc);
            hvp_run<DEG, 2, HW, HM, HL>(tile, tx, tab, lab, 512, end(768), ai, yi, xi, ali, bei, li, tid, law.margin, acc, dacc);
            hvp_run<DEG, 3, HW, HM, HL>(tile, tx, tab, lab, 768, end(1024), ai, yi, xi, ali, bei, li, tid, law.margin, acc, dacc);
        } else {
            hvp_run<DEG, -1, HW, HM, HL>(tile, tx, tab, lab, 0, jn, ai, yi, xi, ali, bei, li, tid, law.margin, acc, dacc);
        }
    }

    bad = __syncthreads_or(bad);
    float *q = Q + r * ldq, *dg = DEG ? Dg + r * ldd : nullptr;
#pragma unroll
    for (int k = 0; k < kPairIpt; ++k) {
        const int p = I * kPairTile + k * kPairThreads + tid;
        if (p < m) {                                   // rounded to fp32 once
            q[p] = bad ? __uint_as_float(0x7fc00000u) : (float)acc[k];
            if (DEG) dg[p] = bad ? __uint_as_float(0x7fc00000u) : (float)dacc[k];
        }
    }
}

// The rest of the two Hessian-vector entries' argument check, after pair_args (X = nullptr: the plain entry).
inline int hvp_args(const float *A, const float *X, const float *Y, const float *Q, const float *deg)
{
    if (!Q || Q == A || Q == Y || Q == X || Q == deg) return MFCD_EINVAL;
    if (deg && (deg == A || deg == Y || deg == X)) return MFCD_EINVAL;
    return 0;
}

inline dim3 pair_grid(int nr, int T) { return dim3((unsigned)((int64_t)nr * T)); }

}  // namespace

extern "C" size_t mfcd_pair_stats_workspace_bytes(int rows, int m)
{
    if (rows < 0 || m < 1 || m > kPairMaxCols) return 0;
    const int T = pair_tiles(m), R = pair_chunk_rows(rows, T);
    return align_up((size_t)(R > 0 ? R : 1) * T * sizeof(PairPartial));
}

extern "C" int mfcd_pair_stats_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m,
                                    double scale, int what, int64_t *counts, double *sums, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (pair_args(A, X, rows, m, scale, {lda, ldx})) return MFCD_EINVAL;
    if (what < 1 || what > 3 || ((what & 1) && !counts) || ((what & 2) && !sums)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_pair_stats_workspace_bytes(rows, m)) return MFCD_EWORKSPACE;
    const int T = pair_tiles(m);
    PairPartial *part = (PairPartial *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const auto tiles = what == 1 ? pair_tiles_kernel<1> : what == 2 ? pair_tiles_kernel<2> : pair_tiles_kernel<3>;
    // stream order keeps one chunk's partials apart from the next's
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        hipLaunchKernelGGL(tiles, pair_grid(nr, T), dim3(kPairThreads), 0, st, A + (int64_t)r0 * lda, lda,
                           X + (int64_t)r0 * ldx, ldx, m, T, (float)scale, part);
        MFCD_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)nr), dim3(64), 0, st, part, T, (long long)m * (m - 1) / 2, what,
                           counts ? counts + (int64_t)r0 * 4 : nullptr, sums ? sums + (int64_t)r0 * 4 : nullptr);
        return (int)hipGetLastError();
    });
}

extern "C" int mfcd_pair_grad_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double scale,
                                   float *G, int64_t ldg, void *stream)
{
    if (pair_args(A, X, rows, m, scale, {lda, ldx, ldg}) || !G || G == A || G == X) return MFCD_EINVAL;
    const int T = pair_tiles(m);
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        hipLaunchKernelGGL((pair_grad_kernel<false, false, false>), pair_grid(nr, T), dim3(kPairThreads), 0,
                           (hipStream_t)stream, A + (int64_t)r0 * lda, lda, X + (int64_t)r0 * ldx, ldx, LawArgs{}, m, T,
                           (float)scale, G + (int64_t)r0 * ldg, ldg);
        return (int)hipGetLastError();
    });
}

extern "C" size_t mfcd_pair_law_stats_workspace_bytes(int rows, int m)
{
    if (rows < 0 || m < 1 || m > kPairMaxCols) return 0;
    const int T = pair_tiles(m), R = pair_chunk_rows(rows, T);
    return align_up((size_t)(R > 0 ? R : 1) * T * sizeof(LawPartial));
}

extern "C" int mfcd_pair_law_stats_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m,
                                        double scale, const mfcd_pair_law *law, int64_t *support, double *sums,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    LawArgs la;
    if (pair_args(A, X, rows, m, scale, {lda, ldx}) || !support || !sums || law_args(law, m, &la)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_pair_law_stats_workspace_bytes(rows, m)) return MFCD_EWORKSPACE;
    const int T = pair_tiles(m);
    LawPartial *part = (LawPartial *)workspace;
    hipStream_t st = (hipStream_t)stream;
    // stream order keeps one chunk's partials apart from the next's
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        law_dispatch(la, law->use_margin != 0, [&](auto hw, auto hm, auto hl) {
            hipLaunchKernelGGL((pair_law_tiles_kernel<hw(), hm(), hl()>), pair_grid(nr, T), dim3(kPairThreads), 0, st,
                               A + (int64_t)r0 * lda, lda, X + (int64_t)r0 * ldx, ldx, law_rows(la, r0), m, T, (float)scale,
                               part);
        });
        MFCD_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pair_law_finish_kernel, dim3((unsigned)nr), dim3(64), 0, st, part, T, support + r0,
                           sums + (int64_t)r0 * 5);
        return (int)hipGetLastError();
    });
}

extern "C" int mfcd_pair_law_grad_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m,
                                       double scale, const mfcd_pair_law *law, float *G, int64_t ldg, void *stream)
{
    LawArgs la;
    if (pair_args(A, X, rows, m, scale, {lda, ldx, ldg}) || !G || G == A || G == X || law_args(law, m, &la)) return MFCD_EINVAL;
    const int T = pair_tiles(m);
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        law_dispatch(la, law->use_margin != 0, [&](auto hw, auto hm, auto hl) {
            hipLaunchKernelGGL((pair_grad_kernel<hw(), hm(), hl()>), pair_grid(nr, T), dim3(kPairThreads), 0,
                               (hipStream_t)stream, A + (int64_t)r0 * lda, lda, X + (int64_t)r0 * ldx, ldx, law_rows(la, r0), m,
                               T, (float)scale, G + (int64_t)r0 * ldg, ldg);
        });
        return (int)hipGetLastError();
    });
}

extern "C" int mfcd_pair_hvp_rows(const float *A, int64_t lda, const float *Y, int64_t ldy, int rows, int m, float *Q,
                                  int64_t ldq, float *deg, int64_t ldd, void *stream)
{
    if (pair_args(A, Y, rows, m, 0.0, {lda, ldy, ldq, deg ? ldd : m}) || hvp_args(A, nullptr, Y, Q, deg)) return MFCD_EINVAL;
    const int T = pair_tiles(m);
    const auto kernel = deg ? pair_hvp_kernel<false, false, false, false, true> : pair_hvp_kernel<false, false, false, false, false>;
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        hipLaunchKernelGGL(kernel, pair_grid(nr, T), dim3(kPairThreads), 0, (hipStream_t)stream, A + (int64_t)r0 * lda, lda,
                           (const float *)nullptr, (int64_t)0, Y + (int64_t)r0 * ldy, ldy, LawArgs{}, m, T,
                           Q + (int64_t)r0 * ldq, ldq, deg ? deg + (int64_t)r0 * ldd : nullptr, ldd);
        return (int)hipGetLastError();
    });
}

extern "C" int mfcd_pair_law_hvp_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *Y, int64_t ldy,
                                      int rows, int m, const mfcd_pair_law *law, float *Q, int64_t ldq, float *deg,
                                      int64_t ldd, void *stream)
{
    LawArgs la;
    if (pair_args(A, Y, rows, m, 0.0, {lda, ldx, ldy, ldq, deg ? ldd : m}) || !X || hvp_args(A, X, Y, Q, deg) ||
        law_args(law, m, &la))
        return MFCD_EINVAL;
    const int T = pair_tiles(m);
    return pair_chunks(rows, pair_chunk_rows(rows, T), [&](int r0, int nr) {
        law_dispatch(la, law->use_margin != 0, [&](auto hw, auto hm, auto hl) {
            const auto kernel = deg ? pair_hvp_kernel<true, hw(), hm(), hl(), true> : pair_hvp_kernel<true, hw(), hm(), hl(), false>;
            hipLaunchKernelGGL(kernel, pair_grid(nr, T), dim3(kPairThreads), 0, (hipStream_t)stream, A + (int64_t)r0 * lda, lda,
                               X + (int64_t)r0 * ldx, ldx, Y + (int64_t)r0 * ldy, ldy, law_rows(la, r0), m, T,
                               Q + (int64_t)r0 * ldq, ldq, deg ? deg + (int64_t)r0 * ldd : nullptr, ldd);
        });
        return (int)hipGetLastError();
    });
}
