// topk.hip — the k best / k worst columns of every requested row of a score matrix on gfx950, the matrix given
// either dense (X [n][ldx] fp32) or as factors (score(r, c) = A[r] . B[c], fp32), without forming anything n x m.
//
// No reference counterpart as a function: the reference calls torch.topk(row, k) per attempt inside its samplers
// (generation_data.py:29-43 "Min-Max", 189-224 "top_10%"); the device law and the bulk host forms need the same
// lists for many rows at once, and the recommendation extensions of structure.py need them for U V^T.
//
// Form built: SLAB, then SELECT.
//   factor mode   topk_scores_kernel (scores_common.h, shared with rank_entries.hip) writes a bounded slab of score rows (at most kSlabBytes, whole rows) into the
//                 caller's workspace: 128 x 128 output block per workgroup, four waves of 2 x 2 tiles on the exact
//                 fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, the same for every element), operands
//                 staged through LDS 32 factor columns at a time, any d.  Each score is computed ONCE, so selection
//                 and emission see the same value by construction.
//   dense mode    the rows of X are the slab.
//   selection     topk_select_kernel<IPT>, one workgroup per (row, end): the row is read once and its ordered 32-bit
//                 keys stay in registers (rows of up to 32768 columns; longer ones are re-read per pass).  (key, column)
//                 composites are unique, so "the k smallest composites" has no ties to break: a radix select over
//                 them (digits of 11 + 11 + 10 key bits, then 11 + 11 column bits, histograms in LDS) stops at the
//                 first level whose bin is wanted whole, every composite at or below that bin is appended to the
//                 candidate list (exactly k, any order), and a bitonic sort of the <= 8192 composites in LDS puts
//                 them in final order.  The result does not depend on the order of the appends.
// Ordered key: best = ~sortable(x), worst = sortable(x) with common.h's sortable_key (-0.0 == +0.0), NaN -> the
// smallest key for best (torch.topk's convention), the largest for worst; equal keys are ordered by column.
#include "common.h"
#include "scores_common.h"

namespace {

constexpr int kTopkThreads = 1024;
constexpr int kTopkWaves = kTopkThreads / MFCD_WAVE;
constexpr int kTopkMaxK = 8192;                 // (key, column) pairs of one row that are sorted in LDS: 64 KiB
constexpr int kBins = 2048;                     // histogram of the widest radix digit (11 bits)

// inclusive sum of v over the workgroup's threads in thread order; total = the sum over all of them
__device__ __forceinline__ int block_scan_incl(int v, int *wtot, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < MFCD_WAVE; off <<= 1) {
        const int t = __shfl_up(v, off, MFCD_WAVE);
        if (lane >= off) v += t;
    }
    __syncthreads();                               // wtot[] may still be read from the previous use
    if (lane == MFCD_WAVE - 1) wtot[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kTopkWaves; ++w) {
        const int t = wtot[w];
        all += t;
        if (w < wave) before += t;
    }
    total = all;
    return v + before;
}

struct TopkOut {
    int32_t *idx[2];   // [rows][k]: 0 best, 1 worst
    float *val[2];     // nullable
};

// The five digits of the 64-bit composite (ordered key << 32 | column), from the top: key bits 31..21, 20..10, 9..0,
// column bits 21..11 (columns are below 2^22) and 10..0.
__device__ __forceinline__ int level_shift(int L) { return L == 0 ? 53 : L == 1 ? 42 : L == 2 ? 32 : L == 3 ? 11 : 0; }
__device__ __forceinline__ int level_width(int L) { return L == 2 ? 10 : L == 3 ? 21 : 11; }   // level_shift(L - 1) - level_shift(L)
__device__ __forceinline__ unsigned level_mask(int L) { return L == 2 ? 0x3FFu : 0x7FFu; }

// One workgroup per (requested row, end).  by_id: the row's scores are row id(r) of S (dense mode); else row r of S
// (the slab).  `ends`: 1 best, 2 worst, 3 both (blockIdx.y = 0 best, 1 worst).  P: power of two >= k, the sort size.
// IPT > 0: the row (m <= IPT * 1024 columns) is read ONCE, every load in flight together, and its ordered keys stay in
// registers (thread t holds columns j * 1024 + t) for all passes; a pass that re-read the row was a chain of
// memory round trips per 1024 columns.  IPT == 0: rows of any length, re-read by every pass (from L2, mostly),
// sixteen loads per thread in flight.
// Selection: a radix select over the composites (unique per column, so "the k smallest" has no ties left to break):
// per level a histogram of the digit in LDS among the elements that match the digits fixed so far, a scan that finds
// the bin holding the k-th, until a bin is wanted WHOLE (at the latest on the last level, where a bin is one element).
// Then every composite at or below that bin is appended to the candidate list (exactly k of them, any order) and a
// bitonic sort in LDS puts them in final order.
template <int IPT>
__global__ __launch_bounds__(kTopkThreads) void topk_select_kernel(const float *__restrict__ S, int64_t ld, int by_id,
                                                                   const int32_t *__restrict__ row_ids, int row_base,
                                                                   int n, int m, int k, int P, int ends,
                                                                   const int64_t *__restrict__ excl_off,
                                                                   const int32_t *__restrict__ excl_items, TopkOut out)
{
    typedef unsigned long long u64;
    extern __shared__ __attribute__((aligned(16))) unsigned long long cand[];   // [P]
    __shared__ unsigned hist[kBins];
    __shared__ int wtot[kTopkWaves];
    __shared__ int sh_bin, sh_below, sh_count;
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const bool worst = ends == 3 ? blockIdx.y == 1 : ends == 2;
    int32_t *oidx = out.idx[worst] + (int64_t)r * k;
    float *oval = out.val[worst] ? out.val[worst] + (int64_t)r * k : nullptr;
    const float qnan = __uint_as_float(0x7FC00000u);
    const int id = row_id_of(row_ids, row_base, r, n);
    if (id < 0) {   // not a row of the table: an empty result
        for (int p = tid; p < k; p += kTopkThreads) {
            oidx[p] = -1;
            if (oval) oval[p] = qnan;
        }
        return;
    }
    const float *row = S + (int64_t)(by_id ? id : r) * ld;
    const int64_t e_lo = excl_off ? excl_off[r] : 0, e_hi = excl_off ? excl_off[r + 1] : 0;
    const bool has_excl = e_hi > e_lo;

    unsigned key[IPT > 0 ? IPT : 1];
    u64 live = 0;   // bit j: column j * 1024 + tid exists and is not barred
    if constexpr (IPT > 0) {
        constexpr int LB = IPT < 16 ? IPT : 16;   // loads in flight together (all of them at once would not fit the registers)
#pragma unroll
        for (int j0 = 0; j0 < IPT; j0 += LB) {
            float x[LB];
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) x[jj] = row[min((j0 + jj) * kTopkThreads + tid, m - 1)];
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) {
                const int c = (j0 + jj) * kTopkThreads + tid;
                key[j0 + jj] = ordered_key(x[jj], worst);
                if (c < m && !(has_excl && is_barred(excl_items, e_lo, e_hi, c))) live |= 1ull << (j0 + jj);
            }
            asm volatile("" ::: "memory");
        }
    }
    // f(composite) for every column of the row that is not barred
    auto visit = [&](auto f) __attribute__((always_inline)) {
        if constexpr (IPT > 0) {
            // opaque copies: otherwise the column numbers and live bits of all IPT elements are hoisted out of the level
            // loop as loop invariants, two more registers per element
            int t = tid;
            u64 lv = live;
            asm volatile("" : "+v"(t), "+v"(lv));
#pragma unroll
            for (int j = 0; j < IPT; ++j)
            {
                if ((lv >> j) & 1ull) f(((u64)key[j] << 32) | (unsigned)(j * kTopkThreads + t));
                asm volatile("" ::: "memory");   // one element at a time: IPT interleaved iterations cost registers
            }
        } else {
            for (int c0 = 0; c0 < m; c0 += 16 * kTopkThreads) {   // 16 loads in flight, then their elements
                float x[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = row[min(c0 + j * kTopkThreads + tid, m - 1)];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = c0 + j * kTopkThreads + tid;
                    if (c < m && !(has_excl && is_barred(excl_items, e_lo, e_hi, c)))
                        f(((u64)ordered_key(x[j], worst) << 32) | (unsigned)c);
                }
            }
        }
    };

    // ---- radix select over the composites ----
    u64 prefix = 0;   // the digits fixed so far = composite >> fshift of the k-th element
    int fshift = 64, krem = k, keff = k;
    for (int L = 0; L < 5; ++L) {
        const int shift = level_shift(L);
        const unsigned mask = level_mask(L);
        for (int b = tid; b < kBins; b += kTopkThreads) hist[b] = 0u;
        __syncthreads();
        const int up = fshift;
        visit([&](u64 v) {
            if (L == 0 || (v >> up) == prefix) atomicAdd(&hist[(unsigned)(v >> shift) & mask], 1u);
        });
        __syncthreads();
        const int h0 = (int)hist[2 * tid], h1 = (int)hist[2 * tid + 1];
        int total;
        const int incl = block_scan_incl(h0 + h1, wtot, total);
        if (L == 0) {   // total = columns that are not barred
            keff = min(k, total);
            krem = keff;
            if (keff == 0) break;
        }
        const int excl = incl - (h0 + h1);
        if (excl < krem && krem <= incl) {   // exactly one thread: the k-th element is in one of its two bins
            const bool first = krem <= excl + h0;
            sh_bin = 2 * tid + (first ? 0 : 1);
            sh_below = excl + (first ? 0 : h0);
        }
        __syncthreads();
        const int bin = sh_bin;
        const int in_bin = (int)hist[bin];
        prefix = (prefix << level_width(L)) | (u64)(unsigned)bin;
        krem -= sh_below;
        fshift = shift;
        __syncthreads();
        if (in_bin == krem) break;   // the whole bin is wanted (always so on the last level: one element per bin)
    }
    if (keff == 0) {   // every column is barred (uniform over the workgroup)
        for (int p = tid; p < k; p += kTopkThreads) {
            oidx[p] = -1;
            if (oval) oval[p] = qnan;
        }
        return;
    }

    // ---- gather: exactly keff composites are at or below the bin ----
    if (tid == 0) sh_count = 0;
    for (int p = keff + tid; p < P; p += kTopkThreads) cand[p] = ~0ull;   // padding sorts last
    __syncthreads();
    visit([&](u64 v) {
        if ((v >> fshift) <= prefix) {
            const int p = atomicAdd(&sh_count, 1);
            if (p < P) cand[p] = v;
        }
    });
    __syncthreads();

    // ---- bitonic sort of cand[0, P), ascending ----
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += kTopkThreads) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const unsigned long long a = cand[lo], b = cand[hi];
                if ((a > b) == asc) {
                    cand[lo] = b;
                    cand[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int p = tid; p < k; p += kTopkThreads) {
        if (p < keff) {
            const int c = (int)(unsigned)(cand[p] & 0xFFFFFFFFull);
            oidx[p] = c;
            if (oval) oval[p] = row[c];   // the value that was compared
        } else {                          // fewer than k columns remain
            oidx[p] = -1;
            if (oval) oval[p] = qnan;
        }
    }
}

struct SelectArgs {
    const float *S;
    int64_t ld;
    int by_id;
    const int32_t *row_ids;
    int row_base, n, m, k, P, ends;
    const int64_t *excl_off;
    const int32_t *excl_items;
    TopkOut out;
};

template <int IPT>
int launch_select(const SelectArgs &a, int rows, hipStream_t st)
{
    const size_t lds = (size_t)a.P * 8;
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)topk_select_kernel<IPT>, lds, allowed));
    hipLaunchKernelGGL(topk_select_kernel<IPT>, dim3((unsigned)rows, a.ends == 3 ? 2u : 1u), dim3(kTopkThreads), lds, st, a.S,
                       a.ld, a.by_id, a.row_ids, a.row_base, a.n, a.m, a.k, a.P, a.ends, a.excl_off, a.excl_items, a.out);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

// registers per thread for the row: the smallest instantiation that holds m columns
int select_rows(const SelectArgs &a, int rows, hipStream_t st)
{
    const int m = a.m;
    return m <= 4 * kTopkThreads ? launch_select<4>(a, rows, st)
         : m <= 16 * kTopkThreads ? launch_select<16>(a, rows, st)
         : m <= 32 * kTopkThreads ? launch_select<32>(a, rows, st)
         : launch_select<0>(a, rows, st);   // (64 keys per thread do not fit 128 registers without scratch)
}

inline bool topk_sizes_ok(int rows, int m, int d, int k, int ends)
{
    return rows >= 1 && m >= 1 && m <= kTopkMaxM && d >= 0 && d <= MFCD_MAX_D && k >= 1 && k <= kTopkMaxK && k <= m &&
           ends >= 1 && ends <= 3;
}

}  // namespace

extern "C" int mfcd_topk_max_k(void) { return kTopkMaxK; }

extern "C" size_t mfcd_topk_rows_workspace_bytes(int rows, int m, int d, int k, int ends)
{
    if (!topk_sizes_ok(rows, m, d, k, ends)) return 0;
    if (d == 0) return 256;   // dense mode: the rows of X are read in place
    return align_up((size_t)slab_rows(rows, m) * (size_t)slab_ld(m) * 4);
}

extern "C" int mfcd_topk_rows(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids,
                              int rows, int n, int m, int k, int ends, const int64_t *excl_off,
                              const int32_t *excl_items, int32_t *best_idx, float *best_val, int32_t *worst_idx,
                              float *worst_val, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool dense = X != nullptr;
    if (!dense && (!A || !B || d < 1)) return MFCD_EINVAL;
    if (!topk_sizes_ok(rows, m, dense ? 0 : d, k, ends) || n < 1) return MFCD_EINVAL;
    if (dense && ldx < m) return MFCD_EINVAL;
    if (!dense && ((int64_t)n * d >= ((int64_t)1 << 40) || (int64_t)m * d >= ((int64_t)1 << 40))) return MFCD_EINVAL;
    if (((ends & 1) && !best_idx) || ((ends & 2) && !worst_idx)) return MFCD_EINVAL;
    if (excl_off && !excl_items) return MFCD_EINVAL;
    if (((uintptr_t)X | (uintptr_t)A | (uintptr_t)B | (uintptr_t)best_idx | (uintptr_t)worst_idx | (uintptr_t)best_val |
         (uintptr_t)worst_val | (uintptr_t)row_ids | (uintptr_t)excl_items) & 3)
        return MFCD_EALIGN;
    if ((uintptr_t)excl_off & 7) return MFCD_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    SelectArgs sa;
    sa.n = n; sa.m = m; sa.k = k; sa.ends = ends; sa.excl_items = excl_items;
    sa.P = 1;
    while (sa.P < k) sa.P <<= 1;
    if (dense) {
        sa.S = X; sa.ld = ldx; sa.by_id = 1; sa.row_ids = row_ids; sa.row_base = 0; sa.excl_off = excl_off;
        sa.out.idx[0] = best_idx; sa.out.idx[1] = worst_idx; sa.out.val[0] = best_val; sa.out.val[1] = worst_val;
        return select_rows(sa, rows, st);
    }
    const int rb = slab_rows(rows, m);
    const int64_t ld = slab_ld(m);
    if (!workspace || ((uintptr_t)workspace & 255)) return workspace ? MFCD_EALIGN : MFCD_EWORKSPACE;
    if (workspace_bytes < align_up((size_t)rb * (size_t)ld * 4)) return MFCD_EWORKSPACE;
    float *S = static_cast<float *>(workspace);
    sa.S = S; sa.ld = ld; sa.by_id = 0;
    for (int r0 = 0; r0 < rows; r0 += rb) {
        const int nb = rows - r0 < rb ? rows - r0 : rb;
        const int32_t *ids = row_ids ? row_ids + r0 : nullptr;
        hipLaunchKernelGGL(topk_scores_kernel, dim3((unsigned)((m + kBlk - 1) / kBlk), (unsigned)((nb + kBlk - 1) / kBlk)),
                           dim3(256), 0, st, A, B, ids, r0, nb, n, m, d, S, ld);
        MFCD_HIP_TRY(hipGetLastError());
        const int64_t o = (int64_t)r0 * k;
        sa.row_ids = ids; sa.row_base = r0; sa.excl_off = excl_off ? excl_off + r0 : nullptr;
        sa.out.idx[0] = best_idx ? best_idx + o : nullptr;
        sa.out.idx[1] = worst_idx ? worst_idx + o : nullptr;
        sa.out.val[0] = best_val ? best_val + o : nullptr;
        sa.out.val[1] = worst_val ? worst_val + o : nullptr;
        const int rc = select_rows(sa, nb, st);
        if (rc) return rc;
    }
    return 0;
}
