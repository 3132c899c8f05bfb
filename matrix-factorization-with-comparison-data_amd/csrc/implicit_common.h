// What implicit.hip and implicit_hvp.hip share: the sizes of the two passes, the kernel arguments, the marking of a chunk's
// columns from the two ascending lists, the prepare kernel that validates a call's rows before anything is gathered, and
// the host rules for chunks, row blocks and overlapping arrays (DESIGN sections 3.17, 3.18).
#pragma once
#include <algorithm>

#include "common.h"
#include "scores_common.h"

namespace {

constexpr int kImpThreads = 256;
constexpr int kImpChunk = 2048;                 // columns per workgroup of the column pass, and per LDS stage of the positive pass
constexpr int kImpOwn = kImpChunk / kImpThreads;   // columns a thread of the column pass owns
constexpr int kImpTile = 256;                   // positives per LDS tile
constexpr int kImpMaxPos = 1 << 20;             // per row
constexpr int kImpMaxSlots = 16;                // positive-pass workgroups per row
constexpr int64_t kImpMaxBlocks = 1 << 20;      // (row, chunk) workgroups per launch: bounds the partials at 40 MiB
static_assert(kImpOwn * 8 == 64, "a flush of a thread's fp32 runs every 8 positives keeps them at 64 terms");

struct ImplicitPartial;                             // implicit.hip's per-(row, chunk) partial

struct ImplicitArgs {
    const float *S;                 // the slab, or X
    int64_t ld;
    int by_id;                      // the row's scores are row id(r) of S (dense mode), else row r - r0
    const int32_t *row_ids;
    int rows, n, m, chunks, slots;
    const int64_t *pos_off;
    const int32_t *pos_items;
    int64_t entries;
    const int64_t *excl_off;
    const int32_t *excl_items;
    int64_t excl_entries;
    const float *coef;
    int64_t *counts;                // null: not written (the Hessian-vector entry)
    double *sums;
    float *g;                       // the gradient rows, or the Hessian-vector entry's q
    int64_t ldg;
    int32_t *status;
    ImplicitPartial *part;          // [rows of a block][chunks]
    // the Hessian-vector entry only
    const float *SY;                // the direction: its slab, or Y, addressed as S is
    int64_t ldy;
    float *deg;                     // nullable
    int64_t ldd;
    int32_t *bad;                   // [rows of a block][chunks]: admissible columns whose score or direction is inf or NaN
};

// The first position of the ascending list items[lo, hi) whose value is >= c.
__device__ __forceinline__ int64_t implicit_lower(const int32_t *__restrict__ items, int64_t lo, int64_t hi, int c)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (items[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// cls[j] = what for the columns of [c0, c0 + len) that the ascending list items[lo, hi) names.  Every thread calls it.
__device__ __forceinline__ void implicit_mark(unsigned char *cls, int c0, int len, const int32_t *__restrict__ items,
                                              int64_t lo, int64_t hi, unsigned char what, int tid)
{
    if (hi <= lo) return;
    for (int64_t p = implicit_lower(items, lo, hi, c0) + tid; p < hi; p += kImpThreads) {
        const unsigned j = (unsigned)(items[p] - c0);
        if (j >= (unsigned)len) break;   // ascending: the rest of this thread's entries lie beyond the chunk
        cls[j] = what;
    }
}

// One workgroup per requested row.  Nothing is read through a value before that value is checked.  An invalid row gets
// its fills: counts -1, sum NaN, NaN rows of g and deg.
__global__ __launch_bounds__(kImpThreads) void implicit_prepare_kernel(const ImplicitArgs a)
{
    __shared__ int red[kImpThreads / MFCD_WAVE];
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const int64_t pb = a.pos_off[r], pe = a.pos_off[r + 1];
    const bool pos_ok = pb >= 0 && pe >= pb && pe <= a.entries;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const bool excl_ok = eb >= 0 && ee >= eb && ee <= a.excl_entries;
    const int id = a.row_ids ? a.row_ids[r] : r;
    int bad = !pos_ok || !excl_ok || id < 0 || id >= a.n || pe - pb > kImpMaxPos;
    if (!bad) {   // uniform
        for (int64_t p = pb + tid; p < pe; p += kImpThreads) {
            const int v = a.pos_items[p];
            bad |= (int)((unsigned)v >= (unsigned)a.m);
            if (p > pb) bad |= (int)(a.pos_items[p - 1] >= v);
        }
        for (int64_t p = eb + tid; p < ee; p += kImpThreads) {
            const int v = a.excl_items[p];
            bad |= (int)((unsigned)v >= (unsigned)a.m);
            if (p > eb) bad |= (int)(a.excl_items[p - 1] >= v);
        }
    }
    bad = __syncthreads_or(bad);
    int both = 0;                                    // positives that are barred: both lists are ascending and in range
    if (!bad)
        for (int64_t p = pb + tid; p < pe; p += kImpThreads) both += (int)is_barred(a.excl_items, eb, ee, a.pos_items[p]);
    both = wave_sum_xor(both);
    if ((tid & (MFCD_WAVE - 1)) == 0) red[tid >> 6] = both;
    __syncthreads();
    if (tid == 0) {
        both = 0;
        for (int w = 0; w < kImpThreads / MFCD_WAVE; ++w) both += red[w];
        const int64_t pos = (pe - pb) - both;
        a.status[r] = bad ? 2 : 0;
        if (a.counts) {
            a.counts[4 * (int64_t)r + 0] = bad ? -1 : pos;
            a.counts[4 * (int64_t)r + 1] = bad ? -1 : (int64_t)a.m - (ee - eb) - pos;
            a.counts[4 * (int64_t)r + 2] = bad ? -1 : 0;
            a.counts[4 * (int64_t)r + 3] = bad ? -1 : 0;
        }
        if (a.sums && bad) a.sums[r] = __longlong_as_double(0x7FF8000000000000ll);
    }
    if (bad && a.g)
        for (int j = tid; j < a.m; j += kImpThreads) a.g[(int64_t)r * a.ldg + j] = __uint_as_float(0x7FC00000u);
    if (bad && a.deg)
        for (int j = tid; j < a.m; j += kImpThreads) a.deg[(int64_t)r * a.ldd + j] = __uint_as_float(0x7FC00000u);
}

inline bool implicit_sizes_ok(int rows, int m, int d) { return rows >= 0 && m >= 1 && m <= kTopkMaxM && d >= 0 && d <= MFCD_MAX_D; }

inline int implicit_chunks(int m) { return (m + kImpChunk - 1) / kImpChunk; }

// rows per launch: at most kImpMaxBlocks (row, chunk) workgroups, and in factor mode the rows of one slab
inline int implicit_block_rows(int rows, int m, bool dense)
{
    int64_t rb = kImpMaxBlocks / implicit_chunks(m);   // >= 512
    if (!dense) rb = std::min<int64_t>(rb, slab_rows(rows, m));
    return (int)std::max<int64_t>(1, std::min<int64_t>(rb, rows));
}

inline size_t implicit_slab_bytes(int rows, int m, bool dense)
{
    return dense ? 0 : align_up((size_t)slab_rows(rows, m) * (size_t)slab_ld(m) * 4);
}

// [p, p + pb) and [q, q + qb) share a byte, or start at the same address
inline bool implicit_overlap(const void *p, size_t pb, const void *q, size_t qb)
{
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a == b || (a < b + qb && b < a + pb);
}

}  // namespace
