// What topk.hip and rank_entries.hip share: the ordered key of a score, the requested-row and barred-column lookups, and
// the factor mode's score slab — topk_scores_kernel and the rule that sizes the slab (DESIGN sections 3.8, 3.16).  Both
// entries compare the numbers this one kernel writes, so a column's position in mfcd_topk_rows' list and its rank from
// mfcd_rank_entries agree by construction.
#pragma once
#include "common.h"

namespace {

constexpr int kTopkMaxM = 1 << 22;
constexpr size_t kSlabBytes = (size_t)128 << 20;   // score slab of the factor mode (at least one block of 128 rows)
constexpr int kBlk = 128, kKC = 32, kLD = kKC + 1;  // score kernel: output block, factor columns per LDS stage, padded row

// ascending ordered key = output order of the end
__device__ __forceinline__ unsigned ordered_key(float f, bool worst)
{
    if (f != f) return worst ? 0xFFFFFFFFu : 0u;
    const unsigned s = sortable_key(f);
    return worst ? s : ~s;
}

// the id of requested row r, or -1 when it is not a row of the table
__device__ __forceinline__ int row_id_of(const int32_t *row_ids, int row_base, int r, int n)
{
    const int id = row_ids ? row_ids[r] : row_base + r;
    return id >= 0 && id < n ? id : -1;
}

// S[r][c] = A[id(r)] . B[c] for the `rows` requested rows of this slab (rows of S are `ld` floats apart).
__global__ __launch_bounds__(256) void topk_scores_kernel(const float *__restrict__ A, const float *__restrict__ B,
                                                          const int32_t *__restrict__ row_ids, int row_base, int rows,
                                                          int n, int m, int d, float *__restrict__ S, int64_t ld)
{
    __shared__ float As[kBlk * kLD], Bs[kBlk * kLD];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
    const int r0 = blockIdx.y * kBlk, c0 = blockIdx.x * kBlk;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    // loader: thread -> factor column lk of the stage, block rows lr + 8 i
    const int lk = tid & 31, lr = tid >> 5;
    int arow[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + lr + 8 * i;
        arow[i] = r < rows ? row_id_of(row_ids, row_base, r, n) : -1;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.0f;

    for (int k0 = 0; k0 < d; k0 += kKC) {
        const int kk = k0 + lk;
        const bool kok = kk < d;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = c0 + lr + 8 * i;
            As[(lr + 8 * i) * kLD + lk] = kok && arow[i] >= 0 ? A[(int64_t)arow[i] * d + kk] : 0.0f;
            Bs[(lr + 8 * i) * kLD + lk] = kok && c < m ? B[(int64_t)c * d + kk] : 0.0f;
        }
        __syncthreads();
        const int steps = (min(kKC, d - k0) + 1) >> 1;   // MFMA k index: step s, lane half h -> k0 + 2 s + h
        for (int s = 0; s < steps; ++s) {
            const float a0 = As[(wr + l31) * kLD + 2 * s + half], a1 = As[(wr + 32 + l31) * kLD + 2 * s + half];
            const float b0 = Bs[(wc + l31) * kLD + 2 * s + half], b1 = Bs[(wc + 32 + l31) * kLD + 2 * s + half];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int col = c0 + wc + 32 * tj + l31;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = r0 + wr + 32 * ti + tile_row(reg, half);
                if (r < rows && col < m) S[(int64_t)r * ld + col] = acc[ti][tj][reg];
            }
        }
}

// column c is in the ascending list items[lo, hi)
__device__ __forceinline__ bool is_barred(const int32_t *__restrict__ items, int64_t lo, int64_t hi, int c)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int v = items[mid];
        if (v == c) return true;
        if (v < c) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

inline int64_t slab_ld(int m) { return ((int64_t)m + 63) & ~(int64_t)63; }   // rows of the slab start on 256 bytes

// rows per slab: whole blocks of the score kernel, at most kSlabBytes (but at least one block)
inline int slab_rows(int rows, int m)
{
    const int64_t per = slab_ld(m) * 4;
    int64_t rb = (int64_t)(kSlabBytes / (size_t)per) / kBlk * kBlk;
    if (rb < kBlk) rb = kBlk;
    const int64_t need = ((int64_t)rows + kBlk - 1) / kBlk * kBlk;
    return (int)(rb < need ? rb : need);
}

}  // namespace
