// rank_entries.hip — where given columns of a row of a score matrix stand among the row's admissible columns, in
// mfcd_topk_rows' `best` order, for every requested row at once (include/mfcd.h: mfcd_rank_entries).  What
// recall@k, NDCG@k, MRR and AUC over the full catalogue need of a model: the rank of every held-out entry, with the
// training items barred, without sorting a row and without forming anything n x m.
//
// No reference counterpart: the reference scores a model on sampled triplets only.
//
// Form built: PREPARE, then per slab of rows SLAB and COUNT.
//   prepare   rank_prepare_kernel, one workgroup per requested row, once per call: every offset, row id, target and barred
//             column of the row is checked before anything is gathered; status and admissible are written, and the row's
//             entries are set to what the counts are added to (rank 0, ties -1: the entry's own column is an equal key),
//             or to -1 where the entry's own column is barred or the row is invalid.
//   slab      factor mode: topk.hip's topk_scores_kernel (scores_common.h) writes the same bounded slab of whole score
//             rows; dense mode: the rows of X are the slab.
//   count     rank_count_kernel, one workgroup per (row, chunk of kRankChunk columns).  The chunk's ordered keys are staged
//             in LDS once (the column is the position, so a key is all that is kept), the row's barred columns that fall
//             into the chunk are overwritten by a key no score has, and the row's targets go through in tiles of 256: a
//             tile of nt targets gives each target a group of 256 / pow2ceil(nt) lanes, every lane of a group takes an
//             interleaved slice of the chunk (16-byte LDS reads) and keeps two integer counts — precedes, equal key — which
//             are added over the group (shuffles inside a wave, LDS integer atomics across waves) and then, one integer
//             atomic per (entry, chunk) with a non-zero count, to the outputs.
// Everything after the key is formed is integer, and integer addition commutes exactly: the outputs do not depend on the
// order in which chunks, tiles or lanes arrive, on the other rows, or on where a slab ends.
#include "common.h"
#include "scores_common.h"

namespace {

constexpr int kRankThreads = 256;
constexpr int kRankChunk = 4096;                // columns per workgroup: 16 KiB of keys in LDS
constexpr int kRankMaxTargets = 1 << 20;        // per row
constexpr int64_t kRankMaxBlocks = 1 << 30;     // (row, chunk) workgroups per launch
constexpr unsigned kAbsentKey = 0xFFFFFFFFu;    // ~sortable_key of the bit pattern 0xFFFFFFFF, a NaN: NaN has key 0, so no score has it

struct RankArgs {
    const float *S;                 // the slab, or X
    int64_t ld;
    int by_id;                      // the row's scores are row id(r) of S (dense mode), else row r - r0
    const int32_t *row_ids;
    int rows, n, m, chunks;
    const int64_t *tgt_off;
    const int32_t *tgt_items;
    int64_t entries;
    const int64_t *excl_off;
    const int32_t *excl_items;
    int64_t excl_entries;
    int32_t *rank, *ties;
    float *score;
    int32_t *admissible, *status;
};

// One workgroup per requested row.  Nothing is read through a value before that value is checked.
__global__ __launch_bounds__(kRankThreads) void rank_prepare_kernel(const RankArgs a)
{
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const int64_t tb = a.tgt_off[r], te = a.tgt_off[r + 1];
    const bool tgt_ok = tb >= 0 && te >= tb && te <= a.entries;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const bool excl_ok = eb >= 0 && ee >= eb && ee <= a.excl_entries;
    const int id = a.row_ids ? a.row_ids[r] : r;
    int bad = !tgt_ok || !excl_ok || id < 0 || id >= a.n || te - tb > kRankMaxTargets;
    if (!bad) {   // uniform
        for (int64_t p = tb + tid; p < te; p += kRankThreads) bad |= (int)((unsigned)a.tgt_items[p] >= (unsigned)a.m);
        for (int64_t p = eb + tid; p < ee; p += kRankThreads) {
            const int v = a.excl_items[p];
            bad |= (int)((unsigned)v >= (unsigned)a.m);
            if (p > eb) bad |= (int)(a.excl_items[p - 1] >= v);
        }
    }
    bad = __syncthreads_or(bad);
    if (tgt_ok) {
        for (int64_t p = tb + tid; p < te; p += kRankThreads) {
            const bool absent = bad || is_barred(a.excl_items, eb, ee, a.tgt_items[p]);
            a.rank[p] = absent ? -1 : 0;
            a.ties[p] = -1;
            if (a.score && bad) a.score[p] = __uint_as_float(0x7FC00000u);
        }
    }
    if (tid == 0) {
        a.status[r] = bad ? 2 : 0;
        a.admissible[r] = bad ? -1 : a.m - (int)(ee - eb);
    }
}

// One workgroup per (row r0 + blockIdx.x / chunks, chunk blockIdx.x % chunks) of a launch; rows the prepare kernel
// refused and rows without a target leave at once.
__global__ __launch_bounds__(kRankThreads) void rank_count_kernel(const RankArgs a, int r0)
{
    __shared__ __attribute__((aligned(16))) unsigned keys[kRankChunk];
    __shared__ unsigned tkey[kRankThreads];
    __shared__ int tcol[kRankThreads];           // the target's column, -1: barred
    __shared__ int acc[2][kRankThreads];
    const int tid = threadIdx.x;
    const int r = r0 + (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    if (a.status[r] != 0) return;
    const int64_t tb = a.tgt_off[r], T = a.tgt_off[r + 1] - tb;
    if (T == 0) return;
    const int id = a.row_ids ? a.row_ids[r] : r;
    const float *row = a.S + (int64_t)(a.by_id ? id : r - r0) * a.ld;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const int c0 = chunk * kRankChunk;
    const int len = min(kRankChunk, a.m - c0), quads = (len + 3) >> 2;

    for (int j = tid; j < 4 * quads; j += kRankThreads) keys[j] = j < len ? ordered_key(row[c0 + j], false) : kAbsentKey;
    __syncthreads();
    if (ee > eb) {   // the barred columns of [c0, c0 + len): from the first list entry >= c0 on
        int64_t lo = eb, hi = ee;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.excl_items[mid] < c0) lo = mid + 1;
            else hi = mid;
        }
        for (int64_t p = lo + tid; p < ee; p += kRankThreads) {
            const unsigned j = (unsigned)(a.excl_items[p] - c0);
            if (j >= (unsigned)len) break;   // ascending: the rest of this thread's entries lie beyond the chunk
            keys[j] = kAbsentKey;
        }
    }

    for (int64_t p0 = 0; p0 < T; p0 += kRankThreads) {
        const int nt = (int)min((int64_t)kRankThreads, T - p0);
        __syncthreads();                             // the keys are staged; the previous tile is done with tkey, tcol, acc
        if (tid < nt) {
            const int64_t e = tb + p0 + tid;
            const int c = a.tgt_items[e];
            const float s = row[c];
            tkey[tid] = ordered_key(s, false);
            tcol[tid] = is_barred(a.excl_items, eb, ee, c) ? -1 : c;
            if (chunk == 0 && a.score) a.score[e] = s;
        }
        acc[0][tid] = 0;
        acc[1][tid] = 0;
        __syncthreads();
        int shift = 8;                               // G = 256 / pow2ceil(nt) lanes per target
        while ((kRankThreads >> shift) < nt) --shift;
        const int G = 1 << shift, g = tid >> shift, l = tid & (G - 1);
        const int ct = g < nt ? tcol[g] : -1;
        const unsigned kt = g < nt ? tkey[g] : 0u;
        int before = 0, equal = 0;
        if (ct >= 0) {
            for (int q = l; q < quads; q += G) {
                const uint4 k = reinterpret_cast<const uint4 *>(keys)[q];
                const int c = c0 + 4 * q;
                before += (int)(k.x < kt || (k.x == kt && c < ct));
                before += (int)(k.y < kt || (k.y == kt && c + 1 < ct));
                before += (int)(k.z < kt || (k.z == kt && c + 2 < ct));
                before += (int)(k.w < kt || (k.w == kt && c + 3 < ct));
                equal += (int)(k.x == kt) + (int)(k.y == kt) + (int)(k.z == kt) + (int)(k.w == kt);
            }
        }
        for (int off = 1; off < G && off < MFCD_WAVE; off <<= 1) {   // the group's lanes of this wave
            before += __shfl_xor(before, off, MFCD_WAVE);
            equal += __shfl_xor(equal, off, MFCD_WAVE);
        }
        if (ct >= 0 && (l & (MFCD_WAVE - 1)) == 0) {                 // one lane per (group, wave)
            atomicAdd(&acc[0][g], before);
            atomicAdd(&acc[1][g], equal);
        }
        __syncthreads();
        if (tid < nt && tcol[tid] >= 0) {
            const int64_t e = tb + p0 + tid;
            if (acc[0][tid]) atomicAdd(&a.rank[e], acc[0][tid]);
            if (acc[1][tid]) atomicAdd(&a.ties[e], acc[1][tid]);
        }
    }
}

inline bool rank_sizes_ok(int rows, int m, int d, int64_t entries)
{
    return rows >= 0 && entries >= 0 && m >= 1 && m <= kTopkMaxM && d >= 0 && d <= MFCD_MAX_D;
}

inline size_t rank_slab_bytes(int rows, int m)
{
    const size_t bytes = align_up((size_t)slab_rows(rows, m) * (size_t)slab_ld(m) * 4);
    return bytes ? bytes : 256;   // rows = 0; 0 means "out of range"
}

// [p, p + pb) and [q, q + qb) share a byte, or start at the same address
inline bool rank_overlap(const void *p, size_t pb, const void *q, size_t qb)
{
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a == b || (a < b + qb && b < a + pb);
}

}  // namespace

extern "C" size_t mfcd_rank_entries_workspace_bytes(int rows, int m, int d, int64_t entries)
{
    if (!rank_sizes_ok(rows, m, d, entries) || d < 1) return 0;
    return rank_slab_bytes(rows, m);
}

extern "C" int mfcd_rank_entries(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids,
                                 int rows, int n, int m, const int64_t *tgt_off, const int32_t *tgt_items, int64_t entries,
                                 const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries, int32_t *rank,
                                 int32_t *ties, float *score, int32_t *admissible, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    const bool dense = X != nullptr;
    if (!dense && (!A || !B || d < 1)) return MFCD_EINVAL;
    if (!rank_sizes_ok(rows, m, dense ? 0 : d, entries) || n < 1 || excl_entries < 0) return MFCD_EINVAL;
    if (dense && ldx < m) return MFCD_EINVAL;
    if (!dense && ((int64_t)n * d >= ((int64_t)1 << 40) || (int64_t)m * d >= ((int64_t)1 << 40))) return MFCD_EINVAL;
    if (rows > 0 && (!tgt_off || !admissible || !status)) return MFCD_EINVAL;
    if (entries > 0 && (!tgt_items || !rank || !ties)) return MFCD_EINVAL;
    if ((excl_off == nullptr) != (excl_items == nullptr)) return MFCD_EINVAL;
    {
        const size_t eb = (size_t)entries * 4, rb = (size_t)rows * 4;
        const struct { const void *p; size_t bytes; } out[] = {{rank, eb}, {ties, eb}, {score, eb}, {admissible, rb}, {status, rb}},
            in[] = {{X, (size_t)n * (size_t)(dense ? ldx : 0) * 4}, {A, (size_t)n * d * 4}, {B, (size_t)m * d * 4},
                    {row_ids, rb}, {tgt_off, rb * 2 + 8}, {tgt_items, eb}, {excl_off, rb * 2 + 8},
                    {excl_items, (size_t)excl_entries * 4}, {workspace, dense ? 0 : rank_slab_bytes(rows, m)}};
        for (int i = 0; i < 5; ++i) {
            for (const auto &q : in)
                if (rank_overlap(out[i].p, out[i].bytes, q.p, q.bytes)) return MFCD_EINVAL;
            for (int j = 0; j < i; ++j)
                if (rank_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return MFCD_EINVAL;
        }
    }
    if (((uintptr_t)X | (uintptr_t)A | (uintptr_t)B | (uintptr_t)row_ids | (uintptr_t)tgt_items | (uintptr_t)excl_items |
         (uintptr_t)rank | (uintptr_t)ties | (uintptr_t)score | (uintptr_t)admissible | (uintptr_t)status) & 3)
        return MFCD_EALIGN;
    if (((uintptr_t)tgt_off | (uintptr_t)excl_off) & 7) return MFCD_EALIGN;
    if (!dense) {
        if (workspace && ((uintptr_t)workspace & 255)) return MFCD_EALIGN;
        if (!workspace || workspace_bytes < rank_slab_bytes(rows, m)) return MFCD_EWORKSPACE;
    }
    if (rows == 0) return 0;

    hipStream_t st = (hipStream_t)stream;
    RankArgs a;
    a.S = dense ? X : static_cast<const float *>(workspace);
    a.ld = dense ? ldx : slab_ld(m);
    a.by_id = dense ? 1 : 0;
    a.row_ids = row_ids; a.rows = rows; a.n = n; a.m = m; a.chunks = (m + kRankChunk - 1) / kRankChunk;
    a.tgt_off = tgt_off; a.tgt_items = tgt_items; a.entries = entries;
    a.excl_off = excl_off; a.excl_items = excl_items; a.excl_entries = excl_entries;
    a.rank = rank; a.ties = ties; a.score = score; a.admissible = admissible; a.status = status;
    hipLaunchKernelGGL(rank_prepare_kernel, dim3((unsigned)rows), dim3(kRankThreads), 0, st, a);
    MFCD_HIP_TRY(hipGetLastError());
    if (entries == 0) return 0;

    int rb = (int)(kRankMaxBlocks / a.chunks);           // >= 2^20 rows
    if (!dense) rb = min(rb, slab_rows(rows, m));
    for (int r0 = 0; r0 < rows; r0 += rb) {
        const int nb = rows - r0 < rb ? rows - r0 : rb;
        if (!dense) {
            hipLaunchKernelGGL(topk_scores_kernel, dim3((unsigned)((m + kBlk - 1) / kBlk), (unsigned)((nb + kBlk - 1) / kBlk)),
                               dim3(256), 0, st, A, B, row_ids ? row_ids + r0 : nullptr, r0, nb, n, m, d,
                               static_cast<float *>(workspace), a.ld);
            MFCD_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)((int64_t)nb * a.chunks)), dim3(kRankThreads), 0, st, a, r0);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return 0;
}
