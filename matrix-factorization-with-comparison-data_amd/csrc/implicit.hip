// implicit.hip — the exact observed-versus-unobserved logistic risk of rows of a score matrix (include/mfcd.h:
// mfcd_implicit_rows): for a requested row with observed columns P, barred columns E and
// N = [0, m) \ (P u E),
//   R = sum over i in P \ E, j in N of softplus(a_j - a_i),
// its gradient with respect to the score row, and the integer counts of the same pairs in mfcd_topk_rows' `best` order
// (how many pairs the row orders wrongly, how many it ties): BPR without the sampling, and the surrogate of the AUC that
// mfcd_rank_entries reports.  L (m - L) pairs per row, nothing n x m formed in factor mode.
//
// No reference counterpart: the reference trains on sampled triplets only.
//
// Form built: PREPARE, then per block of rows SLAB, COLUMNS, POSITIVES (gradient calls only) and FINISH.
//   prepare    implicit_prepare_kernel (implicit_common.h, shared with implicit_hvp.hip), one workgroup per requested row,
//              once per call: every offset, row id and item of both lists is checked before anything is gathered; status,
//              pos = |P \ E| and neg = |N| are written, and an invalid row gets its fills (counts -1, sum NaN, gradient
//              row NaN).  A call without `sums` ends here.
//   slab       factor mode: topk_scores_kernel (scores_common.h) writes the bounded slab of whole score rows that
//              mfcd_topk_rows and mfcd_rank_entries compare; dense mode: the rows of X are the slab.
//   columns    implicit_col_kernel, one workgroup per (row, chunk of kImpChunk columns).  The chunk's classes (negative,
//              positive, barred) are marked in LDS from the two ascending lists, as rank_count_kernel marks its barred
//              columns.  Every thread owns kImpChunk / 256 columns of the chunk, 256 apart; the row's admissible
//              positives stream through LDS in tiles of kImpTile.  A thread adds sigma(a_j - a_i) over the positives into
//              its own columns' sums and stores their g itself; the softplus sum and the two counts are reduced over
//              the workgroup (pair_block_sum) into one ImplicitPartial per (row, chunk).
//   positives  implicit_pos_kernel, one workgroup per (slot, row): slot s owns the row's tiles s, s + slots, ...  A tile of
//              nt positives gives each positive a group of 256 / pow2ceil(nt) lanes; the row's chunks are staged in LDS
//              one after the other (a column that is no negative as -inf: its term is exactly 0) and every lane of a
//              group takes an interleaved slice of 16-byte LDS reads.  The group's f64 sums combine in a fixed tree
//              (xor butterfly inside a wave, then the group's waves in index order) and the positive's owner stores g.
//   finish     implicit_finish_kernel, one workgroup per row: the chunks' partials in chunk order, the sum in natural
//              log, and the non-finite rule (sum NaN, gradient row NaN) when an admissible column is inf or NaN.
// Every float sum has one owner and a fixed order, no fp32 run is longer than 64 terms before it is added to an f64 sum,
// and there is no floating-point atomic: two calls are bit-equal, and a row's outputs do not depend on the other rows,
// on its place in the call, or on where a slab ends.  One exp per pair in a call without g, two in a call with it.
#include "implicit_common.h"
#include "pairs_common.h"

namespace {

struct ImplicitPartial {
    long long c[2];     // inverted, tied pairs of this chunk's negatives
    long long bad;      // admissible (not barred) columns of the chunk that are inf or NaN
    double s[2];        // sum of log2(1 + exp(-|v|)), sum of max(v, 0): ln 2 is applied once, in f64
};
static_assert(sizeof(ImplicitPartial) == 40, "workspace layout");

// One pair from one exp and one reciprocal: v = a_j - a_i → sigma(v) as pair_sigmoid forms it, and the two parts of
// softplus(v) = max(v, 0) + ln 2 * log2(1 + exp(-|v|)) as pair_term keeps them (log2 by v_log_f32, the linear part apart).
__device__ __forceinline__ void implicit_pair(float v, float &sig, float &l2, float &lin)
{
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(v));       // exp(-|v|) <= 1: v_exp_f32
    const float hi = __builtin_amdgcn_rcpf(1.0f + e);
    sig = v >= 0.0f ? hi : e * hi;
    l2 = __builtin_amdgcn_logf(1.0f + e);
    lin = fmaxf(v, 0.0f);
}

// One workgroup per (row r0 + blockIdx.x / chunks, chunk blockIdx.x % chunks) of a launch.
__global__ __launch_bounds__(kImpThreads) void implicit_col_kernel(const ImplicitArgs a, int r0)
{
    __shared__ unsigned char cls[kImpChunk];        // 0 negative, 1 positive, 2 barred
    __shared__ float pa[kImpTile];
    __shared__ unsigned pkey[kImpTile];
    __shared__ int pcol[kImpTile];                   // the positive's column, -1: barred
    const int tid = threadIdx.x;
    const int r = r0 + (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    if (a.status[r] != 0) return;
    const int64_t pb = a.pos_off[r], L = a.pos_off[r + 1] - pb;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const int id = a.row_ids ? a.row_ids[r] : r;
    const float *row = a.S + (int64_t)(a.by_id ? id : r - r0) * a.ld;
    const int c0 = chunk * kImpChunk;
    const int len = min(kImpChunk, a.m - c0);

    for (int j = tid; j < kImpChunk; j += kImpThreads) cls[j] = 0;
    __syncthreads();
    implicit_mark(cls, c0, len, a.pos_items, pb, pb + L, 1, tid);
    __syncthreads();                                 // a barred positive is barred
    implicit_mark(cls, c0, len, a.excl_items, eb, ee, 2, tid);
    __syncthreads();

    float aj[kImpOwn], run_g[kImpOwn];
    unsigned kj[kImpOwn];
    bool neg[kImpOwn];
    double acc_g[kImpOwn];
    long long bad = 0;
#pragma unroll
    for (int c = 0; c < kImpOwn; ++c) {
        const int j = tid + kImpThreads * c;
        const bool in = j < len;
        const float s = in && cls[j] != 2 ? row[c0 + j] : 0.0f;   // a barred column's score is never read
        neg[c] = in && cls[j] == 0;
        bad += (long long)(in && cls[j] != 2 && is_nonfinite_bits(s));
        kj[c] = ordered_key(s, false);
        aj[c] = neg[c] ? s : -INFINITY;              // every float term of such a column is exactly 0
        run_g[c] = 0.0f;
        acc_g[c] = 0.0;
    }
    unsigned inverted = 0, tied = 0;
    double s_l2 = 0.0, s_lin = 0.0;

    for (int64_t p0 = 0; p0 < L; p0 += kImpTile) {
        const int nt = (int)min((int64_t)kImpTile, L - p0);
        __syncthreads();                             // the previous tile is done with pa, pkey, pcol
        if (tid < nt) {
            const int c = a.pos_items[pb + p0 + tid];
            const bool barred = is_barred(a.excl_items, eb, ee, c);
            const float s = barred ? 0.0f : row[c];
            pa[tid] = s;
            pkey[tid] = ordered_key(s, false);
            pcol[tid] = barred ? -1 : c;
        }
        __syncthreads();
        for (int i0 = 0; i0 < nt; i0 += 8) {         // 8 positives x kImpOwn columns: one fp32 run of at most 64 terms
            float run_l2 = 0.0f, run_lin = 0.0f;
            const int i1 = min(i0 + 8, nt);
            for (int i = i0; i < i1; ++i) {
                const int ci = pcol[i];
                if (ci < 0) continue;                // uniform
                const float ai = pa[i];
                const unsigned ki = pkey[i];
#pragma unroll
                for (int c = 0; c < kImpOwn; ++c) {
                    float sig, l2, lin;
                    implicit_pair(aj[c] - ai, sig, l2, lin);
                    run_g[c] += sig;
                    run_l2 += l2;
                    run_lin += lin;
                    const int j = c0 + tid + kImpThreads * c;
                    inverted += (unsigned)(neg[c] && (kj[c] < ki || (kj[c] == ki && j < ci)));
                    tied += (unsigned)(neg[c] && kj[c] == ki);
                }
            }
            s_l2 += (double)run_l2;
            s_lin += (double)run_lin;
            if ((i0 & 63) == 56 || i1 == nt) {       // a column's run: at most 64 positives
#pragma unroll
                for (int c = 0; c < kImpOwn; ++c) {
                    acc_g[c] += (double)run_g[c];
                    run_g[c] = 0.0f;
                }
            }
        }
    }
    if (a.g) {
        const double cf = a.coef ? (double)a.coef[r] : 1.0;
#pragma unroll
        for (int c = 0; c < kImpOwn; ++c) {
            const int j = tid + kImpThreads * c;
            // negatives and barred columns; a positive's element is the positive pass's
            if (j < len && cls[j] != 1) a.g[(int64_t)r * a.ldg + c0 + j] = neg[c] ? (float)(cf * acc_g[c]) : 0.0f;
        }
    }
    long long cnt[3] = {(long long)inverted, (long long)tied, bad};
    double sm[2] = {s_l2, s_lin};
    ImplicitPartial *out = a.part + (int64_t)(r - r0) * a.chunks + chunk;
    pair_block_sum<kImpThreads / MFCD_WAVE>(tid, cnt, sm, [&](const long long (&ct)[3], const double (&st)[2]) {
        out->c[0] = ct[0];
        out->c[1] = ct[1];
        out->bad = ct[2];
        out->s[0] = st[0];
        out->s[1] = st[1];
    });
}

// One workgroup per (row r0 + blockIdx.x % nb, slot blockIdx.x / nb): the row's tiles slot, slot + slots, ...  The slot
// is the slow index: most rows fill slot 0 only, and consecutive workgroups go to different XCDs — with the slot as the
// fast index every working group of such a table lands on one XCD of the eight (measured: 8 times the time).
__global__ __launch_bounds__(kImpThreads) void implicit_pos_kernel(const ImplicitArgs a, int r0, int nb)
{
    __shared__ __attribute__((aligned(16))) float sc[kImpChunk];
    __shared__ unsigned char cls[kImpChunk];
    __shared__ float pa[kImpTile];
    __shared__ int pcol[kImpTile];
    __shared__ double red[kImpThreads];
    const int tid = threadIdx.x;
    const int r = r0 + (int)(blockIdx.x % (unsigned)nb), slot = (int)(blockIdx.x / (unsigned)nb);
    if (a.status[r] != 0) return;
    const int64_t pb = a.pos_off[r], L = a.pos_off[r + 1] - pb;
    if ((int64_t)slot * kImpTile >= L) return;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const int id = a.row_ids ? a.row_ids[r] : r;
    const float *row = a.S + (int64_t)(a.by_id ? id : r - r0) * a.ld;
    const double cf = a.coef ? (double)a.coef[r] : 1.0;

    for (int64_t p0 = (int64_t)slot * kImpTile; p0 < L; p0 += (int64_t)a.slots * kImpTile) {
        const int nt = (int)min((int64_t)kImpTile, L - p0);
        __syncthreads();                             // the previous tile is done with pa, pcol
        if (tid < nt) {
            const int c = a.pos_items[pb + p0 + tid];
            const bool barred = is_barred(a.excl_items, eb, ee, c);
            pa[tid] = barred ? 0.0f : row[c];
            pcol[tid] = barred ? -1 : c;
        }
        __syncthreads();
        int shift = 8;                               // G = 256 / pow2ceil(nt) lanes per positive
        while ((kImpThreads >> shift) < nt) --shift;
        const int G = 1 << shift, gi = tid >> shift, l = tid & (G - 1);
        const bool live = gi < nt && pcol[gi] >= 0;
        const float ai = live ? pa[gi] : 0.0f;
        double acc = 0.0;
        for (int chunk = 0; chunk < a.chunks; ++chunk) {
            const int c0 = chunk * kImpChunk;
            const int len = min(kImpChunk, a.m - c0), quads = (len + 3) >> 2;
            __syncthreads();                         // the previous chunk is done with sc, cls
            for (int j = tid; j < kImpChunk; j += kImpThreads) cls[j] = 0;
            __syncthreads();
            implicit_mark(cls, c0, len, a.pos_items, pb, pb + L, 1, tid);
            implicit_mark(cls, c0, len, a.excl_items, eb, ee, 1, tid);   // either list: no negative
            __syncthreads();
            for (int j = tid; j < 4 * quads; j += kImpThreads) sc[j] = j < len && cls[j] == 0 ? row[c0 + j] : -INFINITY;
            __syncthreads();
            if (live) {
                for (int q0 = l; q0 < quads; q0 += 16 * G) {   // 16 quads: one fp32 run of at most 64 terms
                    float run = 0.0f;
                    for (int q = q0; q < quads && q < q0 + 16 * G; q += G) {
                        const float4 s = reinterpret_cast<const float4 *>(sc)[q];
                        run += pair_sigmoid(s.x - ai);
                        run += pair_sigmoid(s.y - ai);
                        run += pair_sigmoid(s.z - ai);
                        run += pair_sigmoid(s.w - ai);
                    }
                    acc += (double)run;
                }
            }
        }
        const int sub = G < MFCD_WAVE ? G : MFCD_WAVE;   // the group's lanes of one wave, then its waves in index order
        for (int off = 1; off < sub; off <<= 1) acc += __shfl_xor(acc, off, MFCD_WAVE);
        __syncthreads();                             // the previous tile is done with red
        if ((tid & (sub - 1)) == 0) red[tid / sub] = acc;
        __syncthreads();
        if (tid < nt && pcol[tid] >= 0) {
            const int W = G / sub;
            double t = 0.0;
            for (int w = 0; w < W; ++w) t += red[tid * W + w];
            a.g[(int64_t)r * a.ldg + pcol[tid]] = (float)(-cf * t);
        }
    }
}

// One workgroup per row of a block: the chunks in order.
__global__ __launch_bounds__(kImpThreads) void implicit_finish_kernel(const ImplicitArgs a, int r0)
{
    const int tid = threadIdx.x;
    const int r = r0 + (int)blockIdx.x;
    if (a.status[r] != 0) return;
    const ImplicitPartial *p = a.part + (int64_t)blockIdx.x * a.chunks;
    int bad = 0;
    if (tid == 0) {
        long long c0 = 0, c1 = 0, nb = 0;
        double s0 = 0.0, s1 = 0.0;
        for (int k = 0; k < a.chunks; ++k) {
            c0 += p[k].c[0];
            c1 += p[k].c[1];
            nb += p[k].bad;
            s0 += p[k].s[0];
            s1 += p[k].s[1];
        }
        bad = nb != 0;
        a.counts[4 * (int64_t)r + 2] = c0;
        a.counts[4 * (int64_t)r + 3] = c1;
        a.sums[r] = bad ? __longlong_as_double(0x7FF8000000000000ll) : 0.6931471805599453 * s0 + s1;
    }
    bad = __syncthreads_or(bad);
    if (bad && a.g)
        for (int j = tid; j < a.m; j += kImpThreads) a.g[(int64_t)r * a.ldg + j] = __uint_as_float(0x7FC00000u);
}

inline size_t implicit_bytes(int rows, int m, bool dense)
{
    return implicit_slab_bytes(rows, m, dense) +
           align_up((size_t)implicit_block_rows(rows, m, dense) * (size_t)implicit_chunks(m) * sizeof(ImplicitPartial));
}

}  // namespace

extern "C" int mfcd_implicit_chunk(void) { return kImpChunk; }
extern "C" int mfcd_implicit_tile(void) { return kImpTile; }

extern "C" size_t mfcd_implicit_rows_workspace_bytes(int rows, int m, int d)
{
    if (!implicit_sizes_ok(rows, m, d)) return 0;
    return implicit_bytes(rows, m, d == 0);
}

extern "C" int mfcd_implicit_rows(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids,
                                  int rows, int n, int m, const int64_t *pos_off, const int32_t *pos_items, int64_t entries,
                                  const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries,
                                  const float *coef, int64_t *counts, double *sums, float *g, int64_t ldg, int32_t *status,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    const bool scored = sums != nullptr;             // without sums: the prepare pass alone, no scores are needed
    const bool dense = X != nullptr;
    if (!scored && g) return MFCD_EINVAL;
    if (scored && !dense && (!A || !B || d < 1)) return MFCD_EINVAL;
    if (!implicit_sizes_ok(rows, m, dense ? 0 : d) || entries < 0 || n < 1 || excl_entries < 0) return MFCD_EINVAL;
    if (dense && ldx < m) return MFCD_EINVAL;
    if (g && ldg < m) return MFCD_EINVAL;
    if (!dense && ((int64_t)n * d >= ((int64_t)1 << 40) || (int64_t)m * d >= ((int64_t)1 << 40))) return MFCD_EINVAL;
    if (rows > 0 && (!pos_off || !counts || !status)) return MFCD_EINVAL;
    if (entries > 0 && !pos_items) return MFCD_EINVAL;
    if ((excl_off == nullptr) != (excl_items == nullptr)) return MFCD_EINVAL;
    const size_t need = scored ? implicit_bytes(rows, m, dense) : 0;
    {
        const size_t rb = (size_t)rows * 4;
        const struct { const void *p; size_t bytes; } out[] = {{counts, rb * 8}, {sums, rb * 2}, {g, (size_t)rows * (size_t)ldg * 4},
                                                               {status, rb}, {workspace, need}},
            in[] = {{X, (size_t)n * (size_t)(dense ? ldx : 0) * 4}, {A, (size_t)n * d * 4}, {B, (size_t)m * d * 4}, {row_ids, rb},
                    {pos_off, rb * 2 + 8}, {pos_items, (size_t)entries * 4}, {excl_off, rb * 2 + 8},
                    {excl_items, (size_t)excl_entries * 4}, {coef, rb}};
        for (int i = 0; i < 5; ++i) {
            for (const auto &q : in)
                if (implicit_overlap(out[i].p, out[i].bytes, q.p, q.bytes)) return MFCD_EINVAL;
            for (int j = 0; j < i; ++j)
                if (implicit_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return MFCD_EINVAL;
        }
    }
    if (((uintptr_t)X | (uintptr_t)A | (uintptr_t)B | (uintptr_t)row_ids | (uintptr_t)pos_items | (uintptr_t)excl_items |
         (uintptr_t)coef | (uintptr_t)g | (uintptr_t)status) & 3)
        return MFCD_EALIGN;
    if (((uintptr_t)pos_off | (uintptr_t)excl_off | (uintptr_t)counts | (uintptr_t)sums) & 7) return MFCD_EALIGN;
    if (scored) {
        if (workspace && ((uintptr_t)workspace & 255)) return MFCD_EALIGN;
        if (!workspace || workspace_bytes < need) return MFCD_EWORKSPACE;
    }
    if (rows == 0) return 0;

    hipStream_t st = (hipStream_t)stream;
    ImplicitArgs a = {};
    a.S = dense ? X : static_cast<const float *>(workspace);
    a.ld = dense ? ldx : slab_ld(m);
    a.by_id = dense ? 1 : 0;
    a.row_ids = row_ids; a.rows = rows; a.n = n; a.m = m; a.chunks = implicit_chunks(m);
    a.slots = std::min((m + kImpTile - 1) / kImpTile, kImpMaxSlots);
    a.pos_off = pos_off; a.pos_items = pos_items; a.entries = entries;
    a.excl_off = excl_off; a.excl_items = excl_items; a.excl_entries = excl_entries;
    a.coef = coef; a.counts = counts; a.sums = sums; a.g = g; a.ldg = ldg; a.status = status;
    a.part = scored ? reinterpret_cast<ImplicitPartial *>(static_cast<char *>(workspace) + implicit_slab_bytes(rows, m, dense))
                    : nullptr;
    hipLaunchKernelGGL(implicit_prepare_kernel, dim3((unsigned)rows), dim3(kImpThreads), 0, st, a);
    MFCD_HIP_TRY(hipGetLastError());
    if (!scored) return 0;

    const int rb = implicit_block_rows(rows, m, dense);
    for (int r0 = 0; r0 < rows; r0 += rb) {
        const int nb = rows - r0 < rb ? rows - r0 : rb;
        if (!dense) {
            hipLaunchKernelGGL(topk_scores_kernel, dim3((unsigned)((m + kBlk - 1) / kBlk), (unsigned)((nb + kBlk - 1) / kBlk)),
                               dim3(256), 0, st, A, B, row_ids ? row_ids + r0 : nullptr, r0, nb, n, m, d,
                               static_cast<float *>(workspace), a.ld);
            MFCD_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(implicit_col_kernel, dim3((unsigned)((int64_t)nb * a.chunks)), dim3(kImpThreads), 0, st, a, r0);
        MFCD_HIP_TRY(hipGetLastError());
        if (g) {
            hipLaunchKernelGGL(implicit_pos_kernel, dim3((unsigned)((int64_t)nb * a.slots)), dim3(kImpThreads), 0, st, a, r0, nb);
            MFCD_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(implicit_finish_kernel, dim3((unsigned)nb), dim3(kImpThreads), 0, st, a, r0);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return 0;
}
