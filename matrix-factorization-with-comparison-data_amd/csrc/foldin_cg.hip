// foldin_cg.hip — the exact block steps of the BTL fit for 1 <= d <= 256: the two convex problems of
// foldin.hip, solved by damped Newton whose step comes from conjugate gradients on Hessian-vector products.  The Hessian
//     H = sum_t w_t delta_t delta_t^T + l2 I,   w_t = p_t (1 - p_t),
// is never formed: it is applied as q = sum_t w_t (delta_t . p) delta_t + l2 p, 2 d fma per comparison instead of d^2,
// and what LDS holds is the row's delta_t, not a d x d factor.  include/mfcd.h states the algorithm and the stop rule
// (|g|_2 <= l2 gtol |u|_inf, which bounds the distance to the minimiser by strong convexity); tests/foldin_cg_model.py
// restates it in numpy.  The entries' host check, validation, staging, the scalar functions, the line search's rule and
// the epilogue are those of foldin.hip (foldin_common.h); the item policy is the same template parameter.
//
// One workgroup of 256 threads per row, no communication between workgroups, no atomics.  Thread k < d owns entry k of
// every d-vector: g, the Jacobi diagonal, and CG's r, s and M^-1 r live in its registers; u, s and the CG direction p
// are also in LDS because every thread reads them.
//
// A pass over the row takes its comparisons through the stage, R = mfcd_fold_in_cg_resident(d) at a time:
//   phase 1   L = min(64, pow2(d) / 4) lanes per comparison form delta_t . v: lane l takes k = l, l + L, ... in an fma
//             chain, then an xor butterfly inside the L lanes (fixed order, every lane ends with the same sum).  The
//             lanes turn the dot product into what the pass is for: x_t, w_t, p_t - z_t and the term of f (gradient
//             pass), a_t = w_t (delta_t . p) (Hessian-vector product), or delta_t . s (before the line search).
//   barrier
//   phase 2   thread k sums a_t delta_t[k] over the stage's comparisons, t ascending, into its register.
// A row of at most R comparisons is resident: it is staged once, and w_t, x_t and s . delta_t are in LDS too, so every
// CG iteration and every line-search trial reads LDS only.  A longer row is streamed: every pass gathers it again chunk
// by chunk (the chunk is R as well), and its w_t, x_t and s . delta_t are kept in the workspace, 8 bytes each per record.
// The path depends on the row's length and d only.  The line search needs no pass at all: x_t + t (s . delta_t) gives
// every trial point's logits.
//
// Barriers of one CG iteration on a resident row: p visible -> phase 1 -> a_t visible -> phase 2 and p . q -> update
// and (r . r, r . M^-1 r): four.  The sums over k are fixed-order: an xor butterfly in each wave, the four wave sums
// added as (w0 + w1) + (w2 + w3).
//
// LDS (doubles): the stage R x ld with ld = (d + 1) | 1 (odd: comparisons of different lane groups fall on different
// banks; column d holds c_t), R ld <= 8224; three d-vectors; four per-record arrays of R; 33 more.  d = 256: R = 32,
// 73 160 B; d = 128: R = 63, 70 304 B: two workgroups per CU in both.  Pipe: the f64 vector pipe (these are
// matrix-vector products; the matrix pipe has nothing to reuse).
#include <type_traits>

#include "foldin_common.h"

namespace {

constexpr int kCgMaxD = 256;
constexpr int kCgThreads = 256;
constexpr int kCgStageDoubles = 32 * 257;    // the stage: 32 comparisons at d = 256
constexpr double kCgEta = 1e-3;              // CG stops at |r|_2 <= eta |g|_2 ...
inline __host__ __device__ int cg_cap(int d) { return 4 * d + 50; }       // ... or after this many iterations

inline __host__ __device__ int cg_ld(int d) { return (d + 1) | 1; }
inline __host__ __device__ int cg_resident(int d)
{
    const int r = kCgStageDoubles / cg_ld(d);
    return r < kCgThreads ? r : kCgThreads;
}
inline size_t cg_lds_doubles(int d) { return (size_t)cg_resident(d) * cg_ld(d) + 3 * (size_t)d + 4 * (size_t)cg_resident(d) + 32 + 1; }

// Per-record f64 arrays of a streamed row, indexed as the records are (the workspace behind the item step's c_t).
struct FoldCgWork {
    double *w, *x, *sx;
    int64_t cap;               // records each array has room for: a row that ends beyond it is invalid
};

enum { kPassGrad, kPassHv, kPassSx };

template <bool ITEM>
__global__ __launch_bounds__(kCgThreads) void fold_cg_kernel(const float *__restrict__ V, int m, int d,
                                                             const mfcd_sample *__restrict__ rec,
                                                             const int64_t *__restrict__ row_off, double l2,
                                                             const float *__restrict__ U_init, int max_iter, double gtol,
                                                             float *__restrict__ U_out, double *__restrict__ objective,
                                                             int32_t *__restrict__ iters_status,
                                                             int32_t *__restrict__ cg_iters, const FoldItem item,
                                                             const FoldCgWork work)
{
    constexpr int NT = kCgThreads;
    extern __shared__ double cg_lds[];
    const int tid = threadIdx.x, r = blockIdx.x, lane = tid & (MFCD_WAVE - 1), wave = tid / MFCD_WAVE;
    const int ld = cg_ld(d), R = cg_resident(d);
    double *D = cg_lds, *u = D + R * ld, *s = u + d, *p = s + d, *a = p + d, *lw = a + R, *lx = lw + R, *lsx = lx + R;
    double *red = lsx + R;                             // [2][4 waves][4]
    int *flag = (int *)(red + 32);
    float *out = U_out + (int64_t)r * d;

    const int64_t b = row_off[r], e = row_off[r + 1];
    const int own = ITEM ? (item.row_item ? item.row_item[r] : r) : 0;      // the item this row solves
    if (cg_iters && tid == 0) cg_iters[r] = 0;
    if (!ITEM && e == b) {
        fold_empty_user_row<NT>(out, d, objective, iters_status, r, tid);
        return;
    }

    if (tid == 0) *flag = 0;
    __syncthreads();
    if constexpr (ITEM) {
        if (fold_item_row_is_bad<NT>(m, d, rec, b, e, own, item, tid)) *flag = 1;      // item.cap is work.cap
    } else {
        // the range first: no record of a row that starts below 0 or ends beyond the workspace is read
        if (b < 0 || e > work.cap || fold_user_row_is_bad<NT>(m, d, rec, b, e, U_init ? U_init + (int64_t)r * d : nullptr, tid))
            *flag = 1;
    }
    __syncthreads();
    if (*flag) {
        fold_invalid_row<NT, ITEM>(out, d, objective, iters_status, r, tid);
        return;
    }

    const bool owner = tid < d;
    double uk = 0.0;                                   // entry tid of the iterate
    if constexpr (ITEM) {
        const float *vold = item.V + (int64_t)own * d;
        if (e == b) {
            fold_empty_item_row<NT>(out, d, vold, item.theta, l2, objective, iters_status, r, tid);
            return;
        }
        if (fold_form_offsets<NT>(V, d, rec, b, e, own, item, tid)) *flag = 1;
        __syncthreads();                               // c_t is visible to the workgroup that wrote it
        if (*flag) {
            fold_invalid_row<NT, ITEM>(out, d, objective, iters_status, r, tid);
            return;
        }
        if (owner) uk = (double)vold[tid];
    } else {
        if (owner && U_init) uk = (double)U_init[(int64_t)r * d + tid];
    }
    if (owner) u[tid] = uk;

    const int n = (int)(e - b < (int64_t)R + 1 ? e - b : (int64_t)R + 1);      // only whether it exceeds R matters
    const bool resident = n <= R;
    double *pw = resident ? lw : work.w + b, *px = resident ? lx : work.x + b, *psx = resident ? lsx : work.sx + b;

    // staging geometry: P = the power of two >= d lanes per comparison, NT / P comparisons per sweep
    int lgp = 0;
    while ((1 << lgp) < d) ++lgp;
    const int sk = tid & ((1 << lgp) - 1), st0 = tid >> lgp, ststep = NT >> lgp;
    auto stage = [&](int64_t c0, int cn) {
        if (sk < d)
            for (int t = st0; t < cn; t += ststep) {
                const mfcd_sample q = rec[c0 + t];
                D[t * ld + sk] = fold_delta<ITEM>(V, d, q, own, sk, flag);
                if (sk == 0) D[t * ld + d] = ITEM ? item.c[c0 + t] : 0.0;
            }
    };
    // dot-product geometry: L lanes per comparison, NT / L comparisons per sweep
    int lgl = lgp > 2 ? lgp - 2 : 0;
    if (lgl > 6) lgl = 6;
    const int L = 1 << lgl, dl = tid & (L - 1), dg = tid >> lgl, G = NT >> lgl;

    // Sums over the workgroup, fixed order; the last of the NV values is a maximum when MAXLAST.  One barrier; the two
    // halves of red[] alternate, so a call's reads are over before the call after the next one writes.
    int par = 0;
    auto reduce = [&](auto nv, auto maxlast, double *v) {
        constexpr int NV = decltype(nv)::value;
        constexpr bool MAXLAST = decltype(maxlast)::value;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (MAXLAST && i == NV - 1) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v[i] = fmax(v[i], __shfl_xor(v[i], off, MFCD_WAVE));
            } else {
                v[i] = wave_sum_xor(v[i]);
            }
            if (lane == 0) red[par * 16 + wave * 4 + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double *q = red + par * 16 + i;
            v[i] = (MAXLAST && i == NV - 1) ? fmax(fmax(q[0], q[4]), fmax(q[8], q[12])) : (q[0] + q[4]) + (q[8] + q[12]);
        }
        par ^= 1;
    };
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    using three = std::integral_constant<int, 3>;
    using four = std::integral_constant<int, 4>;

    // One pass over the row with the d-vector v (in LDS).  kPassGrad: v = u; x_t, w_t are kept, acc0 = sum (p_t - z_t)
    // delta_t[k], acc1 = sum w_t delta_t[k]^2, facc = this thread's terms of f.  kPassHv: v = p; acc0 = sum w_t
    // (delta_t . p) delta_t[k].  kPassSx: s . delta_t is kept; no phase 2.
    auto pass = [&](auto mode_tag, const double *v, double &acc0, double &acc1, double &facc) {
        constexpr int MODE = decltype(mode_tag)::value;
        acc0 = acc1 = facc = 0.0;
        for (int64_t c0 = b; c0 < e; c0 += R) {
            const int cn = (int)(e - c0 < R ? e - c0 : R), base = (int)(c0 - b);
            if (!resident) {
                __syncthreads();                       // the previous chunk's readers are done
                stage(c0, cn);
            }
            __syncthreads();                           // the stage and v are visible
            for (int t0 = 0; t0 < cn; t0 += G) {       // phase 1: the same trip count for every lane
                const bool live = t0 + dg < cn;
                const int t = live ? t0 + dg : cn - 1;
                const double *row = D + t * ld;
                double dot = 0.0;
                for (int k = dl; k < d; k += L) dot = fma(v[k], row[k], dot);
                for (int off = L >> 1; off > 0; off >>= 1) dot += __shfl_xor(dot, off, MFCD_WAVE);
                if (live && dl == 0) {
                    if constexpr (MODE == kPassGrad) {
                        const FoldLogit at(row[d] + dot);
                        const double z = (double)rec[c0 + t].z;
                        facc += at.term(z);
                        px[base + t] = at.x;
                        pw[base + t] = at.weight();
                        a[t] = at.p() - z;
                    } else if constexpr (MODE == kPassHv) {
                        a[t] = pw[base + t] * dot;
                    } else {
                        psx[base + t] = dot;
                    }
                }
            }
            if constexpr (MODE != kPassSx) {
                __syncthreads();
                if (owner)                             // phase 2: t ascending
                    for (int t = 0; t < cn; ++t) {
                        const double dv = D[t * ld + tid];
                        acc0 = fma(a[t], dv, acc0);
                        if constexpr (MODE == kPassGrad) acc1 = fma(pw[base + t] * dv, dv, acc1);
                    }
            }
        }
    };

    if (resident) stage(b, n);                         // once; the first pass's barrier makes it visible

    const int cap = cg_cap(d);
    const int64_t len = e - b;
    int it = 0, status = 1, cg_total = 0;
    double fcur = 0.0, fstart = 0.0, gk, dk, unused;
    bool first = true;
    for (;;) {
        // ---- gradient pass at u: f, g, the Jacobi diagonal, |g|_2 and |u|_inf ----
        double facc;
        pass(std::integral_constant<int, kPassGrad>(), u, gk, dk, facc);
        gk = owner ? gk + l2 * uk : 0.0;
        double v4[4] = {facc, gk * gk, uk * uk, fabs(uk)};
        reduce(four(), std::true_type(), v4);
        fcur = v4[0] + 0.5 * l2 * v4[2];
        if (first) {
            first = false;
            fstart = fcur;
            if (*flag) {                               // a table row of this row holds an inf or a NaN
                fold_invalid_row<NT, ITEM>(out, d, objective, iters_status, r, tid);
                return;
            }
        }
        const double gnorm = sqrt(v4[1]);
        if (gnorm <= l2 * gtol * v4[3]) {              // certified: |u - u*|_2 <= |g|_2 / l2 <= gtol |u|_inf
            status = 0;
            break;
        }
        if (it >= max_iter) break;
        ++it;
        // ---- CG on H s = -g from s = 0, Jacobi-preconditioned ----
        const double minv = owner ? 1.0 / (dk + l2) : 0.0;
        double sown = 0.0, rk = -gk, zk = minv * rk, pk = zk;
        if (owner) p[tid] = pk;
        double rz = rk * zk;
        reduce(one(), std::false_type(), &rz);
        bool broke = false;
        for (int j = 0; j < cap; ++j) {
            double qk;
            pass(std::integral_constant<int, kPassHv>(), p, qk, unused, unused);
            qk = owner ? qk + l2 * pk : 0.0;
            double pq = pk * qk;
            reduce(one(), std::false_type(), &pq);
            if (!(pq > 0.0) || !(pq <= 1.7976931348623157e308)) {
                broke = true;
                break;
            }
            const double alpha = rz / pq;
            sown = fma(alpha, pk, sown);
            rk = fma(-alpha, qk, rk);
            ++cg_total;
            zk = minv * rk;
            double v2[2] = {rk * rk, rk * zk};
            reduce(two(), std::false_type(), v2);
            if (sqrt(v2[0]) <= kCgEta * gnorm) break;
            pk = fma(v2[1] / rz, pk, zk);
            rz = v2[1];
            if (owner) p[tid] = pk;                    // the next pass's barrier makes it visible
        }
        if (broke) break;                              // status 1: u is the last accepted iterate
        // ---- the line search on the CG iterate, which is a descent direction wherever CG stopped ----
        if (owner) s[tid] = sown;
        double v3[3] = {gk * sown, uk * sown, sown * sown};
        reduce(three(), std::false_type(), v3);
        const double gs = v3[0], us = v3[1], ss = v3[2];
        pass(std::integral_constant<int, kPassSx>(), s, unused, unused, unused);
        __syncthreads();                               // s . delta_t is visible
        // trial point u + t s: its logits are x_t + t (s . delta_t), so f there and the term-wise decrease need no pass
        double t = 1.0;
        bool accepted = false;
        for (int h = 0; h <= kFoldHalvings && !accepted; ++h) {
            double w3[3] = {0.0, 0.0, 0.0};
            for (int64_t i = tid; i < len; i += NT) {
                const FoldLogit at(px[i]);
                const double z = (double)rec[b + i].z, hs = t * psx[i];
                w3[0] += FoldLogit(at.x + hs).term(z);
                w3[1] += fold_decrease_term(at, hs, z);
            }
            const double un = fma(t, sown, uk);
            w3[2] = un * un;
            reduce(three(), std::false_type(), w3);
            const double decrease = w3[1] + l2 * (t * us + 0.5 * t * t * ss), fnew = w3[0] + 0.5 * l2 * w3[2];
            accepted = fold_armijo_accepts(decrease, fnew, fcur, t, gs);
            if (!accepted) t *= 0.5;
        }
        if (!accepted) break;                          // status 1
        uk = fma(t, sown, uk);
        if (owner) u[tid] = uk;                        // the gradient pass's barrier makes it visible
    }

    __syncthreads();
    fold_finish<NT, ITEM>(out, u, d, item, own, objective, iters_status, r, fstart, fcur, it, status, tid);
    if (cg_iters && tid == 0) cg_iters[r] = cg_total;
}

template <bool ITEM>
int fold_cg_launch(const float *V, int m, int d, const mfcd_sample *rec, const int64_t *row_off, int rows, double l2,
                   const float *U_init, int max_iter, double gtol, float *U_out, double *objective, int32_t *iters_status,
                   int32_t *cg_iters, const FoldItem &item, const FoldCgWork &work, hipStream_t st)
{
    const size_t lds = cg_lds_doubles(d) * sizeof(double);
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)fold_cg_kernel<ITEM>, lds, allowed));
    hipLaunchKernelGGL((fold_cg_kernel<ITEM>), dim3((unsigned)rows), dim3(kCgThreads), lds, st, V, m, d, rec, row_off, l2,
                       U_init, max_iter, gtol, U_out, objective, iters_status, cg_iters, item, work);
    return (int)hipGetLastError();
}

// the workspace behind its first 256 bytes: `arrays` f64 arrays of one length, as long as the bytes allow
inline int64_t cg_work_cap(size_t workspace_bytes, int arrays) { return (int64_t)((workspace_bytes - 256) / (sizeof(double) * arrays)); }

}  // namespace

extern "C" int mfcd_fold_in_cg_max_d(void) { return kCgMaxD; }

extern "C" int mfcd_fold_in_cg_resident(int d) { return d < 1 || d > kCgMaxD ? 0 : cg_resident(d); }

extern "C" int mfcd_fold_in_cg_chunk(int d) { return mfcd_fold_in_cg_resident(d); }    // a streamed row goes through the same stage

extern "C" size_t mfcd_fold_in_cg_workspace_bytes(int rows, int d, int64_t records)
{
    if (rows < 0 || d < 1 || d > kCgMaxD || records < 0 || records > (int64_t)1 << 56) return 0;
    return 256 + align_up(3 * sizeof(double) * (size_t)records);      // w_t, x_t and s . delta_t per record
}

extern "C" int mfcd_fold_in_users_cg(const float *V, int m, int d, const mfcd_sample *records, const int64_t *row_off,
                                     int rows, double l2, const float *U_init, int max_iter, double gtol, float *U_out,
                                     double *objective, int32_t *iters_status, int32_t *cg_iters, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    if (!V || m < 1) return MFCD_EINVAL;
    // the record count is on the device (row_off[rows]): the host requires the fixed part, and a row whose records end
    // beyond what the workspace holds is refused by its own workgroup (status 2)
    const int bad = fold_entry_check(d, kCgMaxD, row_off, rows, l2, max_iter, gtol, U_out, iters_status, V, m, U_init, rows,
                                     workspace, workspace_bytes, mfcd_fold_in_cg_workspace_bytes(rows, d, 0));
    if (bad || rows == 0) return bad;
    const int64_t cap = cg_work_cap(workspace_bytes, 3);
    double *base = (double *)((char *)workspace + 256);
    const FoldCgWork work{base, base + cap, base + 2 * cap, cap};
    return fold_cg_launch<false>(V, m, d, records, row_off, rows, l2, U_init, max_iter, gtol, U_out, objective,
                                 iters_status, cg_iters, FoldItem{}, work, (hipStream_t)stream);
}

extern "C" size_t mfcd_item_step_cg_workspace_bytes(int rows, int d, int64_t records)
{
    if (rows < 0 || d < 1 || d > kCgMaxD || records < 0 || records > (int64_t)1 << 56) return 0;
    return 256 + align_up(4 * sizeof(double) * (size_t)records);      // c_t, w_t, x_t and s . delta_t per record
}

extern "C" int mfcd_item_step_cg(const float *U, int n, const float *V, int m, int d, const mfcd_sample *records,
                                 const int64_t *row_off, const int32_t *row_item, int rows, double l2, double theta,
                                 int max_iter, double gtol, float *V_out, double *objective2, int32_t *iters_status,
                                 int32_t *cg_iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!U || !V || n < 1 || m < 1 || (!row_item && rows > m) || !(theta > 0.0 && theta <= 1.0)) return MFCD_EINVAL;
    const int bad = fold_entry_check(d, kCgMaxD, row_off, rows, l2, max_iter, gtol, V_out, iters_status, U, n, V, m,
                                     workspace, workspace_bytes, mfcd_item_step_cg_workspace_bytes(rows, d, 0));
    if (bad || rows == 0) return bad;
    const int64_t cap = cg_work_cap(workspace_bytes, 4);
    double *base = (double *)((char *)workspace + 256);
    const FoldItem item{V, m, row_item, theta, base, cap};
    const FoldCgWork work{base + cap, base + 2 * cap, base + 3 * cap, cap};
    return fold_cg_launch<true>(U, n, d, records, row_off, rows, l2, nullptr, max_iter, gtol, V_out, objective2,
                                iters_status, cg_iters, item, work, (hipStream_t)stream);
}
