// foldin_common.h — what the per-row Newton kernels share.  All three (foldin.hip, foldin_cg.hip,
// ratings_foldin.hip): the line search's acceptance rule and constant, fold_overlap.  fold_cholesky_solve, the dense SPD
// solve in LDS: foldin.hip calls it, ratings_foldin.hip keeps the same steps written out because the call measured
// slower there (profiles/fold_family_refactor.txt); a new solver of this family calls it.  The two triplet kernels: the
// host check of their four entries, the item policy's launch block, row validation, the NaN row, the empty rows, the
// prologue that forms c_t, the staging rule, the per-comparison scalar functions and the epilogue.  Every device
// function is called by all threads of the row's workgroup (NT of them) unless it says otherwise.
#pragma once
#include <cmath>

#include "common.h"

namespace {

constexpr int kFoldHalvings = 30;
constexpr double kFoldArmijo = 1e-4;                   // population.ARMIJO

// What the item step adds to a launch; the user step passes an empty one and never reads it.
struct FoldItem {
    const float *V;            // the item table [m][d]: the start rows and the partner rows of c_t
    int m;
    const int32_t *row_item;   // nullable: row r solves item r
    double theta;
    double *c;                 // c_t per record, indexed as the records are; written and read by the row's workgroup only
    int64_t cap;               // records the workspace has room for: a row that ends beyond it is invalid
};

inline bool fold_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// l2, the iteration cap and the stop tolerance (xtol or gtol) of a triplet entry
inline bool fold_scalars_ok(double l2, int max_iter, double tol)
{
    return std::isfinite(l2) && l2 > 0.0 && max_iter >= 1 && max_iter <= 1000 && std::isfinite(tol) && tol >= 0.0;
}

// The host check the four triplet entries share: the common arguments, the output [rows][d] against the two float tables
// read ([n0][d], [n1][d]; a null one is skipped), the workspace.  0: the caller launches unless rows == 0.
inline int fold_entry_check(int d, int max_d, const int64_t *row_off, int rows, double l2, int max_iter, double tol,
                            const float *out, const int32_t *iters_status, const float *in0, int n0, const float *in1,
                            int n1, const void *workspace, size_t workspace_bytes, size_t needed)
{
    if (!row_off || !out || !iters_status || d < 1 || d > max_d || rows < 0 || !fold_scalars_ok(l2, max_iter, tol))
        return MFCD_EINVAL;
    const size_t row_bytes = (size_t)d * sizeof(float), out_bytes = (size_t)rows * row_bytes;
    if ((in0 && (out == in0 || fold_overlap(out, out_bytes, in0, (size_t)n0 * row_bytes))) ||
        (in1 && (out == in1 || fold_overlap(out, out_bytes, in1, (size_t)n1 * row_bytes))))
        return MFCD_EINVAL;
    if (rows == 0) return 0;
    return !workspace ? MFCD_EINVAL : workspace_bytes < needed ? MFCD_EWORKSPACE : 0;
}

// ---- validation: indices and labels before any gather, the start vector; table rows are checked as they are staged ----
// User step: V [m][d] is the gathered table, start the row's U_init (nullable).  Returns this thread's verdict.
template <int NT>
__device__ __forceinline__ bool fold_user_row_is_bad(int m, int d, const mfcd_sample *__restrict__ rec, int64_t b, int64_t e,
                                                     const float *__restrict__ start, int tid)
{
    bool bad = e < b || rec == nullptr;
    if (!bad)
        for (int64_t t = b + tid; t < e; t += NT) {
            const mfcd_sample q = rec[t];
            if ((unsigned)q.i >= (unsigned)m || (unsigned)q.j >= (unsigned)m || !(q.z >= 0.0f && q.z <= 1.0f)) bad = true;
        }
    if (start)
        for (int k = tid; k < d; k += NT)
            if (is_nonfinite_bits(start[k])) bad = true;
    return bad;
}

// Item step: the row's own item first, then every index of its records (n users), that each record holds the item, the
// labels, and that the row's c_t fit into the workspace.
template <int NT>
__device__ __forceinline__ bool fold_item_row_is_bad(int n, int d, const mfcd_sample *__restrict__ rec, int64_t b, int64_t e,
                                                     int own, const FoldItem &item, int tid)
{
    bool bad = (unsigned)own >= (unsigned)item.m || e < b || b < 0 || e > item.cap || (e > b && rec == nullptr);
    if (!bad) {
        for (int64_t t = b + tid; t < e; t += NT) {
            const mfcd_sample q = rec[t];
            if ((unsigned)q.u >= (unsigned)n || (unsigned)q.i >= (unsigned)item.m || (unsigned)q.j >= (unsigned)item.m ||
                (q.i != own && q.j != own) || !(q.z >= 0.0f && q.z <= 1.0f))
                bad = true;
        }
        for (int k = tid; k < d; k += NT)
            if (is_nonfinite_bits(item.V[(int64_t)own * d + k])) bad = true;
    }
    return bad;
}

// Status 2: the row all NaN, the objective(s) NaN, 0 iterations.
template <int NT, bool ITEM>
__device__ __forceinline__ void fold_invalid_row(float *__restrict__ out, int d, double *__restrict__ objective,
                                                 int32_t *__restrict__ iters_status, int r, int tid)
{
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int k = tid; k < d; k += NT) out[k] = qnan;
    if (tid == 0) {
        if constexpr (ITEM) {
            if (objective) objective[2 * r] = objective[2 * r + 1] = (double)qnan;
        } else {
            if (objective) objective[r] = (double)qnan;
        }
        iters_status[2 * r] = 0;
        iters_status[2 * r + 1] = 2;
    }
}

// A user without comparisons: u = 0 whatever U_init holds.
template <int NT>
__device__ __forceinline__ void fold_empty_user_row(float *__restrict__ out, int d, double *__restrict__ objective,
                                                    int32_t *__restrict__ iters_status, int r, int tid)
{
    for (int k = tid; k < d; k += NT) out[k] = 0.0f;
    if (tid == 0) {
        if (objective) objective[r] = 0.0;
        iters_status[2 * r] = 0;
        iters_status[2 * r + 1] = 0;
    }
}

// An item without comparisons: v* = 0, the row moves theta of the way to it.
template <int NT>
__device__ __forceinline__ void fold_empty_item_row(float *__restrict__ out, int d, const float *__restrict__ vold,
                                                    double theta, double l2, double *__restrict__ objective,
                                                    int32_t *__restrict__ iters_status, int r, int tid)
{
    for (int k = tid; k < d; k += NT) out[k] = (float)fma(theta, -(double)vold[k], (double)vold[k]);
    if (tid == 0) {
        double vv = 0.0;
        for (int k = 0; k < d; ++k) vv = fma((double)vold[k], (double)vold[k], vv);
        if (objective) {
            objective[2 * r] = 0.5 * l2 * vv;
            objective[2 * r + 1] = 0.0;
        }
        iters_status[2 * r] = 0;
        iters_status[2 * r + 1] = 0;
    }
}

// The item step's prologue: c_t = -sigma_t U[u_t] . V[o_t], one thread per comparison, k ascending; both rows are
// checked.  Returns this thread's verdict; a barrier has to follow before c_t is read.
template <int NT>
__device__ __forceinline__ bool fold_form_offsets(const float *__restrict__ U, int d, const mfcd_sample *__restrict__ rec,
                                                  int64_t b, int64_t e, int own, const FoldItem &item, int tid)
{
    bool bad = false;
    for (int64_t t = b + tid; t < e; t += NT) {
        const mfcd_sample q = rec[t];
        const int sigma = (q.i == own) - (q.j == own);
        const float *ur = U + (int64_t)q.u * d, *vr = item.V + (int64_t)(q.i == own ? q.j : q.i) * d;
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
            const float a = ur[k], c = vr[k];
            if (is_nonfinite_bits(a) || is_nonfinite_bits(c)) bad = true;
            acc = fma((double)a, (double)c, acc);
        }
        item.c[t] = sigma == 0 ? 0.0 : -(double)sigma * acc;
    }
    return bad;
}

// One staged entry delta_t[k], exact in f64.  User step: V[i][k] - V[j][k], and *flag is set for a non-finite entry.
// Item step: sigma U[u][k] (the rows were checked by the prologue).
template <bool ITEM>
__device__ __forceinline__ double fold_delta(const float *__restrict__ V, int d, const mfcd_sample q, int own, int k, int *flag)
{
    if constexpr (ITEM) {
        return (double)((q.i == own) - (q.j == own)) * (double)V[(int64_t)q.u * d + k];
    } else {
        const float vi = V[(int64_t)q.i * d + k], vj = V[(int64_t)q.j * d + k];
        if (is_nonfinite_bits(vi) || is_nonfinite_bits(vj)) *flag = 1;
        return (double)vi - (double)vj;
    }
}

// ---- the per-comparison scalar functions ----
// e^-|x| and 1 / (1 + e^-|x|): what p, the weight and softplus are formed from
struct FoldLogit {
    double x, ex, q;
    __device__ __forceinline__ explicit FoldLogit(double x_) : x(x_), ex(exp(-fabs(x_))), q(1.0 / (1.0 + ex)) {}
    __device__ __forceinline__ double p() const { return x >= 0.0 ? q : ex * q; }
    __device__ __forceinline__ double weight() const { return ex * q * q; }                          // p (1 - p)
    __device__ __forceinline__ double softplus() const { return fmax(x, 0.0) + log1p(ex); }
    __device__ __forceinline__ double term(double z) const { return softplus() - z * x; }            // its term of f
};

// softplus(x0 + h) - softplus(x0) - z h: log1p(p expm1(h)) for |h| < 1, the difference of the two values otherwise
__device__ __forceinline__ double fold_decrease_term(const FoldLogit &at, double h, double z)
{
    if (fabs(h) < 1.0) return log1p(at.p() * expm1(h)) - z * h;
    const double x1 = at.x + h;                        // a long step: the two softplus values differ visibly
    return ((fmax(x1, 0.0) + log1p(exp(-fabs(x1)))) - at.softplus()) - z * h;
}

// ---- the acceptance rule of the backtracking line search (t = 1, 1/2, ..., at most kFoldHalvings halvings): the Armijo
// decrease with gs = g . s, on the decrease f(u + t s) - f(u) summed term by term or on the two values of f.  Either
// evaluation accepts: the term-wise decrease resolves steps that f cannot show, the values of f settle a step so small
// that the term-wise sum is itself at its rounding level (u + t s == u at last). ----
__device__ __forceinline__ bool fold_armijo_accepts(double decrease, double fnew, double fcur, double t, double gs)
{
    return decrease <= kFoldArmijo * t * gs || fnew <= fcur + kFoldArmijo * t * gs;
}

// ---- the Newton direction of a Cholesky kernel: out = -H^-1 g for the symmetric H [n][ld] in LDS, n <= NT ----
// H is factored in place on its lower triangle, right-looking, two barriers per column, the trailing block walked on a
// G x G grid of threads; the diagonal of L goes to diag[].  Then L y = -g (y in sol[]) and L^T out = y: one entry per
// thread, one barrier per column.  The first column's barrier makes H and g visible, the last solve step's makes out
// visible on return.  False when a pivot is not positive: out is untouched, every thread has left at the same column.
template <int NT, int G>
__device__ __forceinline__ bool fold_cholesky_solve(double *H, int ld, int n, double *diag, double *sol, const double *g,
                                                    double *out, int tid)
{
    for (int k = 0; k < n; ++k) {
        __syncthreads();
        const double dk = H[k * ld + k];
        if (!(dk > 0.0)) return false;
        const double lkk = sqrt(dk);
        if (tid == 0) diag[k] = lkk;
        for (int i = k + 1 + tid; i < n; i += NT) H[i * ld + k] = H[i * ld + k] / lkk;
        __syncthreads();
        for (int i = k + 1 + (tid / G); i < n; i += G)
            for (int j = k + 1 + (tid % G); j <= i; j += G)
                H[i * ld + j] = fma(-H[i * ld + k], H[j * ld + k], H[i * ld + j]);
    }
    double rhs = tid < n ? -g[tid] : 0.0;
    for (int k = 0; k < n; ++k) {
        if (tid == k) sol[k] = rhs / diag[k];
        __syncthreads();
        if (tid > k && tid < n) rhs = fma(-H[tid * ld + k], sol[k], rhs);
    }
    rhs = tid < n ? sol[tid] : 0.0;
    for (int k = n - 1; k >= 0; --k) {
        if (tid == k) out[k] = rhs / diag[k];
        __syncthreads();
        if (tid < k) rhs = fma(-H[k * ld + tid], out[k], rhs);
    }
    return true;
}

// ---- epilogue: the f64 iterate u rounded once (item step: v_old + theta (v* - v_old) in f64 first), objectives, status ----
template <int NT, bool ITEM>
__device__ __forceinline__ void fold_finish(float *__restrict__ out, const double *u, int d, const FoldItem &item, int own,
                                            double *__restrict__ objective, int32_t *__restrict__ iters_status, int r,
                                            double fstart, double fcur, int it, int status, int tid)
{
    if constexpr (ITEM) {
        const float *vold = item.V + (int64_t)own * d;
        for (int k = tid; k < d; k += NT) out[k] = (float)fma(item.theta, u[k] - (double)vold[k], (double)vold[k]);
    } else {
        for (int k = tid; k < d; k += NT) out[k] = (float)u[k];
    }
    if (tid == 0) {
        if constexpr (ITEM) {
            if (objective) {
                objective[2 * r] = fstart;
                objective[2 * r + 1] = fcur;
            }
        } else {
            if (objective) objective[r] = fcur;
        }
        iters_status[2 * r] = it;
        iters_status[2 * r + 1] = status;
    }
}

}  // namespace
