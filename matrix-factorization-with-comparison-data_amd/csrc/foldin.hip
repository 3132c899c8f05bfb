// foldin.hip — the exact block steps of the BTL fit on gfx950.  The user step: with the item table V held
// fixed, every user's row u minimises
//     f(u) = sum over the row's comparisons t of  softplus(x_t) - z_t x_t  +  (l2 / 2) |u|^2,
//     x_t = u . delta_t,   delta_t = V[i_t] - V[j_t],
// a strictly convex d-dimensional logistic regression.  Rows are independent, so one workgroup owns one row and runs
// the whole damped Newton iteration for it: there is no communication between workgroups, no atomic and no workspace.
//
// The item step is the same kernel with another staging policy (template parameter ITEM): with U and the other items
// fixed, item k's row v minimises the same f over the comparisons that hold k, with
//     x_t = v . delta_t + c_t,   delta_t = sigma_t U[u_t],   sigma_t = [i_t = k] - [j_t = k],   c_t = -sigma_t U[u_t] . V[o_t],
// o_t the other item of the comparison: a logistic regression with an offset.  c_t does not change during a row's
// iteration, so the workgroup forms it once in a prologue (an f64 fma chain over k per comparison, one thread each) and
// keeps it in the call's workspace, 8 bytes per record that only this workgroup reads back; staging then gathers one U
// row per comparison and puts c_t into the stage's pad column D[t * ld + dpad], which the user step leaves unused, so
// the LDS budget is the same.  The x chains start at c_t instead of 0; everything after staging is shared code.  The
// output is v_old + theta (v* - v_old): at theta = 1/2 all items may move at once and F still descends.
//
// Per iteration (include/mfcd.h states the algorithm; tests/foldin_model.py restates it in numpy):
//   pass with Hessian   the row's comparisons go through LDS kFoldChunk = 64 at a time.  Staging gathers the two V rows
//                       of a comparison and stores delta_t = (double)V[i] - (double)V[j], which is exact.  Thread t < 64
//                       forms x_t by a serial f64 fma chain over k, then p_t, the weight p_t (1 - p_t), the residual
//                       p_t - z_t and its term of f.  Thread k < d adds the chunk's residual * delta[.][k] to its
//                       gradient entry; thread (bi, bj) adds the chunk's rank-64 update to the 4 x 4 block of the Hessian
//                       it owns.  Gradient entries, Hessian blocks and the f partials live in registers for the whole
//                       pass: every sum has one owner and a fixed order, so no reduction over d^2 entries is needed.
//   Cholesky            fold_cholesky_solve (foldin_common.h): in place in LDS, right-looking, two barriers per column;
//                       the two triangular solves keep one right-hand-side entry per thread, one barrier per column.
//   line search         the same staging without the Hessian part.  The Armijo test is taken on the decrease
//                       f(u + t s) - f(u) summed term by term, softplus(x + h) - softplus(x) = log1p(p expm1(h)) for
//                       |h| < 1, not on two rounded values of f: close to the minimiser (a warm start from an fp32 row)
//                       the decrease of a full Newton step is below the last bit of f, and a test on f itself would
//                       halve such steps at random.
//
// Which pipe forms the Hessian: the f64 vector pipe (v_fma_f64).  On gfx950 the fp32 MFMA runs at the fp32 vector
// rate and the f64 MFMA at the f64 vector rate, so a matrix form would save instruction issue and LDS reads, not
// arithmetic; an fp32 Hessian is allowed by the contract but costs iterations where the weights span many orders of
// magnitude (separable rows), and the pass is shared with the gradient, which has to be f64.  With 4 x 4 register
// blocks a thread reads 8 doubles and one weight from LDS per 16 fma; all 64 lanes of a wave read at most 5 distinct
// block columns of one staged row, which the LDS serves as broadcasts.
//
// LDS at d = 64: H 64 x 65 doubles (33 280 B, the odd stride keeps a column walk off one bank), the stage 64 x 65
// doubles (33 280 B), seven vectors of 64 doubles and three of kFoldChunk: 72 KiB, two workgroups of 256 threads per
// CU.  d <= 16 takes one wave per row (H and the stage are then at most 4.4 KiB each).  More rows than CUs is the
// normal case; the hardware's workgroup dispatcher balances ragged rows.
//
// d > 64: foldin_cg.hip solves the same two problems by conjugate gradients on Hessian-vector products instead of a
// Cholesky factor in LDS; what the two kernels share, the host check of their entries included, is in foldin_common.h.
#include "foldin_common.h"

namespace {

constexpr int kFoldMaxD = 64;
constexpr int kFoldChunk = 64;        // T: comparisons staged per pass of the inner loop

// doubles of LDS a workgroup needs for width d (the int flag rides in the last one)
inline size_t fold_lds_doubles(int d)
{
    const int dpad = ((d + 3) >> 2) << 2, ld = dpad + 1;
    return (size_t)dpad * ld + (size_t)kFoldChunk * ld + 6 * (size_t)dpad + 3 * (size_t)kFoldChunk + 5 + 1;
}

// ITEM = false: the user step.  V [m][d] is the gathered table, U_init the start rows, objective [rows].
// ITEM = true: the item step.  V is the gathered table U [m = n][d], U_init is unused, item holds the rest,
// objective [rows][2] = {f at the start, f at the solution}.
template <int NT, bool ITEM>
__global__ __launch_bounds__(NT) void fold_in_kernel(const float *__restrict__ V, int m, int d,
                                                     const mfcd_sample *__restrict__ rec,
                                                     const int64_t *__restrict__ row_off, double l2,
                                                     const float *__restrict__ U_init, int max_iter, double xtol,
                                                     float *__restrict__ U_out, double *__restrict__ objective,
                                                     int32_t *__restrict__ iters_status, const FoldItem item)
{
    constexpr int T = kFoldChunk;
    constexpr int G = NT == 256 ? 16 : 8;              // the Cholesky update walks the trailing block on a G x G grid
    extern __shared__ double fold_lds[];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int nb = (d + 3) >> 2, dpad = nb << 2, ld = dpad + 1;
    double *H = fold_lds, *D = H + dpad * ld, *u = D + T * ld, *g = u + dpad, *s = g + dpad, *ut = s + dpad;
    double *sol = ut + dpad, *diag = sol + dpad, *w = diag + dpad, *res = w + T, *fpart = res + T, *scal = fpart + T;
    int *flag = (int *)(scal + 5);
    float *out = U_out + (int64_t)r * d;

    const int64_t b = row_off[r], e = row_off[r + 1];
    const int own = ITEM ? (item.row_item ? item.row_item[r] : r) : 0;      // the item this row solves
    if (!ITEM && e == b) {
        fold_empty_user_row<NT>(out, d, objective, iters_status, r, tid);
        return;
    }

    // ---- validation: indices and labels before any gather, the start vector; V rows are checked as they are staged ----
    if (tid == 0) *flag = 0;
    __syncthreads();
    if constexpr (ITEM) {
        if (fold_item_row_is_bad<NT>(m, d, rec, b, e, own, item, tid)) *flag = 1;
    } else {
        if (fold_user_row_is_bad<NT>(m, d, rec, b, e, U_init ? U_init + (int64_t)r * d : nullptr, tid)) *flag = 1;
    }
    __syncthreads();

    auto invalid_row = [&]() { fold_invalid_row<NT, ITEM>(out, d, objective, iters_status, r, tid); };
    if (*flag) {
        invalid_row();
        return;
    }

    if constexpr (ITEM) {
        const float *vold = item.V + (int64_t)own * d;
        if (e == b) {
            fold_empty_item_row<NT>(out, d, vold, item.theta, l2, objective, iters_status, r, tid);
            return;
        }
        if (fold_form_offsets<NT>(V, d, rec, b, e, own, item, tid)) *flag = 1;
        __syncthreads();                               // c_t is visible to the workgroup that wrote it
        if (*flag) {
            invalid_row();
            return;
        }
        for (int k = tid; k < dpad; k += NT) u[k] = k < d ? (double)vold[k] : 0.0;
    } else {
        for (int k = tid; k < dpad; k += NT) u[k] = (U_init && k < d) ? (double)U_init[(int64_t)r * d + k] : 0.0;
    }

    // staging geometry: P = the power of two >= dpad lanes per comparison, NT / P comparisons per sweep
    int lg = 2;
    while ((1 << lg) < dpad) ++lg;
    const int sk = tid & ((1 << lg) - 1), st0 = tid >> lg, ststep = NT >> lg;
    const bool hthread = tid < nb * nb;
    const int bi = hthread ? tid / nb : 0, bj = hthread ? tid - bi * nb : 0;

    // One pass over the row at the point uv: returns f(uv); with HESS also g (gradient) and H (Hessian) at uv.  Without
    // HESS uv is the trial point u + tt s, and scal[4] receives the decrease f(u + tt s) - f(u) summed term by term:
    // with h = tt s . delta_t and p = sigmoid(u . delta_t), softplus(x + h) - softplus(x) = log1p(p expm1(h)), which is
    // exact to the rounding of the difference itself, so the Armijo test sees decreases far below the rounding of f.
    auto pass = [&](const double *uv, bool hess, double tt) -> double {
        double facc = 0.0, gacc = 0.0, dacc = 0.0;
        double hacc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) hacc[a][c] = 0.0;
        for (int64_t c0 = b; c0 < e; c0 += T) {
            const int cn = (int)(e - c0 < T ? e - c0 : T);
            __syncthreads();                           // the previous chunk's readers are done; uv is visible
            if (sk < dpad)
                for (int t = st0; t < cn; t += ststep) {
                    D[t * ld + sk] = sk < d ? fold_delta<ITEM>(V, d, rec[c0 + t], own, sk, flag) : 0.0;
                    if constexpr (ITEM)                // c_t rides in the pad column
                        if (sk == 0) D[t * ld + dpad] = item.c[c0 + t];
                }
            __syncthreads();
            if (tid < cn) {
                const double *row = D + tid * ld;
                double x = 0.0;
                if constexpr (ITEM) x = row[dpad];
                for (int k = 0; k < d; ++k) x = fma(uv[k], row[k], x);
                const double z = (double)rec[c0 + tid].z;
                const FoldLogit at(x);
                facc += at.term(z);
                if (hess) {
                    w[tid] = at.weight();
                    res[tid] = at.p() - z;
                } else {
                    double x0 = 0.0, sx = 0.0;
                    if constexpr (ITEM) x0 = row[dpad];
                    for (int k = 0; k < d; ++k) {
                        x0 = fma(u[k], row[k], x0);
                        sx = fma(s[k], row[k], sx);
                    }
                    dacc += fold_decrease_term(FoldLogit(x0), tt * sx, z);
                }
            }
            if (hess) {
                __syncthreads();
                if (tid < dpad)
                    for (int t = 0; t < cn; ++t) gacc = fma(res[t], D[t * ld + tid], gacc);
                if (hthread)
                    for (int t = 0; t < cn; ++t) {
                        const double *ra = D + t * ld + 4 * bi, *rb = D + t * ld + 4 * bj;
                        const double wt = w[t];
                        double wa[4], cb[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            wa[a] = wt * ra[a];
                            cb[a] = rb[a];
                        }
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int c = 0; c < 4; ++c) hacc[a][c] = fma(wa[a], cb[c], hacc[a][c]);
                    }
            }
        }
        __syncthreads();
        if (tid < T) fpart[tid] = facc;
        if (!hess && tid < T) w[tid] = dacc;
        if (hess) {
            if (tid < dpad) g[tid] = tid < d ? gacc + l2 * uv[tid] : 0.0;
            if (hthread)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int hi = 4 * bi + a, hj = 4 * bj + c;
                        // the padding rows and columns carry an identity block: their solution entries stay 0
                        H[hi * ld + hj] = hacc[a][c] + (hi == hj ? (hi < d ? l2 : 1.0) : 0.0);
                    }
        }
        __syncthreads();
        if (tid == 0) {
            double f = 0.0, uu = 0.0;
            for (int t = 0; t < T; ++t) f += fpart[t];
            for (int k = 0; k < d; ++k) uu = fma(uv[k], uv[k], uu);
            scal[0] = f + 0.5 * l2 * uu;
            if (!hess) {
                double dsum = 0.0, us = 0.0, ss = 0.0;
                for (int t = 0; t < T; ++t) dsum += w[t];
                for (int k = 0; k < d; ++k) {
                    us = fma(u[k], s[k], us);
                    ss = fma(s[k], s[k], ss);
                }
                scal[4] = dsum + l2 * (tt * us + 0.5 * tt * tt * ss);
            }
        }
        __syncthreads();
        return scal[0];
    };

    double fcur = pass(u, true, 0.0);
    const double fstart = fcur;
    if (*flag) {                                       // a V row of this user holds an inf or a NaN
        invalid_row();
        return;
    }

    int it = 0, status = 1;
    for (;;) {                                         // g, H and fcur belong to u
        ++it;
        // s = -H^-1 g; a pivot that is not positive is not reached for l2 > 0 and finite data: u stays as it is
        if (!fold_cholesky_solve<NT, G>(H, ld, dpad, diag, sol, g, s, tid)) break;
        if (tid == 0) {
            double smax = 0.0, gs = 0.0;
            for (int k = 0; k < d; ++k) {
                smax = fmax(smax, fabs(s[k]));
                gs = fma(g[k], s[k], gs);
            }
            scal[1] = smax;
            scal[2] = gs;
        }
        __syncthreads();
        const double smax = scal[1], gs = scal[2];
        if (smax == 0.0) {
            status = 0;
            break;
        }
        // ---- backtracking: t = 1, 1/2, ... until the Armijo decrease holds ----
        double t = 1.0, fnew = 0.0;
        bool accepted = false;
        for (int h = 0; h <= kFoldHalvings && !accepted; ++h) {
            if (tid < dpad) ut[tid] = fma(t, s[tid], u[tid]);
            fnew = pass(ut, false, t);
            accepted = fold_armijo_accepts(scal[4], fnew, fcur, t, gs);
            if (!accepted) t *= 0.5;
        }
        if (!accepted) break;                          // status 1: u is the last accepted iterate
        if (tid < dpad) u[tid] = ut[tid];
        fcur = fnew;
        if (tid == 0) {
            double umax = 0.0;
            for (int k = 0; k < d; ++k) umax = fmax(umax, fabs(ut[k]));
            scal[3] = umax;
        }
        __syncthreads();
        if (t * smax <= xtol * scal[3]) {
            status = 0;
            break;
        }
        if (it >= max_iter) break;
        fcur = pass(u, true, 0.0);
    }

    __syncthreads();
    fold_finish<NT, ITEM>(out, u, d, item, own, objective, iters_status, r, fstart, fcur, it, status, tid);
}

template <int NT, bool ITEM>
int fold_launch(const float *V, int m, int d, const mfcd_sample *rec, const int64_t *row_off, int rows, double l2,
                const float *U_init, int max_iter, double xtol, float *U_out, double *objective, int32_t *iters_status,
                const FoldItem &item, hipStream_t st)
{
    const size_t lds = fold_lds_doubles(d) * sizeof(double);
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)fold_in_kernel<NT, ITEM>, lds, allowed));
    hipLaunchKernelGGL((fold_in_kernel<NT, ITEM>), dim3((unsigned)rows), dim3(NT), lds, st, V, m, d, rec, row_off, l2,
                       U_init, max_iter, xtol, U_out, objective, iters_status, item);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mfcd_fold_in_max_d(void) { return kFoldMaxD; }

extern "C" int mfcd_fold_in_chunk(void) { return kFoldChunk; }

extern "C" size_t mfcd_fold_in_workspace_bytes(int rows, int d)
{
    if (rows < 0 || d < 1 || d > kFoldMaxD) return 0;
    return 256;                                        // every sum of the kernel has one owner: nothing is staged in HBM
}

extern "C" int mfcd_fold_in_users(const float *V, int m, int d, const mfcd_sample *records, const int64_t *row_off,
                                  int rows, double l2, const float *U_init, int max_iter, double xtol, float *U_out,
                                  double *objective, int32_t *iters_status, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    if (!V || m < 1) return MFCD_EINVAL;
    const int bad = fold_entry_check(d, kFoldMaxD, row_off, rows, l2, max_iter, xtol, U_out, iters_status, V, m, U_init, rows,
                                     workspace, workspace_bytes, mfcd_fold_in_workspace_bytes(rows, d));
    if (bad || rows == 0) return bad;
    hipStream_t st = (hipStream_t)stream;
    const FoldItem none{};
    if (d <= 16)
        return fold_launch<64, false>(V, m, d, records, row_off, rows, l2, U_init, max_iter, xtol, U_out, objective,
                                      iters_status, none, st);
    return fold_launch<256, false>(V, m, d, records, row_off, rows, l2, U_init, max_iter, xtol, U_out, objective,
                                   iters_status, none, st);
}

extern "C" size_t mfcd_item_step_workspace_bytes(int rows, int d, int64_t records)
{
    if (rows < 0 || d < 1 || d > kFoldMaxD || records < 0 || records > (int64_t)1 << 56) return 0;
    return 256 + align_up(sizeof(double) * (size_t)records);      // c_t per record behind the common 256 bytes
}

extern "C" int mfcd_item_step(const float *U, int n, const float *V, int m, int d, const mfcd_sample *records,
                              const int64_t *row_off, const int32_t *row_item, int rows, double l2, double theta,
                              int max_iter, double xtol, float *V_out, double *objective2, int32_t *iters_status,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    if (!U || !V || n < 1 || m < 1 || (!row_item && rows > m) || !(theta > 0.0 && theta <= 1.0)) return MFCD_EINVAL;
    // the record count is on the device (row_off[rows]): the host requires the fixed part, and a row whose records end
    // beyond what the workspace holds is refused by its own workgroup (status 2)
    const int bad = fold_entry_check(d, kFoldMaxD, row_off, rows, l2, max_iter, xtol, V_out, iters_status, U, n, V, m,
                                     workspace, workspace_bytes, mfcd_item_step_workspace_bytes(rows, d, 0));
    if (bad || rows == 0) return bad;
    const FoldItem item{V, m, row_item, theta, (double *)((char *)workspace + 256),
                        (int64_t)((workspace_bytes - 256) / sizeof(double))};
    hipStream_t st = (hipStream_t)stream;
    if (d <= 16)
        return fold_launch<64, true>(U, n, d, records, row_off, rows, l2, nullptr, max_iter, xtol, V_out, objective2,
                                     iters_status, item, st);
    return fold_launch<256, true>(U, n, d, records, row_off, rows, l2, nullptr, max_iter, xtol, V_out, objective2,
                                  iters_status, item, st);
}
