// ratings_foldin.hip — the exact user step on observed ratings in one launch on gfx950 (include/mfcd.h:
// mfcd_ratings_fold_in_users).  Row r of a CSR ratings table owns entries [row_off[r], row_off[r+1]) of idx (the
// entry's item, a row of V [m][d]) and x (its rating); with V fixed its vector u minimises
//     f(u) = coef * R_r(a) + (l2 / 2) |u|^2,   a_e = u . v~_e,
//     R_r(a) = sum over the pairs e < l of the row of  w_el [softplus(a_e - a_l) - sigmoid(scale (x_e - x_l)) (a_e - a_l)],
// w_el = 1, or [x_e != x_l] under MFCD_RAGGED_SKIP_TIES: mfcd/ratings_exact.py's ratings_user_step, which runs
// population._newton over all rows in lockstep, one chain of small launches per iteration.  Here one workgroup of 256
// threads owns one row and runs that iteration (solver "direct": the d x d Hessian and a Cholesky factor in LDS) from
// start to finish; tests/ratings_foldin_model.py restates it in numpy.
//
// v~_e is the row's gathered item vector minus the row's f64 column mean, rounded to fp32 once (pair_info.hip's rule):
// every quantity depends on differences of the v_e only.  It is never stored: wherever a v~ is needed it is gathered
// again from V (L d loads against L^2 pairs per pass), so there is no split between resident and streamed rows and no
// workspace.  What stays in LDS for the whole row is (a_e, x_e), g_e and the step's share h_e, 16 bytes per entry.
//
// The three passes over a row's L^2 ordered pairs; thread t of the workgroup owns entries t, t + 256, ... and meets
// every entry l of the row as a broadcast read of (a_l, x_l) from LDS; a wave whose 64 entries lie past the row's end
// skips the pair loops:
//   value and gradient   one loop: the risk terms of pair_term<2, true> (both orders of a pair give the same term, so
//                        the sum over ordered pairs is halved, exactly) and g_e = sum_l w (sigmoid(a_e - a_l) -
//                        sigmoid(scale (x_e - x_l))), fp32 runs of 64 columns widened to f64.  g = coef sum_e g_e v~_e
//                        + l2 u: thread (k, slice) adds the entries of its slice for column k in f64, the slices are
//                        added in order.  At a trial point u + t p the loop also adds the decrease f(u + t p) - f(u)
//                        pair by pair, from h_e = t p . v~_e: the Armijo test is taken on it as well as on the two
//                        values of f, whose fp32 rounding (1e-7 of c R) exceeds the decrease of the last Newton steps
//                        of a short row in a large table (measured: a row of 3 entries stalled at grad_ratio 0.03).
//   Hessian              Z = (D - C) V~ at DK multiply-adds per pair on the fp32 vector pipe: the columns l go through
//                        LDS in stages of 64 rows of V~, thread e keeps z_e in registers (fp32 per stage, widened to
//                        f64), z_e = deg_e v~_e - sum_l c_el v~_l rounded to fp32 once.  Then H = V~^T Z in f64: the
//                        tile's entries go through LDS in slabs of 64 and thread (bi, bj), bi >= bj, adds the rank-64
//                        update of the 4 x 4 block it owns, as fold_in_kernel does; the upper triangle is the mirror
//                        image of the lower, bit for bit.
//   Cholesky and solves  in place in LDS, right-looking: foldin_common.h's fold_cholesky_solve written out, because the
//                        call cost this kernel 0.4 to 1 % (profiles/fold_family_refactor.txt): fix both copies together.
// No atomics, no allocation, no host wait; every sum has one owner and a fixed order that depends on the row alone.
#include <cmath>

#include "foldin_common.h"
#include "pairs_common.h"

namespace {

constexpr int kRfMaxD = 64;
constexpr int kRfMaxLen = 3072;                        // see include/mfcd.h: from the measured pass times at d = 64
constexpr int kRfThreads = 256;
constexpr int kRfStage = 64;                           // columns per LDS stage = terms per fp32 run
constexpr double kRfMinStep = 1.0 / 4096.0;            // population.MIN_STEP

struct RfArgs {
    const float *V;
    int m, d;
    const int32_t *idx;
    const float *x;
    int64_t entries;
    const int64_t *row_off;
    int r0;
    float scale;
    double coef, l2;
    const float *U_init;
    int max_newton;
    double gtol;
    float *U_out;
    double *objective, *grad_ratio;
    int32_t *iters_status;
    double *info;
};

// bytes of LDS a workgroup of the DK form takes
constexpr size_t rf_lds_bytes(int DK)
{
    return sizeof(double) * ((size_t)DK * (DK + 1) + 8 * (size_t)DK + kRfThreads + 32) +
           sizeof(float) * ((size_t)kRfStage * DK + (size_t)kRfStage * (DK + 1) + 4 * (size_t)kRfMaxLen) + 16;
}

// softplus(da) - softplus(da - h) - q h of one ordered pair, da the score difference at the trial point and h the step's
// share of it: log1p(p expm1(h)) with p = sigmoid(da - h) for |h| < 1, exact to the rounding of the difference itself;
// the difference of the two softplus values for a long step, where they differ visibly.  h = 0 gives exactly 0.
__device__ __forceinline__ float rf_decrease_term(float da, float h, float q)
{
    const float d0 = da - h;
    if (fabsf(h) < 1.0f) return fmaf(-q, h, log1pf(pair_sigmoid(d0) * expm1f(h)));
    const float s1 = fmaxf(da, 0.0f) + 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(da)));
    const float s0 = fmaxf(d0, 0.0f) + 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(d0)));
    return fmaf(-q, h, s1 - s0);
}

// Statuses 2 and 3, and the closed form of a row without a supporting pair (status 0).
__device__ __forceinline__ void rf_constant_row(const RfArgs &g, int r, int tid, bool nan, int status, double f_start)
{
    const int d = g.d;
    const float rowv = nan ? __uint_as_float(0x7fc00000u) : 0.0f;
    const double dv = nan ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    for (int k = tid; k < d; k += kRfThreads) g.U_out[(int64_t)r * d + k] = rowv;
    if (g.info)
        for (int q = tid; q < d * d; q += kRfThreads) g.info[(int64_t)r * d * d + q] = dv;
    if (tid == 0) {
        if (g.objective) {
            g.objective[2 * (int64_t)r] = nan ? dv : f_start;
            g.objective[2 * (int64_t)r + 1] = dv;
        }
        if (g.grad_ratio) g.grad_ratio[r] = dv;
        g.iters_status[2 * (int64_t)r] = 0;
        g.iters_status[2 * (int64_t)r + 1] = status;
    }
}

template <int DK, bool SKIP>
__global__ __launch_bounds__(kRfThreads) void ratings_fold_in_kernel(const RfArgs g)
{
    constexpr int NT = kRfThreads, LD = DK + 1, ZLD = DK + 1, NB = DK / 4, GR = 16;
    extern __shared__ double rf_lds[];
    double *H = rf_lds, *u = H + DK * LD, *gv = u + DK, *gt = gv + DK, *p = gt + DK, *ut = p + DK, *mean = ut + DK;
    double *sol = mean + DK, *diag = sol + DK, *part = diag + DK, *scal = part + NT;
    float *S = (float *)(scal + 32), *Zs = S + kRfStage * DK, *G = Zs + kRfStage * ZLD, *HS = G + kRfMaxLen;
    float2 *AX = (float2 *)(HS + kRfMaxLen);           // an even number of floats precedes it: 8-byte aligned

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = g.d;
    const int r = g.r0 + blockIdx.x;
    const float *__restrict__ V = g.V;

    // ---- validation: offsets, length, every index and rating, the start row: before any gather ----
    const int64_t b = g.row_off[r], e_end = g.row_off[r + 1];
    if (!(b >= 0 && e_end >= b && e_end <= g.entries)) {
        rf_constant_row(g, r, tid, true, 2, 0.0);
        return;
    }
    if (e_end - b > kRfMaxLen) {
        rf_constant_row(g, r, tid, true, 3, 0.0);
        return;
    }
    const int L = (int)(e_end - b);
    const int32_t *__restrict__ idx = g.idx + b;
    const float *__restrict__ x = g.x + b;
    const float *start = g.U_init ? g.U_init + (int64_t)r * d : nullptr;
    int bad = 0, differs = 0;
    {
        const float x0 = L > 0 ? x[0] : 0.0f;
        for (int e = tid; e < L; e += NT) {
            const float xe = x[e];
            bad |= (int)((unsigned)idx[e] >= (unsigned)g.m || is_nonfinite_bits(xe));
            differs |= (int)(xe < x0 || xe > x0);
        }
        if (start)
            for (int k = tid; k < d; k += NT) bad |= (int)is_nonfinite_bits(start[k]);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        rf_constant_row(g, r, tid, true, 2, 0.0);
        return;
    }
    differs = __syncthreads_or(differs);
    if (L < 2 || (SKIP && !differs)) {                 // no supporting pair: the risk is identically 0
        double uu = 0.0;
        if (start)
            for (int k = 0; k < d; ++k) uu = fma((double)start[k], (double)start[k], uu);
        rf_constant_row(g, r, tid, false, 0, 0.5 * g.l2 * uu);
        return;
    }

    // ---- geometry ----
    int lg = 0;
    while ((1 << lg) < d) ++lg;
    const int P = 1 << lg, ck = tid & (P - 1), csl = tid >> lg, nsl = NT >> lg;   // column sums: (column, slice)
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= tid) ++bi;       // the lower block (bi, bj) this thread owns
    const int bj = tid - bi * (bi + 1) / 2;
    const bool hthread = bi < NB;
    const int T = (L + NT - 1) / NT;

    // One gathered, centred entry of V~.
    auto centred = [&](int e, int k) -> float { return (float)((double)V[(int64_t)idx[e] * d + k] - mean[k]); };

    // out[k] = sum over the row's entries of V[idx_e][k] / L (WEIGHTED = false: the mean; flags a non-finite entry) or
    // coef * sum_e G[e] v~_e[k] + l2 uv[k] (the gradient).  Ends with a barrier.
    auto colsum = [&](bool weighted, const double *uv, double *out) -> int {
        double s = 0.0;
        int badv = 0;
        if (ck < d)
            for (int e = csl; e < L; e += nsl) {
                const float v = V[(int64_t)idx[e] * d + ck];
                if (!weighted) {
                    badv |= (int)is_nonfinite_bits(v);
                    s += (double)v;
                } else {
                    s = fma((double)G[e], (double)(float)((double)v - mean[ck]), s);
                }
            }
        part[tid] = s;
        badv = __syncthreads_or(badv);
        if (tid < DK) {
            double tsum = 0.0;
            if (tid < d)
                for (int w = 0; w < nsl; ++w) tsum += part[w * P + tid];   // fixed order
            out[tid] = tid < d ? (weighted ? fma(g.coef, tsum, g.l2 * uv[tid]) : tsum / (double)L) : 0.0;
        }
        __syncthreads();
        return badv;
    };

    // AX[e] = (a_e, x_e) at the point uv and HS[e] = tt p . v~_e, the entry's share of the step from u to uv = u + tt p:
    // f64 chains over k, each rounded to fp32 once.  Ends with a barrier.
    auto scores = [&](const double *uv, double tt) {
        for (int e = tid; e < L; e += NT) {
            const float *vr = V + (int64_t)idx[e] * d;
            double a = 0.0, h = 0.0;
            for (int k = 0; k < d; ++k) {
                const double vt = (double)(float)((double)vr[k] - mean[k]);
                a = fma(uv[k], vt, a);
                h = fma(p[k], vt, h);
            }
            AX[e] = make_float2((float)a, x[e]);
            HS[e] = (float)(tt * h);
        }
        __syncthreads();
    };

    // f(uv), and the gradient at uv into gout; uv = u + tt p (the start: tt = 0).  scal[5] receives the decrease
    // f(uv) - f(u) summed pair by pair (rf_decrease_term), which resolves steps whose decrease lies below the fp32
    // rounding of the two values of f: close to the minimiser of a short row that is every step the certificate needs.
    auto value_grad = [&](const double *uv, double *gout, double tt) -> double {
        scores(uv, tt);
        double f0 = 0.0, f1 = 0.0, fd = 0.0;           // log2 parts, linear parts, decreases of the thread's entries
        for (int I = 0; I < T; ++I) {
            const int e = I * NT + tid;
            if (I * NT + (tid & ~63) >= L) continue;   // the wave holds no entry of this tile
            const bool in = e < L;
            const float2 own = in ? AX[e] : make_float2(0.0f, 0.0f);
            const float hown = in ? HS[e] : 0.0f;
            double ga = 0.0, a0 = 0.0, a1 = 0.0, ad = 0.0;
            for (int lb = 0; lb < L; lb += kRfStage) {
                const int le = lb + kRfStage < L ? lb + kRfStage : L;
                float f[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, gf = 0.0f, df = 0.0f;   // at most kRfStage terms each
                unsigned cnt[4] = {0u, 0u, 0u, 0u};
#pragma unroll 4
                for (int l = lb; l < le; ++l) {
                    const float2 v = AX[l];
                    const bool counts = !SKIP || own.y < v.y || own.y > v.y;
                    pair_term<2, true>(own.x, own.y, v.x, v.y, counts && l != e, g.scale, cnt, f);
                    const float da = own.x - v.x, q = pair_sigmoid(g.scale * (own.y - v.y));
                    gf += counts ? pair_sigmoid(da) - q : 0.0f;                 // the column l == e adds exactly +0
                    df += counts ? rf_decrease_term(da, hown - HS[l], q) : 0.0f;   // and so it does here: h = 0
                }
                a0 += (double)f[0];
                a1 += (double)f[1];
                ga += (double)gf;
                ad += (double)df;
            }
            if (in) {
                G[e] = (float)ga;                      // rounded to fp32 once
                f0 += a0;
                f1 += a1;
                fd += ad;
            }
        }
        f0 = wave_sum_xor(f0);
        f1 = wave_sum_xor(f1);
        fd = wave_sum_xor(fd);
        if (lane == 0) {
            scal[16 + 3 * wave] = f0;
            scal[17 + 3 * wave] = f1;
            scal[18 + 3 * wave] = fd;
        }
        __syncthreads();                               // G and the waves' sums are visible
        colsum(true, uv, gout);
        if (tid == 0) {
            double s0 = 0.0, s1 = 0.0, sd = 0.0, uu = 0.0, up = 0.0, pp = 0.0;
            for (int w = 0; w < NT / 64; ++w) {
                s0 += scal[16 + 3 * w];
                s1 += scal[17 + 3 * w];
                sd += scal[18 + 3 * w];
            }
            for (int k = 0; k < d; ++k) {
                uu = fma(uv[k], uv[k], uu);
                up = fma(u[k], p[k], up);
                pp = fma(p[k], p[k], pp);
            }
            scal[0] = g.coef * (0.5 * (0.6931471805599453 * s0 + s1)) + 0.5 * g.l2 * uu;
            scal[5] = g.coef * (0.5 * sd) + g.l2 * (tt * up + 0.5 * tt * tt * pp);
        }
        __syncthreads();
        return scal[0];
    };

    // Rows [e0, e0 + 64) of V~ into S, zeros past the row's end and past column d.  The caller places the barriers.
    auto stage = [&](int e0) {
        for (int q = tid; q < kRfStage * DK; q += NT) {
            const int j = q / DK, k = q - j * DK;
            S[q] = (e0 + j < L && k < d) ? centred(e0 + j, k) : 0.0f;
        }
    };

    // sum over the pairs e < l of w_el sigmoid'(a_e - a_l) (v~_e - v~_l)(v~_e - v~_l)^T at u: coef times it plus the
    // ridge into H (padding rows and columns carry an identity block), or the sum itself into info[r].
    auto hessian = [&](bool to_info) {
        scores(u, 0.0);
        double hacc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) hacc[a][c] = 0.0;
        for (int I = 0; I < T; ++I) {
            const int e = I * NT + tid;
            const bool live = I * NT + (tid & ~63) < L, in = e < L;
            const float2 own = in ? AX[e] : make_float2(0.0f, 0.0f);
            double zacc[DK], dacc = 0.0;
#pragma unroll
            for (int k = 0; k < DK; ++k) zacc[k] = 0.0;
            for (int l0 = 0; l0 < L; l0 += kRfStage) {
                const int ln = L - l0 < kRfStage ? L - l0 : kRfStage;
                __syncthreads();                       // the previous readers of S are done
                stage(l0);
                __syncthreads();
                if (!live) continue;                   // the wave only helps to stage
                float acc[DK], dg = 0.0f;              // at most kRfStage terms each
#pragma unroll
                for (int k = 0; k < DK; ++k) acc[k] = 0.0f;
                for (int j = 0; j < ln; ++j) {
                    const float2 v = AX[l0 + j];
                    float s = pair_curvature(own.x - v.x);
                    if (SKIP) s = (own.y < v.y || own.y > v.y) ? s : 0.0f;
                    s = l0 + j == e ? 0.0f : s;        // the diagonal
                    dg += s;
                    const float *sr = S + j * DK;
#pragma unroll
                    for (int k = 0; k < DK; ++k) acc[k] = fmaf(s, sr[k], acc[k]);
                }
                dacc += (double)dg;
#pragma unroll
                for (int k = 0; k < DK; ++k) zacc[k] += (double)acc[k];
            }
            // H += V~^T Z over the tile's entries, one wave's 64 entries at a time
            for (int w = 0; w < NT / 64; ++w) {
                const int e0 = I * NT + 64 * w;
                if (e0 >= L) break;
                __syncthreads();                       // the previous readers of S and Zs are done
                if (wave == w) {
#pragma unroll
                    for (int k = 0; k < DK; ++k) {
                        float z = 0.0f;
                        if (in && k < d) z = (float)(dacc * (double)centred(e, k) - zacc[k]);   // rounded to fp32 once
                        Zs[lane * ZLD + k] = z;
                    }
                }
                stage(e0);
                __syncthreads();
                if (hthread) {
                    const int tn = L - e0 < 64 ? L - e0 : 64;
                    for (int t = 0; t < tn; ++t) {
                        const float *sr = S + t * DK + 4 * bi, *zr = Zs + t * ZLD + 4 * bj;
                        double va[4], zc[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            va[a] = (double)sr[a];
                            zc[a] = (double)zr[a];
                        }
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int c = 0; c < 4; ++c) hacc[a][c] = fma(va[a], zc[c], hacc[a][c]);
                    }
                }
            }
        }
        if (hthread) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int hi = 4 * bi + a, hj = 4 * bj + c;
                    if (hi < hj) continue;             // the upper triangle is the mirror image
                    if (to_info) {
                        if (hi < d) {
                            double *out = g.info + (int64_t)r * d * d;
                            out[hi * d + hj] = hacc[a][c];
                            out[hj * d + hi] = hacc[a][c];
                        }
                    } else {
                        const double h = hi < d ? fma(g.coef, hacc[a][c], hi == hj ? g.l2 : 0.0) : (hi == hj ? 1.0 : 0.0);
                        H[hi * LD + hj] = h;
                        H[hj * LD + hi] = h;
                    }
                }
        }
        __syncthreads();
    };

    // p = -H^{-1} gv by Cholesky (fold_cholesky_solve's steps); a pivot that is not positive: p = -gv / mean(diag H).
    auto direction = [&]() {
        if (tid == 0) {
            double tr = 0.0;
            for (int k = 0; k < d; ++k) tr += H[k * LD + k];
            scal[3] = tr / (double)d;
        }
        bool pd = true;
        for (int k = 0; k < DK; ++k) {
            __syncthreads();
            const double dk = H[k * LD + k];
            if (!(dk > 0.0)) {
                pd = false;
                break;
            }
            const double lkk = sqrt(dk);
            if (tid == 0) diag[k] = lkk;
            for (int i = k + 1 + tid; i < DK; i += NT) H[i * LD + k] = H[i * LD + k] / lkk;
            __syncthreads();
            for (int i = k + 1 + (tid / GR); i < DK; i += GR)
                for (int j = k + 1 + (tid % GR); j <= i; j += GR)
                    H[i * LD + j] = fma(-H[i * LD + k], H[j * LD + k], H[i * LD + j]);
        }
        __syncthreads();
        if (!pd) {
            if (tid < DK) p[tid] = tid < d ? -gv[tid] / scal[3] : 0.0;
            __syncthreads();
            return;
        }
        double rhs = tid < DK ? -gv[tid] : 0.0;
        for (int k = 0; k < DK; ++k) {
            if (tid == k) sol[k] = rhs / diag[k];
            __syncthreads();
            if (tid > k && tid < DK) rhs = fma(-H[tid * LD + k], sol[k], rhs);
        }
        rhs = tid < DK ? sol[tid] : 0.0;
        for (int k = DK - 1; k >= 0; --k) {
            if (tid == k) p[k] = rhs / diag[k];
            __syncthreads();
            if (tid < k) rhs = fma(-H[k * LD + tid], p[k], rhs);
        }
        __syncthreads();
    };

    // ---- the row's centre (and the check of its V rows), the start ----
    if (tid < DK) {
        u[tid] = (start && tid < d) ? (double)start[tid] : 0.0;
        mean[tid] = 0.0;
        p[tid] = 0.0;
    }
    __syncthreads();
    if (colsum(false, nullptr, mean)) {                // a V row of this user holds an inf or a NaN
        rf_constant_row(g, r, tid, true, 2, 0.0);
        return;
    }

    double f = value_grad(u, gv, 0.0);
    const double f_start = f;
    int it = 0, status = 1;
    double t = 1.0;
    bool have = false, moved = true;
    for (;;) {                                         // gv and f belong to u
        if (tid == 0) {
            double gg = 0.0, um = 0.0;
            for (int k = 0; k < d; ++k) {
                gg = fma(gv[k], gv[k], gg);
                um = fmax(um, fabs(u[k]));
            }
            scal[1] = sqrt(gg);
            scal[2] = um;
        }
        __syncthreads();
        if (scal[1] <= g.gtol * (g.l2 * scal[2])) {
            status = 0;
            break;
        }
        if (it == g.max_newton) break;
        if (moved || !have) {
            hessian(false);
            direction();
            have = true;
        }
        if (tid < DK) ut[tid] = fma(t, p[tid], u[tid]);
        if (tid == 0) {
            double gp = 0.0;
            for (int k = 0; k < d; ++k) gp = fma(gv[k], p[k], gp);
            scal[4] = gp;
        }
        __syncthreads();
        const double gp = scal[4];
        const double ft = value_grad(ut, gt, t);
        ++it;
        // the Armijo rule on the decrease summed pair by pair or on the two values of f; a NaN trial is a rejected one
        if (fold_armijo_accepts(scal[5], ft, f, t, gp)) {
            if (tid < DK) {
                u[tid] = ut[tid];
                gv[tid] = gt[tid];
            }
            f = ft;
            t = fmin(2.0 * t, 1.0);
            moved = true;
        } else {
            t *= 0.5;
            moved = false;
            if (t < kRfMinStep) break;
        }
        __syncthreads();
    }
    __syncthreads();

    if (g.info) hessian(true);
    for (int k = tid; k < d; k += NT) g.U_out[(int64_t)r * d + k] = (float)u[k];
    if (tid == 0) {
        if (g.objective) {
            g.objective[2 * (int64_t)r] = f_start;
            g.objective[2 * (int64_t)r + 1] = f;
        }
        if (g.grad_ratio) g.grad_ratio[r] = scal[1] / (g.l2 * scal[2]);
        g.iters_status[2 * (int64_t)r] = it;
        g.iters_status[2 * (int64_t)r + 1] = status;
    }
}

template <int DK, bool SKIP>
int rf_launch(RfArgs g, int rows, hipStream_t st)
{
    constexpr size_t lds = rf_lds_bytes(DK);
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)ratings_fold_in_kernel<DK, SKIP>, lds, allowed));
    return pair_chunks(rows, (int)kPairMaxBlocks, [&](int r0, int nr) {
        g.r0 = r0;
        hipLaunchKernelGGL((ratings_fold_in_kernel<DK, SKIP>), dim3((unsigned)nr), dim3(kRfThreads), lds, st, g);
        return (int)hipGetLastError();
    });
}

template <bool SKIP>
int rf_dispatch(const RfArgs &g, int rows, hipStream_t st)
{
    if (g.d <= 4) return rf_launch<4, SKIP>(g, rows, st);
    if (g.d <= 16) return rf_launch<16, SKIP>(g, rows, st);
    if (g.d <= 32) return rf_launch<32, SKIP>(g, rows, st);
    return rf_launch<64, SKIP>(g, rows, st);
}

}  // namespace

extern "C" int mfcd_ratings_fold_in_max_d(void) { return kRfMaxD; }

extern "C" int mfcd_ratings_fold_in_max_len(void) { return kRfMaxLen; }

extern "C" size_t mfcd_ratings_fold_in_workspace_bytes(int rows, int d, int64_t entries)
{
    if (rows < 0 || d < 1 || d > kRfMaxD || entries < 0) return 0;
    return 256;                                        // nothing is staged in HBM: a row's state lives in its workgroup's LDS
}

extern "C" int mfcd_ratings_fold_in_users(const float *V, int m, int d, const int32_t *idx, const float *x, int64_t entries,
                                          const int64_t *row_off, int rows, double scale, int flags, double coef, double l2,
                                          const float *U_init, int max_newton, double gtol, float *U_out, double *objective,
                                          double *grad_ratio, int32_t *iters_status, double *info, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    if (!V || !row_off || !U_out || !iters_status || m < 1 || d < 1 || d > kRfMaxD || rows < 0 || entries < 0) return MFCD_EINVAL;
    if (entries > 0 && (!idx || !x)) return MFCD_EINVAL;
    if (flags & ~MFCD_RAGGED_SKIP_TIES) return MFCD_EINVAL;
    if (!std::isfinite(scale) || !std::isfinite((float)scale)) return MFCD_EINVAL;
    if (!std::isfinite(coef) || !(coef > 0.0) || !std::isfinite(l2) || !(l2 > 0.0)) return MFCD_EINVAL;
    if (!std::isfinite(gtol) || gtol < 0.0 || max_newton < 0 || max_newton > 1000) return MFCD_EINVAL;
    const size_t row_bytes = (size_t)rows * d * sizeof(float), info_bytes = (size_t)rows * d * d * sizeof(double);
    const struct {
        const void *p;
        size_t n;
    } inputs[] = {{V, (size_t)m * d * sizeof(float)},
                  {idx, (size_t)entries * sizeof(int32_t)},
                  {x, (size_t)entries * sizeof(float)},
                  {row_off, ((size_t)rows + 1) * sizeof(int64_t)},
                  {U_init, row_bytes}};
    for (const auto &in : inputs) {
        if (!in.p) continue;
        if (U_out == in.p || (info && info == in.p)) return MFCD_EINVAL;
        if (fold_overlap(U_out, row_bytes, in.p, in.n) || (info && fold_overlap(info, info_bytes, in.p, in.n)))
            return MFCD_EINVAL;
    }
    if (info && ((const void *)info == (const void *)U_out || fold_overlap(info, info_bytes, U_out, row_bytes)))
        return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_ratings_fold_in_workspace_bytes(rows, d, entries)) return MFCD_EWORKSPACE;
    RfArgs g{V,      m,          d,    idx,   x,         entries,    row_off,      0,   (float)scale, coef, l2,
             U_init, max_newton, gtol, U_out, objective, grad_ratio, iters_status, info};
    hipStream_t st = (hipStream_t)stream;
    return flags & MFCD_RAGGED_SKIP_TIES ? rf_dispatch<true>(g, rows, st) : rf_dispatch<false>(g, rows, st);
}
