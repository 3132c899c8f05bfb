"""Plain f64 statement of the dense UV^T pass (include/mfcd.h: mfcd_uvt_stats), per-row error bounds derived from the
arithmetic csrc/uvt.hip documents, a numpy fp32 emulation of the tiled form with switchable deliberate errors, and the
input families the CPU and GPU tests share.  numpy only (torch is used for its bf16 rounding).

model(U, V, X, s)         what the pass is defined to return, in f64
bounds(U, V, X, s, form)  how far a correct implementation of `form` may be from it, per row and per output
emulate(...)              the tiled form's arithmetic in numpy fp32 (bounds are validated against it on the CPU)
check(...)                the comparison both test files use: error / bound per row and output, NaN rules, exact zeros

---------------------------------------------------------------------------------------------------------------------
DERIVATION OF THE BOUNDS.  u = 2^-24 (fp32 unit roundoff, round to nearest), u64 = 2^-53, gamma(k) = k u / (1 - k u).
Every line names the place in uvt.hip it follows.  `|.|` of a matrix is elementwise; g = (U V^T)[r][c] exactly.

(P) the product.  ~g is what the kernel holds for g, P = bound on |~g - g|, from A = |U| |V|^T (f64):
    fp32      tile_mfma / the fp32 branch of uvt_tiled_kernel: a chain of d fp32 multiply-adds         P = gamma(d) A
    generic   uvt_main_kernel<0>: `acc[r] += U[..] * vk`, d steps, product and sum may round apart     P = gamma(d+1) A
    split     u = uh + um + du, |du| <= 2^-16 |u| (header comment of uvt_tiled_kernel; likewise v); the kernel adds
              vm uh + vh um + vh uh and drops um vm: three terms of at most 2^-16 |u v| each are missing, and the 3 d
              kept products (each at most (1 + 2^-8)^2 |u v|) are accumulated in fp32          P = (3 2^-16 + 1.01 gamma(3d)) A

(R) the centring vectors (centre_vectors_kernel).  vbar, ubar are f64 column sums stored as fp32 (`bar`), rm[r] =
    fp32(U[r] . vbar), cm[c] = fp32(ubar . V[c]) with f64 accumulation.  Against the model's [3] = fp32(row mean of G):
        B3[r] = u sum_k |U[r][k]| |vbar[k]|      rounding of vbar to fp32
              + 2 u |rm|                         the final rounding, taken as one whole ulp: a value half an ulp from a
                                                 rounding boundary may fall on either neighbour
              + (m + d) u64 sum_k |U[r][k]| mean_c |V[c][k]|     the f64 sums
    The model forms cm with the same two roundings, so only the one-ulp ambiguity of each remains:
        Bcm[c] = 2 u |cm| + 2 u sum_k |ubar[k]| |V[c][k]| + (n + d) u64 sum_k mean_r |U[r][k]| |V[c][k]|

(E) the epilogue, per element (the `tile` lambda of uvt_tiled_kernel; the loop body of uvt_main_kernel):
        a  = fp32(~g - rm)          |a - (g - rm)|  <= da = P + u (|g - rm| + B3 + P)
        c' = fp32(x - x0)           |c' - (x - x0)| <= dc = u |x - x0|          (generic: c = fp32(x - xm), dc = u |x - xm|)
        e  = fp32(fp32(~g - cm) - fp32(s32 x)),  s32 = fp32(s)
                                    |e - (g - cm - s x)| <= de = P + Bcm + u (|g - cm| + P + Bcm) + (u |s| + |s - s32|) |x| + u |e|

(T) the tile sums.  A lane adds its 16 terms of a tile in fp32 (8 fused multiply-adds in each half of a packed pair and
    one addition, or 16 in a row in the ragged tile): at most 16 roundings, each relative to a partial sum of absolute
    values, T = 16 u.  Across tiles, lane halves and splits everything is f64.  For a split with columns C, per row:
        E(S_ac') = sum_C (da |c'| + |a| dc + da dc) + T sum_C (|a| + da)(|c'| + dc)
        E(S_aa)  = sum_C (2 |a| da + da^2)          + T sum_C (|a| + da)^2
        E(S_a)   = sum_C da                         + T sum_C (|a| + da)
        E(S_c')  = sum_C dc                         + T sum_C (|c'| + dc)
        E(S_c'c')= sum_C (2 |c'| dc + dc^2)         + T sum_C (|c'| + dc)^2
    with |a| = |g - rm_model| + B3.  The generic form adds every term in f64: T = 0 there.

(F) finish_row.  sum x = sum_s (S_c' + n_s x0_s), mu = fp32(sum x / m):
        B4 = sum_s E(S_c') / m + 2 u |mu| + K64 (sum |c'| + sum_s n_s |x0_s|) / m
    (2 u |mu|: one whole ulp, as for rm).  With t_s = |mu_model - x0_s| + B4 the re-centring polynomials give
        [0]  sum_s (E(S_ac') + t_s E(S_a))                      ac = s_ac - mu s_a + s_ax0
        [1]  sum_s E(S_aa)
        [2]  sum_s (E(S_c'c') + 2 t_s E(S_c'))                  cc = s_cc - 2 (mu s_c - s_cx0) + (mu^2 n - 2 mu n x0 + n x0^2)
        [5]  sum_s (E(S_c'c') + 2 |x0_s| E(S_c'))               qr = s_cc + 2 s_cx0 + s_nx00
    each plus K64 times the sum of the absolute values of the f64 terms of its polynomial, K64 = (m / 16 + 16) u64
    (one f64 rounding per tile and per term of the polynomial).
    The kernel centres with ITS rm and mu, the model with the model's; with dr = rm_k - rm_model (|dr| <= B3) and
    dm = mu_k - mu_model (|dm| <= B4):
        sum (g - rm_k)(x - mu_k) - sum (g - rm)(x - mu) = -dr sum (x - mu) - dm sum (g - rm) + m dr dm
        sum (g - rm_k)^2 - sum (g - rm)^2               = -2 dr sum (g - rm) + m dr^2
        sum (x - mu_k)^2 - sum (x - mu)^2               = -2 dm sum (x - mu) + m dm^2
    so [0] += B3 |sum (x - mu)| + B4 |sum (g - rm)| + m B3 B4, [1] += 2 B3 |sum (g - rm)| + m B3^2,
    [2] += 2 B4 |sum (x - mu)| + m B4^2; [5] does not depend on either mean.
    Generic form (x_rows_kernel, uvt_final_kernel): xm = fp32(s1 / m), s1, s2 in f64: B4 = 2 u |mu| + K64 mean |x|;
    [2] = s2 - 2 mu s1 + m mu^2 in f64: K64 (sum x^2 + 2 |mu| sum |x| + m mu^2); [5] = s2: K64 sum x^2.

(S) the global sums.  scal[0]: sum over all elements of 2 |e| de + de^2, plus T sum (|e| + de)^2 (tiled), plus
    K64' sum e^2 with K64' = (n m / 16 + 16) u64 bounded by 1e-9.  scal[1] = s^2 sum x^2: s^2 times the sum of the rows'
    [5] bounds (what & 1), or s^2 T sum x^2 for the error-only pass (what = 2 adds x^2 itself in the tile sums).

[3] and [4] are fp32 values: check() also requires that they are representable in fp32.
SAFETY multiplies every bound.  It is chosen against emulate() on the CPU (tests/test_uvt_cpu.py prints the largest
error / bound ratio of the emulation per family; profiles/uvt_accuracy.txt records it), never against the kernel.
---------------------------------------------------------------------------------------------------------------------
"""
import math

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SAFETY = 1.0          # see the end of the derivation; profiles/uvt_accuracy.txt

FORMS = ("fp32", "split", "generic")
MUTATIONS = ("no_shift", "drop_mid_hi", "ragged_mask_off_by_one", "ns_is_cols_per_split", "mean_not_rounded",
             "colmean_for_rowmean")
FAMILIES = ("benign", "offset", "outlier_first", "cancelling", "wide_range", "mixed_rows", "degenerate",
            "degenerate_v0")


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def f32r(a):
    """Round to fp32, return as f64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the plan of csrc/uvt.hip (plan_ws, tiled_shape, run_uvt): which form runs and how the columns are split
# ---------------------------------------------------------------------------------------------------------------------
def tiled_tc(d):
    """Stage width TC of the tiled form, 0 where there is none."""
    return {32: 128, 64: 64, 128: 64, 256: 32}.get(d, 0)


def plan(n, m, d, target_wgs=512, min_stages=8):
    """-> (tiled, cols_per_split, splits) as plan_ws computes them for a pass over n rows."""
    tc = tiled_tc(d) if n >= 32 and m * d < 0x7fff0000 else 0
    if tc:
        row_blocks = (n + 127) // 128
        stages = (m + tc - 1) // tc
        want = (target_wgs + row_blocks - 1) // row_blocks
        by_l2 = (m * d * 4 + (2 << 20) - 1) // (2 << 20)
        want = max(want, by_l2)
        splits = 1 if want <= 1 else (want + 7) // 8 * 8
        max_splits = stages // min_stages if stages // min_stages > 0 else (stages // 2 if stages // 2 > 0 else 1)
        if splits > max_splits:
            splits = max_splits // 8 * 8 if max_splits >= 8 else max_splits
        splits = min(splits, 256)
        per = (stages + splits - 1) // splits
        cps = per * tc
    else:
        rtiles, ctiles, splits = (n + 31) // 32, (m + 31) // 32, 1
        while splits < ctiles and rtiles * splits < 4096:
            splits *= 2
        splits = min(splits, ctiles, 64)
        cps = (ctiles + splits - 1) // splits * 32
    return bool(tc), cps, (m + cps - 1) // cps


def form_for(n, m, d, uvt_split=1, tables_aligned=True, x_aligned=True, target_wgs=512, min_stages=8):
    """-> (form, cols_per_split) run_uvt takes for these arguments."""
    tiled, cps, _ = plan(n, m, d, target_wgs, min_stages)
    if not (tiled and tables_aligned):
        return "generic", cps
    xv = x_aligned and m % 4 == 0
    return ("split" if (uvt_split and xv) else "fp32"), cps


# ---------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------
def _centre_vectors(U, V):
    """(rm, cm) with the roundings of centre_vectors_kernel: fp32 column means, f64 dot, fp32 result (as f64 arrays)."""
    ubar, vbar = f32r(U.mean(axis=0)), f32r(V.mean(axis=0))
    return f32r(U @ vbar), f32r(V @ ubar)


def model(U, V, X, s, rows=None):
    """-> (row_stats f64 [n, 8], scal f64 [4], interval f64 [n, 2, 2]) as include/mfcd.h defines the pass.
    interval[r, k] = (lo, hi): the fp32 neighbours of [3] (k = 0) and [4] (k = 1) the output may fall on.
    rows = slice: what mfcd_uvt_stats_slab returns for those rows of the full U and X (centring vectors from all rows,
    scal = the slab's share)."""
    U, V, X = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (U, V, X))
    Uf = U
    if rows is not None:
        U, X = U[rows], X[rows]
    n, m = X.shape
    with np.errstate(invalid="ignore", over="ignore"):
        G = U @ V.T
        rm, mu = f32r(G.mean(axis=1)), f32r(X.mean(axis=1))
        a, c = G - rm[:, None], X - mu[:, None]
        rs = np.zeros((n, 8))
        rs[:, 0], rs[:, 1], rs[:, 2] = (a * c).sum(axis=1), (a * a).sum(axis=1), (c * c).sum(axis=1)
        rs[:, 3], rs[:, 4], rs[:, 5] = rm, mu, (X * X).sum(axis=1)
        _, cm = _centre_vectors(Uf, V)
        e = G - cm[None, :] - s * X
        scal = np.array([(e * e).sum(), s * s * (X * X).sum(), 0.0, 0.0])
        iv = np.empty((n, 2, 2))
        for k, v in enumerate((rm, mu)):
            v32 = v.astype(np.float32)
            iv[:, k, 0] = np.nextafter(v32, np.float32(-np.inf)).astype(np.float64)
            iv[:, k, 1] = np.nextafter(v32, np.float32(np.inf)).astype(np.float64)
    return rs, scal, iv


def model_two_pass(U, V, X, s):
    """The same quantities by another route (for the CPU tests): centre with the EXACT means, sum, and put the fp32
    rounding of the means back through  sum (a0 - dr)(c0 - dm) = sum a0 c0 + m dr dm  (sum a0 = sum c0 = 0);
    G from a k-loop of outer products; the global sums with math.fsum.  -> (row_stats [n, 8], scal [4])."""
    U, V, X = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (U, V, X))
    n, m = X.shape
    G = np.zeros((n, m))
    for k in range(U.shape[1]):
        G += np.outer(U[:, k], V[:, k])
    rs = np.zeros((n, 8))
    for r in range(n):
        gm, xm = math.fsum(G[r]) / m, math.fsum(X[r]) / m
        rm, mu = float(np.float32(gm)), float(np.float32(xm))
        a0, c0 = G[r] - gm, X[r] - xm
        dr, dm = rm - gm, mu - xm
        rs[r, 0] = math.fsum(a0 * c0) + m * dr * dm
        rs[r, 1] = math.fsum(a0 * a0) + m * dr * dr
        rs[r, 2] = math.fsum(c0 * c0) + m * dm * dm
        rs[r, 3], rs[r, 4] = rm, mu
        rs[r, 5] = math.fsum(c0 * c0) + m * xm * xm
    ubar = np.array([np.float32(math.fsum(U[:, k]) / n) for k in range(U.shape[1])], dtype=np.float64)
    cm = np.array([np.float32(math.fsum(V[c] * ubar)) for c in range(m)], dtype=np.float64)
    e = G - cm[None, :] - s * X
    return rs, np.array([math.fsum((e * e).ravel()), s * s * math.fsum((X * X).ravel()), 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def bounds(U, V, X, s, form, cols_per_split=None, what=3, rows=None):
    """-> (rows f64 [n, 6], scal f64 [2]): absolute error bounds of columns 0-5 per row and of scal[0], scal[1] for a
    pass in `form` ("fp32", "split": tiled; "generic") whose column split is `cols_per_split` (None: one split).
    See the module docstring; the letters below refer to it.  Rows or sums with a non-finite input get a NaN bound
    (check() treats those by the NaN rules).  rows = slice: the bounds of a slab pass over those rows, as in model()."""
    assert form in FORMS
    U, V, X = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (U, V, X))
    Uf = U
    if rows is not None:
        U, X = U[rows], X[rows]
    (n, d), m = U.shape, V.shape[0]
    cps = m if cols_per_split is None else int(cols_per_split)
    u, tiled = U32, form != "generic"
    T = 16.0 * u if tiled else 0.0
    K64 = (m / 16.0 + 16.0) * U64
    s32 = float(np.float32(s))
    with np.errstate(invalid="ignore", over="ignore"):
        G, A = U @ V.T, np.abs(U) @ np.abs(V).T
        P = {"fp32": gamma(d), "generic": gamma(d + 1), "split": 3.0 * 2.0 ** -16 + 1.01 * gamma(3 * d)}[form] * A   # (P)
        aU, aV = np.abs(U), np.abs(V)
        ubar, vbar = Uf.mean(axis=0), V.mean(axis=0)
        _, cm = _centre_vectors(Uf, V)
        rm_m, mu = f32r(G.mean(axis=1)), f32r(X.mean(axis=1))
        B3 = u * (aU @ np.abs(vbar)) + 2.0 * u * np.abs(rm_m) + (m + d) * U64 * (aU @ aV.mean(axis=0))                # (R)
        Bcm = 2.0 * u * np.abs(cm) + 2.0 * u * (aV @ np.abs(ubar)) + (Uf.shape[0] + d) * U64 * (aV @ np.abs(Uf).mean(axis=0))
        absa = np.abs(G - rm_m[:, None]) + B3[:, None]                                                                 # (E)
        da = P + u * (absa + P)
        abse = np.abs(G - cm[None, :] - s * X)
        de = (P + Bcm[None, :] + u * (np.abs(G - cm[None, :]) + P + Bcm[None, :]) + (u * abs(s) + abs(s - s32)) * np.abs(X)
              + u * abse)
        sum_a, sum_c = np.abs((G - rm_m[:, None]).sum(axis=1)), np.abs((X - mu[:, None]).sum(axis=1))
        B = np.zeros((n, 6))
        B[:, 3] = B3
        if tiled:
            starts = list(range(0, m, cps))
            Eac, Eaa, Ea, Ec, Ecc, x0s, cabs = [], [], [], [], [], [], []
            for c0 in starts:                                                                                          # (T)
                sl = slice(c0, min(m, c0 + cps))
                x0 = X[:, c0]
                cp = np.abs(X[:, sl] - x0[:, None])
                dc = u * cp
                a_, da_ = absa[:, sl], da[:, sl]
                Eac.append((da_ * cp + a_ * dc + da_ * dc).sum(axis=1) + T * ((a_ + da_) * (cp + dc)).sum(axis=1))
                Eaa.append((2 * a_ * da_ + da_ * da_).sum(axis=1) + T * ((a_ + da_) ** 2).sum(axis=1))
                Ea.append(da_.sum(axis=1) + T * (a_ + da_).sum(axis=1))
                Ec.append(dc.sum(axis=1) + T * (cp + dc).sum(axis=1))
                Ecc.append((2 * cp * dc + dc * dc).sum(axis=1) + T * ((cp + dc) ** 2).sum(axis=1))
                x0s.append(x0)
                cabs.append((cp.sum(axis=1), (cp * cp).sum(axis=1), (a_ * cp).sum(axis=1), a_.sum(axis=1), float(cp.shape[1])))
            B4 = (sum(Ec) / m + 2.0 * u * np.abs(mu)                                                                   # (F)
                  + K64 * sum(cb[0] + cb[4] * np.abs(x0) for cb, x0 in zip(cabs, x0s)) / m)
            for k in range(len(starts)):
                x0, (s1, s2, sac, sa, ns) = np.abs(x0s[k]), cabs[k]
                t = np.abs(mu - x0s[k]) + B4
                w = np.abs(mu) + B4 + x0
                B[:, 0] += Eac[k] + t * Ea[k] + K64 * (sac + w * sa)
                B[:, 1] += Eaa[k]
                B[:, 2] += Ecc[k] + 2.0 * t * Ec[k] + K64 * (s2 + 2.0 * w * s1 + ns * w * w)
                B[:, 5] += Ecc[k] + 2.0 * x0 * Ec[k] + K64 * (s2 + 2.0 * x0 * s1 + ns * x0 * x0)
            B[:, 1] += K64 * (absa * absa).sum(axis=1)
        else:
            aX = np.abs(X)
            B4 = 2.0 * u * np.abs(mu) + K64 * aX.mean(axis=1)
            cabs_ = np.abs(X - mu[:, None]) + B4[:, None]
            dc = u * cabs_
            B[:, 0] = (da * cabs_ + absa * dc + da * dc).sum(axis=1) + K64 * (absa * cabs_).sum(axis=1)
            B[:, 1] = (2 * absa * da + da * da).sum(axis=1) + K64 * (absa * absa).sum(axis=1)
            x2 = (X * X).sum(axis=1)
            B[:, 2] = K64 * (x2 + 2.0 * np.abs(mu) * aX.sum(axis=1) + m * mu * mu)
            B[:, 5] = K64 * x2
        B[:, 4] = B4
        B[:, 0] += B3 * sum_c + B4 * sum_a + m * B3 * B4
        B[:, 1] += 2.0 * B3 * sum_a + m * B3 * B3
        B[:, 2] += 2.0 * B4 * sum_c + m * B4 * B4
        K64s = (n * m / 16.0 + 16.0) * U64                                                                             # (S)
        S0 = (2 * abse * de + de * de).sum() + T * ((abse + de) ** 2).sum() + K64s * (abse * abse).sum()
        xx = (X * X).sum()
        S1 = s * s * ((T * xx if (tiled and what == 2) else B[:, 5].sum()) + K64s * xx)
    return SAFETY * B, SAFETY * np.array([S0, S1])


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the tiled form
# ---------------------------------------------------------------------------------------------------------------------
def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in f64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _product(U, V, form, mutation):
    """~G [n, m] fp32 as the tiled kernel forms it."""
    n, d = U.shape
    acc = np.zeros((n, V.shape[0]), dtype=np.float32)
    if form == "fp32":      # v_mfma_f32_32x32x2_f32: step kk adds the products k = kk and k = d/2 + kk
        assert d % 2 == 0
        U6, V6 = U.astype(np.float64), V.astype(np.float64)
        for kk in range(d // 2):
            acc = (acc.astype(np.float64) + np.outer(U6[:, kk], V6[:, kk])
                   + np.outer(U6[:, d // 2 + kk], V6[:, d // 2 + kk])).astype(np.float32)
        return acc
    assert d % 16 == 0
    uh, vh = _bf16(U), _bf16(V)
    um, vm = _bf16(U - uh), _bf16(V - vh)
    terms = [(vm, uh), (vh, um), (vh, uh)]         # the kernel's order: small terms first
    if mutation == "drop_mid_hi":
        terms = [(vm, uh), (vh, uh)]
    for kb in range(d // 16):                      # one v_mfma_f32_32x32x16_bf16 per term and k block
        k = slice(16 * kb, 16 * kb + 16)
        for vt, ut in terms:
            acc = (acc.astype(np.float64) + ut[:, k].astype(np.float64) @ vt[:, k].astype(np.float64).T).astype(np.float32)
    return acc


def emulate(U, V, X, s, cols_per_split, form, mutation=None):
    """numpy fp32 emulation of uvt_tiled_kernel<.., WHAT = 3> + finish_row for every row given (use a handful).
    -> (row_stats f64 [n, 8], scal f64 [4]).  `mutation`: one of MUTATIONS, a deliberate error."""
    assert form in ("fp32", "split") and (mutation is None or mutation in MUTATIONS)
    U, V, X = (np.ascontiguousarray(t, dtype=np.float32) for t in (U, V, X))
    (n, d), m = U.shape, V.shape[0]
    cps = int(cols_per_split)
    f4 = np.float32
    rm, cm = (t.astype(f4) for t in _centre_vectors(U.astype(np.float64), V.astype(np.float64)))
    Gt = _product(U, V, form, mutation)
    s32 = f4(s)
    offs = {h: np.array([8 * g + 4 * h + e for g in range(4) for e in range(4)]) for h in (0, 1)}   # acc index r = 4 g + e
    splits = (m + cps - 1) // cps
    part = np.zeros((splits, n, 6))
    err2 = 0.0
    for sp in range(splits):
        c_begin, c_end = sp * cps, min(m, sp * cps + cps)
        x0 = np.zeros(n, dtype=f4) if mutation == "no_shift" else X[:, c_begin].copy()
        acc6 = np.zeros((2, n, 5))                      # per lane half: sac, saa, ssa, ssc, sscc in f64
        for cb in range(c_begin, c_end, 32):
            full = cb + 32 <= c_end
            for h in (0, 1):
                cols = cb + offs[h]
                ld = np.minimum(cols, m - 1)            # clamped loads
                g, x = Gt[:, ld], X[:, ld]
                av = (g - rm[:, None]).astype(f4)
                cv = (x - x0[:, None]).astype(f4)
                centre = rm[:, None] if mutation == "colmean_for_rowmean" else cm[None, ld]
                ev = ((g - centre).astype(f4) - (s32 * x).astype(f4)).astype(f4)
                z = np.zeros(n, dtype=f4)
                if full:    # packed pairs: element 2 j of the 16 goes to the .x sums, 2 j + 1 to the .y sums
                    p = {k: [z.copy(), z.copy()] for k in ("ac", "aa", "e", "a", "c", "cc")}
                    for r in range(16):
                        q = r & 1
                        p["ac"][q] = _fma(av[:, r], cv[:, r], p["ac"][q])
                        p["aa"][q] = _fma(av[:, r], av[:, r], p["aa"][q])
                        p["a"][q] = (p["a"][q] + av[:, r]).astype(f4)
                        p["c"][q] = (p["c"][q] + cv[:, r]).astype(f4)
                        p["cc"][q] = _fma(cv[:, r], cv[:, r], p["cc"][q])
                        p["e"][q] = _fma(ev[:, r], ev[:, r], p["e"][q])
                    t = {k: (v[0] + v[1]).astype(f4) for k, v in p.items()}
                else:       # ragged last tile of the split: per-term masks, one chain
                    lim = c_end + 1 if mutation == "ragged_mask_off_by_one" else c_end
                    t = {k: z.copy() for k in ("ac", "aa", "e", "a", "c", "cc")}
                    for r in range(16):
                        if cols[r] >= lim:
                            continue                   # masked terms are +0
                        t["ac"] = _fma(av[:, r], cv[:, r], t["ac"])
                        t["aa"] = _fma(av[:, r], av[:, r], t["aa"])
                        t["a"] = (t["a"] + av[:, r]).astype(f4)
                        t["c"] = (t["c"] + cv[:, r]).astype(f4)
                        t["cc"] = _fma(cv[:, r], cv[:, r], t["cc"])
                        t["e"] = _fma(ev[:, r], ev[:, r], t["e"])
                for k, name in enumerate(("ac", "aa", "a", "c", "cc")):
                    acc6[h, :, k] += t[name].astype(np.float64)
                err2 += float(t["e"].astype(np.float64).sum())
        part[sp, :, :5] = acc6[0] + acc6[1]
        part[sp, :, 5] = x0.astype(np.float64)
    # finish_row, verbatim
    sx = s_ac = s_a = s_ax0 = aa = s_cc = s_c = s_cx0 = s_n = s_nx0 = s_nx00 = np.zeros(n)
    for sp in range(splits):
        c0 = sp * cps
        ns = float(cps if mutation == "ns_is_cols_per_split" else min(m, c0 + cps) - c0)
        t0, t1, t2, t3, t4, x0 = (part[sp, :, k] for k in range(6))
        sx = sx + (t3 + ns * x0)
        s_ac = s_ac + t0; s_a = s_a + t2; s_ax0 = s_ax0 + x0 * t2
        aa = aa + t1
        s_cc = s_cc + t4; s_c = s_c + t3; s_cx0 = s_cx0 + x0 * t3
        s_n = s_n + ns; s_nx0 = s_nx0 + ns * x0; s_nx00 = s_nx00 + ns * x0 * x0
    mu = sx / m if mutation == "mean_not_rounded" else f32r(sx / m)
    ac = s_ac - mu * s_a + s_ax0
    cc = s_cc - 2.0 * (mu * s_c - s_cx0) + (mu * mu * s_n - 2.0 * mu * s_nx0 + s_nx00)
    qr = s_cc + 2.0 * s_cx0 + s_nx00
    rs = np.zeros((n, 8))
    rs[:, 0], rs[:, 1], rs[:, 2], rs[:, 3], rs[:, 4], rs[:, 5] = ac, aa, np.maximum(0.0, cc), rm.astype(np.float64), mu, qr
    return rs, np.array([err2, float(s) * float(s) * qr.sum(), 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    """error / bound elementwise.  NaN rules: where the model is NaN the output must be NaN, where it is infinite the
    output must not be finite (the shifted sums may turn inf - inf into NaN), where it is finite so must the output be.
    0 / 0 = 0; a broken rule or an error over a zero bound is inf."""
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64))
    out = np.zeros(want.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fin = np.isfinite(want)
        err = np.abs(got - want)
        r = np.where(err == 0.0, 0.0, np.where(bound > 0.0, err / bound, np.inf))
        out[fin] = np.where(np.isfinite(got[fin]), r[fin], np.inf)
        nan = np.isnan(want)
        out[nan] = np.where(np.isnan(got[nan]), 0.0, np.inf)
        inf = np.isinf(want)
        out[inf] = np.where(np.isfinite(got[inf]), np.inf, 0.0)
    return out


def check(got_rows, got_scal, mdl, bnd, what=3):
    """-> (ratio_rows [n, 6], ratio_scal [2], problems: list of str).  `mdl` = model(...), `bnd` = bounds(...).
    problems lists what is wrong beyond a ratio > 1: reserved outputs not exactly zero, [3] / [4] not fp32 values."""
    (rs, sc, _iv), (B, Bs) = mdl, bnd
    problems = []
    rr, rsc = np.zeros((rs.shape[0], 6)), np.zeros(2)
    if what & 1:
        got_rows = np.asarray(got_rows, dtype=np.float64)
        rr = _ratio(got_rows[:, :6], rs[:, :6], B)
        if not (got_rows[:, 6:8] == 0.0).all():
            problems.append("row_stats[:, 6:8] not zero")
        for col in (3, 4):
            v = got_rows[:, col]
            ok = np.isnan(v) | (f32r(v) == v)
            if not ok.all():
                problems.append(f"row_stats[:, {col}] is not an fp32 value in rows {np.flatnonzero(~ok)[:8].tolist()}")
                rr[~ok, col] = np.inf
    if what & 2:
        got_scal = np.asarray(got_scal, dtype=np.float64)
        rsc = _ratio(got_scal[:2], sc[:2], Bs)
        if not (got_scal[2:4] == 0.0).all():
            problems.append("scal[2:4] not zero")
    return rr, rsc, problems


# ---------------------------------------------------------------------------------------------------------------------
# input families (fp32 numpy arrays U [n, d], V [m, d], X [n, m]), seeded, at the caller's shape
# ---------------------------------------------------------------------------------------------------------------------
def family(name, n, m, d, seed=0):
    assert name in FAMILIES, name
    rng = np.random.default_rng([FAMILIES.index(name), n, m, d, seed])
    U = rng.standard_normal((n, d)) / np.sqrt(d)
    V = rng.standard_normal((m, d)) / np.sqrt(d)
    X = rng.standard_normal((n, m)) * 0.5 + rng.uniform(0.1, 0.3, (n, 1))      # "benign": what the older tests feed
    i = np.arange(n)
    if name == "offset":
        # |mean| / std from 1 to 1e5 down the rows; |mean| cycles over 1e-2 .. 1e4 and alternates in sign
        ratio = 10.0 ** (5.0 * i / max(n - 1, 1))
        mag = 10.0 ** ((i * 7 % 13) / 2.0 - 2.0)
        X = ((-1.0) ** i * mag)[:, None] + (mag / ratio)[:, None] * rng.standard_normal((n, m))
    elif name == "outlier_first":
        # every 32nd column (every possible first column of a split) is an outlier of ~2000 standard deviations
        k = X[:, ::32].shape[1]
        X[:, ::32] = ((-1.0) ** i)[:, None] * 1000.0 * (1.0 + rng.uniform(0.0, 1.0, (n, k)))
    elif name == "cancelling":
        # V = one large common component + a small part; U alternates in sign along k, so sum_k |u v| ~ 10 d while
        # |sum_k u v| ~ sqrt(d): g - rm and g - cm are small differences of large numbers
        V = 10.0 + 0.1 * rng.standard_normal((m, d))
        U = ((-1.0) ** np.arange(d))[None, :] * (1.0 + 0.1 * rng.standard_normal((n, d))) + 0.05 * rng.standard_normal((n, 1))
    elif name == "wide_range":
        # entries span 2^-20 .. 2^20 within every row of U and V (products stay below 2^45)
        U = rng.standard_normal((n, d)) * 2.0 ** rng.integers(-20, 21, (n, d))
        V = rng.standard_normal((m, d)) * 2.0 ** rng.integers(-20, 21, (m, d))
    elif name == "mixed_rows":
        sc = 10.0 ** rng.permutation(np.linspace(-6.0, 6.0, n))
        U, X = U * sc[:, None], X * sc[:, None]
    elif name in ("degenerate", "degenerate_v0"):
        for k, val in enumerate((0.0, 0.3, 1000.0)):
            X[k + 1::8] = val            # constant X rows 1, 9, .. / 2, 10, .. / 3, 11, ..
        U[5::8] = 0.0                    # zero U rows
        if n > 6:
            U[1] = 0.0                   # a zero U row against a constant X row
        if name == "degenerate_v0":
            V[:] = 0.0                   # cold start
    return U.astype(np.float32), V.astype(np.float32), X.astype(np.float32)
