"""Plain f64 statement of ONE fused optimiser step (include/mfcd.h: mfcd_train_steps, _bf16, _big; oracle/mfcd_oracle.c),
per-element error bounds derived from the arithmetic the step kernels document, a numpy fp32 restatement of the oracle
with switchable deliberate errors, and the inputs the CPU and GPU tests share.  numpy only (torch is used for its bf16
rounding).

model(state, batch, hyper, step)            what one step is defined to return, in f64: U', V', the four moments, the loss
bounds(state, batch, hyper, step, form, flavour)   how far a correct implementation of that form may be from it, per element
emulate(state, batch, hyper, step, fault)   the oracle's fp32 arithmetic in numpy (the bounds are validated against it)
check(got, mdl, bnd, bf16)                  the comparison both test files use: error / bound per element and output

state = dict(U, V, mU, vU, mV, vV) of fp32 arrays (U, V hold bf16-representable values for bf16 tables); batch =
(u, i, j, z) of ONE step (b = len(u) samples: a short last batch divides by its own length); hyper = dict(lr, beta1,
beta2, eps, wd) as Python floats; step = the 1-based Adam step number of this step.

---------------------------------------------------------------------------------------------------------------------
THE STEP (f64; structure.py:847-851 as oracle/mfcd_oracle.c restates it).
    x_t = U[u_t] . (V[i_t] - V[j_t]),  p_t = sigmoid(x_t),  q_t = 1 - p_t
    loss = mean_t (z_t - 1) max(log q_t, -100) - z_t max(log p_t, -100)                              (bce_term)
    c_t  = (p_t - z_t) / b * f_t,   f_t = p_t q_t / max(p_t q_t, 1e-12)                              (mfcd_orc_grad)
    dU[u_t] += c_t (V[i_t] - V[j_t]),  dV[i_t] += c_t U[u_t],  dV[j_t] -= c_t U[u_t]
    every element of both tables (mfcd_orc_adam; coupled L2, bias corrections from the 1-based step):
    g = d + wd P,  m' = m + (1 - beta1)(g - m),  v' = beta2 v + (1 - beta2) g^2
    ss = lr / (1 - beta1^t),  den = sqrt(v') / sqrt(1 - beta2^t) + eps,  Delta = -ss m' / den,  P' = P + Delta

DERIVATION OF THE BOUNDS.  u = 2^-24 (fp32 unit roundoff), gamma(k) = k u / (1 - k u); "1 ulp" = 2 u relative.  A hat is
what the kernel holds.  Every line names the code it follows.  Constants that count roundings carry one extra u that
absorbs the products of the others (all relative errors here are below 2^-10).  Flavours: streaming.hip is always
"ieee"; resident_kernel.h and big.hip take both the hit path and the Adam update of the flavour mfcd_set_resident_math
selects; local.hip takes only the Adam update from it (its phase A calls sigmoid_f32 / bce_sigmoid_backward_f32).

(X) the score.  streaming.hip phase 1 / common.h wave_score / local.hip phase A / resident_kernel.h `acc += row[0] *
    (row[1] - row[2])` / big.hip `wave_sum64(row[0] * (row[1] - row[2]))`, contraction off (common.h): every product
    passes one subtraction, one multiplication and fewer than d additions whatever the order of the sum:
        dx = gamma(d + 2) sum_k |U[u][k]| |V[i][k] - V[j][k]|
(S) the sigmoid.  |sigma(x + e) - sigma(x)| <= p q |e| exp(|e|) (|d log sigma'/dx| <= 1).  e^ = exp(-x^) has relative
    error E:  ieee (common.h sigmoid_f32: expf, 1 ulp): E = 2 u;  fast (resident_kernel.h / big.hip hit path:
    v_exp_f32 of x * -log2(e)): the constant and the product each round the exponent by u, which moves the result by
    2 u |x|, and v_exp_f32 is 1 ulp: E = (2 |x| + 2 dx + 2) u.  p^ = fl(1 / fl(1 + e^)) moves by q E relatively, by u
    for the addition and by u (IEEE division) or 2 u (train_common.h div_newton: <= 1 ulp) for the quotient:
        dp = p q dx exp(dx) + p (q E + c_s u) + 2^-124,     c_s = 3 (ieee), 4 (fast)
    2^-124: below x = -87 the quotient is subnormal or (fast: v_rcp_f32 result flushed, `e == inf`) zero.
(C) the coefficient (common.h bce_sigmoid_backward_f32; the fast hit path of resident_kernel.h / big.hip).  The clamp
    factor is evaluated over the interval: with phi = p q on [p - dp, p + dp] (concave: its minimum is at an end), f_lo
    = min(1, phi_lo / 1e-12), f_hi likewise.  An interval that reaches p = 1 (fp32: p^ = 1 from x ~ 17 on, then
    (1 - p^) p^ = 0 and g = 0 exactly) has f_lo = 0 and the bound is the whole coefficient: a large bound, no free pass.
    Roundings: 1 / b, p - z, their product, (1 - p) p, the constant 1e-12f, the quotient (1 or 2 u), two products:
        dc = (|p - z| max(f - f_lo, f_hi - f) + dp f_hi + c_c u (|p - z| + dp) f_hi) / b,   c_c = 10 (ieee), 11 (fast)
(G) the row gradients.  A row with h hits in the batch: every term c_t w_t (w = V[i] - V[j] or U[u]) passes one
    subtraction, one multiplication, at most h additions (batch order in streaming.hip phase 1, the claim rounds of
    local.hip, `gr[q] +=` / `lgr[] +=` of resident_kernel.h, the slots of big.hip) and, in the oracle, the addition of
    the separate j-branch tensor.  With S1 = sum_hits dc |w|, S2 = sum_hits |c| |w|:
        ds = (1 + gamma(h + 3)) S1 + gamma(h + 3) S2
    then train_common.h adam_update: g = fmaf(wd, P, d): wd rounded to fp32 and one rounding:
        dg = ds + 2 u |wd P| + u (|g| + ds)
(M) m' = fmaf(w1, g - m, m), w1 = fp32(1 - beta1) (adam_update):  A = (1 - beta1)(dg + 2 u (|g - m| + dg))(1 + 2 u),
        dm = A + u (|m'| + A)
(V) v' = fl(fl(v b2) + fl(fl(w2 g) g)) (adam_update: no fma):  T1 = 2.01 u beta2 v,
    T2 = (1 - beta2)(2 |g| dg + dg^2) + 3.01 u (1 - beta2)(|g| + dg)^2,
        dv = T1 + T2 + u (v' + T1 + T2)
(D) den = fl(fl(sqrt(v^') / bc2s) + eps), as an INTERVAL (no linearisation: v' - dv may reach 0):
        den_lo = (sqrt(max(v' - dv, 0)) / bc2s (1 - k u) - a + eps (1 - u)) (1 - u)
        den_hi = (sqrt(v' + dv) / bc2s (1 + k u) + a + eps (1 + u)) (1 + u)
    ieee (adam_update: sqrtf and an IEEE division, correctly rounded; bc2s rounded from f64 in step_scalars): k = 4, a = 0;
    fast (adam_update_fast: v_sqrt_f32 1 ulp, div_newton 1 ulp): k = 6, and a = 2^-63 / bc2s for an argument below 2^-126
    that v_sqrt_f32 may flush.
(U) Delta^ = fl(fl(nss m^') / den^), nss = fp32(-lr / bc1) (step_scalars):  two roundings and the quotient (1 or 2 u):
        dDelta = ss (dm / den_lo + |m'| max(1 / den_lo - 1 / den, 1 / den - 1 / den_hi)) + k' u ss (|m'| + dm) / den_lo
        k' = 4 (ieee), 5 (fast)
(U2) The interval of (U) treats dm and dv as independent, yet both come from the one g^: next to a fresh state (m' ~ w1
    g, v' ~ w2 g^2) Delta hardly depends on g at all while dm / den_lo is large.  So, also: Delta as a function of g,
        dDelta/dg = -(ss / den^2) (w1 eps + (w1 beta2 v - beta1 w2 m g) / (bc2s sqrt(v')))          (w1 = 1 - beta1 ..)
    (from w1 v' - m' w2 g = w1 beta2 v - beta1 w2 m g), bounded over g +- dg by
        G = (w1 eps + (w1 beta2 v + beta1 w2 |m| (|g| + dg)) / (bc2s sqrt(v_lo))) / den_lo^2,   v_lo = beta2 v + w2 max(|g| - dg, 0)^2
    and the roundings alone around m'(g^), v'(g^): dm_r = dm - w1 dg, dv_r = dv - w2 (2 |g| dg + dg^2),
        dden = min(sqrt(dv_r), dv_r / sqrt(v_lo)) / bc2s + k u sqrt(v' + dv) / bc2s + a + 2 u den_hi
        dDelta2 = ss (G dg + dm_r / den_lo + (|m'| + w1 dg) dden / den_lo^2) + k' u ss (|m'| + dm) / den_lo
    Both hold, so dDelta = min(dDelta, dDelta2).  An element whose g +- dg contains a zero of den - eps keeps a bound of
    the order of lr from either: that is Adam's sign sensitivity, stated per element instead of excused.
    P^' = fl(P + Delta^):  dP = dDelta + u (|P'| + dDelta); a Delta^ that is exactly 0 (dDelta = 0 and Delta = 0) adds
    nothing: dP = 0 and the parameter must be bit-unchanged (lr = 0; an untouched row with wd = 0 and zero moments).
    Results small enough to be subnormal add 2^-140 to dg, dm, dv, dDelta wherever the quantity is not exactly zero.
(B) bf16 tables (streaming.hip store_vec, resident_kernel.h `post`: one round-to-nearest-even of the fp32 result): the
    stored value lies in [rn_bf16(P' - dP), rn_bf16(P' + dP)]: rounding is monotone and dP covers the fp32 intermediate.
(L) the loss (common.h bce_term_f32; streaming.hip batch_mean_kernel, the in-launch means of resident_kernel.h): logf and
    log1pf are 1 ulp, both logs lie in [-100, 0] after the clamp:
        dl0 = -log(1 - dp / p) + 3 u |l0|   (100 + 3 u |l0| where dp >= p / 2),   dl1 likewise with q
        dterm = (1 - z) dl1 + z dl0 + 3 u ((1 - z)(|l1| + dl1) + z (|l0| + dl0))
        dloss = mean dterm + gamma(b + 2) mean (|term| + dterm)

SAFETY multiplies every bound and is 1: tests/test_step_cpu.py prints the largest error / bound of emulate() and of the C
oracle per family and output (profiles/step_accuracy_cpu.txt); a ratio above 1 on the GPU is a finding, not a reason to
raise it.

THE PARTS (evaluation and the split step kernels: csrc/eval.hip, the split entries of csrc/streaming.hip; always
"ieee").  eval_model, coef_model, grad_model, adam_model, apply_model return (model, bounds) of one entry from the same
stage functions model() and bounds() are made of; emu_* are the oracle's fp32 arithmetic with the errors of PART_FAULTS.
(E) evaluation (eval.hip eval_batches_kernel; mfcd_eval_batches, _bf16, _multi).  `p = sigmoid_f32(wave_score(..))`
    (eval.hip:37; common.h wave_score: `acc += ldf(ur, k) * (ldf(vi, k) - ldf(vj, k))`, then wave_sum64) is (X) and (S)
    unchanged: p_out is held to dp.  bf16 tables are widened exactly by ldf (common.h: `(float)p[i]`), so the model takes
    the widened values and (B) does not apply.  `terms[t] = bce_term_f32(p, s.z)` (eval.hip:39) is the dterm of (L).
    `acc += terms[t]` over a lane's samples, wave_sum64, `acc / (float)b` (eval.hip:48-55) are at most b - 1 additions
    and one division of the batch's own b = min(B, N - off) (eval.hip:34): the mean bound of (L) with that b.
    `match[t] = ((p > 0.5f ? 1.0f : 0.0f) == s.z)` (eval.hip:40): a sample with |p - 0.5| > dp is decided, the kernel's
    prediction is the model's, and it matches iff the prediction EQUALS the label (a soft label never does, p = 0.5
    predicts 0).  The count is exact integer arithmetic (wave_sum64_i), so correct_per_batch lies in [lo, lo + a] with
    lo the decided matches and a the undecided samples of the batch.
    Exact zero: if every product U[u][k] (V[i][k] - V[j][k]) is exactly zero (i == j: vi[k] - vj[k] = 0 for finite
    values; a zero U row), every lane's acc is 0, wave_sum64 adds zeros, expf(-0) = 1, 1 + 1 = 2 and 1 / 2 = 0.5 with no
    rounding: dp = 0, p_out must be 0.5 and the sample is decided (prediction 0).
(K) coefficients (streaming.hip coeff_kernel).  The same `sigmoid_f32(wave_score(..))` (streaming.hip:269): p_out is
    held to dp, term_out to dterm; `bce_sigmoid_backward_f32(p, s.z, inv_batch)` with inv_batch = `1.0f /
    (float)batch_divisor` (streaming.hip:398) is (C) with 1 / b replaced by 1 / batch_divisor, the same count of
    roundings: g_out is held to dc(batch_divisor).
(DG) dense gradient (train_step_kernel MODE 1).  Phase 1 recomputes p per hit (streaming.hip:199-201), forms g by
    bce_sigmoid_backward_f32 with inv_batch = 1 / batch_divisor, and accumulates `dst[k] += g * (ldf(vi, k) - ldf(vj,
    k))`, `dst[k] += g * ldf(ur, k)`, `dst[k] += -(g * ldf(ur, k))` (streaming.hip:210-218) in batch order, one wave per
    row; phase 2 stores the LDS value unchanged (`store_vec(G + e, gs)`, streaming.hip:241).  That is (G): gradU, gradV
    are held to ds with dc from (C); a row no sample touches has ds = 0 and must be exactly 0 (streaming.hip:238).
    mfcd_dense_grad_from_coefficients reads `g = g_in[(base + tl) * g_stride]` (streaming.hip:196): the caller's fp32
    value is exact, the model takes it as given, dc = 0 and ds = gamma(h + 3) S2.
(AD) Adam from a dense gradient (MODE 2, mfcd_adam_dense).  `load_vec(G + e, gs)` (streaming.hip:233) reads the dense
    gradient exactly: ds = 0, so dg = 2 u |wd P| + u |g| (+ 2^-140 where not zero) from `fmaf(wd, P, d)`, then (M), (V),
    (D), (U), (U2) of adam_update unchanged.  A NaN gradient element makes m', v', P' NaN; an infinite one makes m', v'
    infinite and P' NaN (num / den = inf / inf); _ratio demands exactly that, and the neighbours' bounds do not widen.
(AS) the step from given coefficients (MODE 0 with g_in, mfcd_apply_step).  (G) with dc = 0 as in (DG), then the chain
    with that ds; the result is copied back by hipMemcpyAsync (streaming.hip:423-424), which changes no bit.  B = 0:
    no hit, ds = 0, the pure weight-decay / moment step of (AD) with a zero gradient.
---------------------------------------------------------------------------------------------------------------------
"""
import os

import numpy as np

U32 = 2.0 ** -24
SAFETY = 1.0
ETA = 2.0 ** -140
TABLES = ("U", "V", "mU", "vU", "mV", "vV")
OUTPUTS = TABLES + ("loss",)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5)
FORMS = ("streaming", "resident", "local", "big", "oracle")
FAULTS = ("drop_second_hit", "stale_second_hit", "short_batch_by_B", "flip_j_sign", "bias_from_step0", "decoupled_wd",
          "skip_untouched", "bf16_truncate", "v_before_wd")
FAMILIES = ("uniform", "dense23", "repeat", "ij_cross", "one_user", "zipf", "soft", "saturated", "fuzz")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def bf16_round(a):
    """Round to the nearest bf16 (ties to even), returned as fp32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def hyper(**kw):
    h = dict(HYPER)
    h.update(kw)
    return h


def fast_parts(form, flavour):
    """-> (fast hit path, fast Adam update) of a form under a flavour (see the head of the derivation)."""
    assert form in FORMS and flavour in ("ieee", "fast")
    fast = flavour == "fast" and form not in ("streaming", "oracle")
    return fast and form in ("resident", "big"), fast


# ---------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------
def _scalars(h, step):
    bc1, bc2 = 1.0 - h["beta1"] ** float(step), 1.0 - h["beta2"] ** float(step)
    return h["lr"] / bc1, np.sqrt(bc2)


def _adam64(P, m, v, g, h, step):
    ss, bc2s = _scalars(h, step)
    m1 = m + (1.0 - h["beta1"]) * (g - m)
    v1 = h["beta2"] * v + (1.0 - h["beta2"]) * g * g
    den = np.sqrt(v1) / bc2s + h["eps"]
    delta = -ss * m1 / den
    return P + delta, m1, v1, den, delta


def _batch64(batch):
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    return u, i, j, np.asarray(batch[3], dtype=np.float64)


def stage_forward(U, V, u, i, j, z):
    """Score, sigmoid and BCE term of every sample (f64 tables) -> dict(Uu, W, x, p, q, l0, l1, term, zero); zero marks
    the samples whose products U[u][k] (V[i][k] - V[j][k]) are all exactly zero."""
    with np.errstate(all="ignore"):
        Uu, W = U[u], V[i] - V[j]
        x = (Uu * W).sum(axis=1)
        p, q = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))
        l0, l1 = np.maximum(-np.logaddexp(0.0, -x), -100.0), np.maximum(-np.logaddexp(0.0, x), -100.0)
        term = (z - 1.0) * l1 - z * l0
        zero = (Uu * W == 0.0).all(axis=1)
    return {"Uu": Uu, "W": W, "x": x, "p": p, "q": q, "l0": l0, "l1": l1, "term": term, "zero": zero}


def stage_coefficient(fw, z, div):
    """The backward coefficient of every sample for a mean over `div` samples -> dict(f, pz, c)."""
    p, q = fw["p"], fw["q"]
    with np.errstate(all="ignore"):
        pq = p * q
        f = np.where(pq > 0.0, pq / np.maximum(pq, 1e-12), 0.0)
        pz = np.where(z > 0.5, (1.0 - z) - q, p - z)          # p - z without cancellation next to p = 1
        c = pz / div * f
    return {"f": f, "pz": pz, "c": c}


def stage_rows(gU, gV, u, i, j, c, Uu, W):
    """The row gradients of the batch added onto gU, gV (which hold wd P, or zeros) in place."""
    with np.errstate(all="ignore"):
        np.add.at(gU, u, c[:, None] * W)
        np.add.at(gV, i, c[:, None] * Uu)
        np.add.at(gV, j, -c[:, None] * Uu)
    return gU, gV


def model(state, batch, h, step):
    """-> dict: U, V, mU, vU, mV, vV, loss as the step defines them (f64), and "aux": what bounds() reuses."""
    U, V = state["U"].astype(np.float64), state["V"].astype(np.float64)
    u, i, j, z = _batch64(batch)
    b = len(u)
    with np.errstate(all="ignore"):
        fw = stage_forward(U, V, u, i, j, z)
        co = stage_coefficient(fw, z, b)
        gU, gV = stage_rows(h["wd"] * U, h["wd"] * V, u, i, j, co["c"], fw["Uu"], fw["W"])
        out = {"loss": float(fw["term"].mean())}
        aux = {k: fw[k] for k in ("x", "p", "q", "l0", "l1", "term")}
        aux.update(co, b=b)
        for T, g in (("U", gU), ("V", gV)):
            P1, m1, v1, den, delta = _adam64(U if T == "U" else V, state["m" + T].astype(np.float64),
                                             state["v" + T].astype(np.float64), g, h, step)
            out[T], out["m" + T], out["v" + T] = P1, m1, v1
            aux["g" + T], aux["den" + T], aux["delta" + T] = g, den, delta
    out["aux"] = aux
    return out


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def _nz(a):
    return ETA * (np.asarray(a) > 0.0)


def _dlog(dp, p, l):
    """(L): how far the clamped log of a value within dp of p may be from l = max(log p, -100)."""
    r = dp / p
    return np.where(r < 0.5, -np.log1p(-np.minimum(r, 0.5)), 100.0) + 3.0 * U32 * np.abs(l)


def bound_forward(Uu, W, x, p, q, d, fast_hit=False):
    """(X), (S) -> (dx, dp) per sample."""
    uu = U32
    with np.errstate(all="ignore"):
        dx = gamma(d + 2) * (np.abs(Uu) * np.abs(W)).sum(axis=1)                                                  # (X)
        E = (2.0 * np.abs(x) + 2.0 * dx + 2.0) * uu if fast_hit else 2.0 * uu                                     # (S)
        dp = p * q * dx * np.exp(dx) + p * (q * E + (4.0 if fast_hit else 3.0) * uu) + 2.0 ** -124
    return dx, dp


def bound_coefficient(p, q, f, pz, dp, div, fast_hit=False):
    """(C) -> dc per sample, for a mean over `div` samples."""
    uu = U32
    with np.errstate(all="ignore"):
        dlo, dhi = np.minimum(dp, p), np.minimum(dp, q)          # the interval [p - dlo, p + dhi] inside [0, 1]     (C)
        phiA, phiB = (p - dlo) * (q + dlo), (p + dhi) * (q - dhi)
        phi_lo = np.minimum(phiA, phiB)
        phi_hi = np.where((p - dlo <= 0.5) & (p + dhi >= 0.5), 0.25, np.maximum(phiA, phiB))
        f_lo, f_hi = np.minimum(1.0, phi_lo / 1e-12), np.minimum(1.0, phi_hi / 1e-12)
        cc = 11.0 if fast_hit else 10.0
        return (np.abs(pz) * np.maximum(f - f_lo, f_hi - f) + dp * f_hi + cc * uu * (np.abs(pz) + dp) * f_hi) / div + ETA


def bound_rows(T, shape, u, i, j, dc, c, Uu, W):
    """(G) -> ds [rows, d] of table T ("U" or "V"): the row gradients summed over a row's hits."""
    with np.errstate(all="ignore"):
        S1, S2, hits = np.zeros(shape), np.zeros(shape), np.zeros(shape[0])                                       # (G)
        if T == "U":
            np.add.at(S1, u, dc[:, None] * np.abs(W))
            np.add.at(S2, u, np.abs(c)[:, None] * np.abs(W))
            np.add.at(hits, u, 1.0)
        else:
            for idx in (i, j):
                np.add.at(S1, idx, dc[:, None] * np.abs(Uu))
                np.add.at(S2, idx, np.abs(c)[:, None] * np.abs(Uu))
                np.add.at(hits, idx, 1.0)
        gh = gamma(hits + 3.0)[:, None]
        return (1.0 + gh) * S1 + gh * S2


def bound_adam(P, m, v, g, m1, v1, den, delta, P1, ds, h, step, fast_adam=False):
    """(M), (V), (D), (U), (U2) -> (dP, dm, dv) of one table from the bound ds of its sparse (or dense) gradient."""
    uu = U32
    ss, bc2s = _scalars(h, step)
    k, kp = (6.0, 5.0) if fast_adam else (4.0, 4.0)
    with np.errstate(all="ignore"):
        dg = ds + 2.0 * uu * np.abs(h["wd"] * P) + uu * (np.abs(g) + ds)
        dg = dg + _nz(dg)
        A = (1.0 - h["beta1"]) * (dg + 2.0 * uu * (np.abs(g - m) + dg)) * (1.0 + 2.0 * uu)                     # (M)
        dm = A + uu * (np.abs(m1) + A)
        dm = dm + _nz(dm)
        T1 = 2.01 * uu * h["beta2"] * v                                                                       # (V)
        T2 = (1.0 - h["beta2"]) * (2.0 * np.abs(g) * dg + dg * dg) + 3.01 * uu * (1.0 - h["beta2"]) * (np.abs(g) + dg) ** 2
        dv = T1 + T2 + uu * (v1 + T1 + T2)
        dv = dv + _nz(dv)
        ab = (2.0 ** -63 / bc2s) * (v1 - dv < 2.0 ** -125) if fast_adam else 0.0                              # (D)
        den_lo = (np.sqrt(np.maximum(v1 - dv, 0.0)) / bc2s * (1.0 - k * uu) - ab + h["eps"] * (1.0 - uu)) * (1.0 - uu)
        den_hi = (np.sqrt(v1 + dv) / bc2s * (1.0 + k * uu) + ab + h["eps"] * (1.0 + uu)) * (1.0 + uu)
        den_lo = np.maximum(den_lo, 0.0)
        mhi = np.abs(m1) + dm                                                                                 # (U)
        dD = ss * (dm / den_lo + np.abs(m1) * np.maximum(1.0 / den_lo - 1.0 / den, 1.0 / den - 1.0 / den_hi)) \
            + kp * uu * ss * mhi / den_lo
        # (U2): through g, whose error m' and v' share; the rounding-only parts of dm and dv; the smaller of the two
        w1, w2, b1, b2 = 1.0 - h["beta1"], 1.0 - h["beta2"], h["beta1"], h["beta2"]
        v_lo = b2 * v + w2 * np.maximum(np.abs(g) - dg, 0.0) ** 2
        num = w1 * b2 * v + b1 * w2 * np.abs(m) * (np.abs(g) + dg)
        G = (w1 * h["eps"] + np.where(num > 0.0, num / (bc2s * np.sqrt(v_lo)), 0.0)) / (den_lo * den_lo)
        dm_r = np.maximum(dm - w1 * dg, 0.0)
        dv_r = np.maximum(dv - w2 * (2.0 * np.abs(g) * dg + dg * dg), 0.0)
        D_r = np.where(dv_r > 0.0, np.minimum(np.sqrt(dv_r), dv_r / np.sqrt(v_lo)), 0.0)
        dden = D_r / bc2s + k * uu * np.sqrt(v1 + dv) / bc2s + ab + 2.0 * uu * den_hi
        dD2 = ss * (G * dg + dm_r / den_lo + (np.abs(m1) + w1 * dg) * dden / (den_lo * den_lo)) + kp * uu * ss * mhi / den_lo
        dD = np.where(np.isnan(dD2), dD, np.fmin(dD, dD2))
        dD = np.where(ss * mhi > 0.0, dD + ETA, 0.0)
        dP = np.where(np.abs(delta) + dD > 0.0, dD + uu * (np.abs(P1) + dD), 0.0)
        return tuple(np.where(np.isfinite(ref), SAFETY * val, np.nan) for val, ref in ((dP, P1), (dm, m1), (dv, v1)))


def bound_term(dp, p, q, l0, l1, z):
    """(L) -> dterm per sample."""
    with np.errstate(all="ignore"):
        dl0, dl1 = _dlog(dp, p, l0), _dlog(dp, q, l1)
        return (1.0 - z) * dl1 + z * dl0 + 3.0 * U32 * ((1.0 - z) * (np.abs(l1) + dl1) + z * (np.abs(l0) + dl0))


def bound_mean(term, dterm):
    """(L) -> the bound of the fp32 mean of one batch's terms (its own length b)."""
    with np.errstate(all="ignore"):
        return SAFETY * float(dterm.mean() + gamma(len(term) + 2) * (np.abs(term) + dterm).mean())


def bounds(state, batch, h, step, form, flavour="ieee", mdl=None):
    """-> dict: absolute error bounds of U, V, mU, vU, mV, vV (arrays) and loss (float) for a step in `form` under
    `flavour`; see the module docstring, whose letters the stage functions name."""
    mdl = mdl if mdl is not None else model(state, batch, h, step)
    fast_hit, fast_adam = fast_parts(form, flavour)
    a = mdl["aux"]
    U, V = state["U"].astype(np.float64), state["V"].astype(np.float64)
    u, i, j, z = _batch64(batch)
    b, d = a["b"], U.shape[1]
    x, p, q, f, pz, c = a["x"], a["p"], a["q"], a["f"], a["pz"], a["c"]
    out = {}
    with np.errstate(all="ignore"):
        Uu, W = U[u], V[i] - V[j]
        dx, dp = bound_forward(Uu, W, x, p, q, d, fast_hit)
        dc = bound_coefficient(p, q, f, pz, dp, b, fast_hit)
        for T in ("U", "V"):
            P = U if T == "U" else V
            m, v = state["m" + T].astype(np.float64), state["v" + T].astype(np.float64)
            ds = bound_rows(T, P.shape, u, i, j, dc, c, Uu, W)
            out[T], out["m" + T], out["v" + T] = bound_adam(P, m, v, a["g" + T], mdl["m" + T], mdl["v" + T], a["den" + T],
                                                            a["delta" + T], mdl[T], ds, h, step, fast_adam)
        out["loss"] = bound_mean(a["term"], bound_term(dp, p, q, a["l0"], a["l1"], z))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatement of oracle/mfcd_oracle.c, with deliberate errors
# ---------------------------------------------------------------------------------------------------------------------
F4 = np.float32


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 values is exact in f64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F4)


def _score32(Uu, Vi, Vj):
    """fwd_one: x += ur[k] * (vi[k] - vj[k]) in order, rows [b, d] -> x [b]."""
    acc = np.zeros(Uu.shape[0], dtype=F4)
    W = (Vi - Vj).astype(F4)
    for kk in range(Uu.shape[1]):
        acc = (acc + (Uu[:, kk] * W[:, kk]).astype(F4)).astype(F4)
    return acc


def _adam32(P, m, v, g, h, step, fault, untouched=None):
    """mfcd_orc_adam on whole tables -> (P', m', v')."""
    t = step - 1 if fault == "bias_from_step0" else step
    with np.errstate(all="ignore"):
        bc1, bc2 = 1.0 - h["beta1"] ** float(t), 1.0 - h["beta2"] ** float(t)
        nss, bc2s = F4(-(np.float64(h["lr"]) / bc1)), F4(np.sqrt(bc2))
        w1, b2, w2, wd, eps = F4(1.0 - h["beta1"]), F4(h["beta2"]), F4(1.0 - h["beta2"]), F4(h["wd"]), F4(h["eps"])
        gs, P0 = g, P
        if fault == "decoupled_wd":
            P = (P * F4(1.0 - h["lr"] * h["wd"])).astype(F4)
        elif h["wd"] != 0.0:
            g = _fma(wd, P, g)
        m1 = _fma(w1, (g - m).astype(F4), m)
        gv = gs if fault == "v_before_wd" else g
        v1 = ((v * b2).astype(F4) + ((w2 * gv).astype(F4) * gv).astype(F4)).astype(F4)
        den = ((np.sqrt(v1).astype(F4) / bc2s).astype(F4) + eps).astype(F4)
        P1 = (P + ((nss * m1).astype(F4) / den).astype(F4)).astype(F4)
    if fault == "skip_untouched" and untouched is not None:
        P1[untouched], m1[untouched], v1[untouched] = P0[untouched], m[untouched], v[untouched]
    return P1, m1, v1


def emulate(state, batch, h, step, fault=None, bf16=False, B=None):
    """One step in the oracle's fp32 arithmetic -> dict(U, V, mU, vU, mV, vV fp32 arrays, loss).  `fault`: one of FAULTS
    (B: the call's batch size, for the fault that divides a short batch by it); bf16: round U', V' to bf16."""
    assert fault is None or fault in FAULTS
    U, V = np.ascontiguousarray(state["U"], dtype=F4), np.ascontiguousarray(state["V"], dtype=F4)
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    z = np.asarray(batch[3], dtype=F4)
    b = len(u)
    div = B if (fault == "short_batch_by_B" and B) else b
    invb = F4(1.0) / F4(div)
    dU, dVi, dVj = np.zeros_like(U), np.zeros_like(V), np.zeros_like(V)
    Uw, Vw = U, V
    stale, drop = fault == "stale_second_hit", fault == "drop_second_hit"
    if stale:
        Uw, Vw = U.copy(), V.copy()
    seen_u, seen_v = set(), set()
    one = F4(1.0)
    with np.errstate(all="ignore"):
        if not stale:
            x_all = _score32(U[u], V[i], V[j])
        terms = np.zeros(b, dtype=F4)
        for t in range(b):
            ut, it, jt = int(u[t]), int(i[t]), int(j[t])
            x = _score32(Uw[ut:ut + 1], Vw[it:it + 1], Vw[jt:jt + 1])[0] if stale else x_all[t]
            p = one / (one + np.exp(-x, dtype=F4))
            l1, l0 = max(np.log1p(-p, dtype=F4), F4(-100.0)), max(np.log(p, dtype=F4), F4(-100.0))
            terms[t] = (z[t] - one) * l1 - z[t] * l0
            den = max((one - p) * p, F4(1e-12))
            g = invb * (p - z[t]) / den * (one - p) * p
            ur, w = Uw[ut], (Vw[it] - Vw[jt]).astype(F4)
            gu = (g * ur).astype(F4)
            if not (drop and ut in seen_u):
                dU[ut] = (dU[ut] + (g * w).astype(F4)).astype(F4)
            if not (drop and it in seen_v):
                dVi[it] = (dVi[it] + gu).astype(F4)
            if not (drop and (jt in seen_v or jt == it)):
                dVj[jt] = (dVj[jt] + (gu if fault == "flip_j_sign" else -gu)).astype(F4)
            seen_u.add(ut)
            seen_v.update((it, jt))
            if stale:      # later samples of the batch read these rows as this step will leave them
                Uw[ut] = _adam32(U[ut], state["mU"][ut], state["vU"][ut], dU[ut], h, step, None)[0]
                for r in (it, jt):
                    Vw[r] = _adam32(V[r], state["mV"][r], state["vV"][r], (dVi[r] + dVj[r]).astype(F4), h, step, None)[0]
        dV = (dVi + dVj).astype(F4)
        s = F4(0.0)
        for t in range(b):
            s = F4(s + terms[t])
        out = {"loss": float(s / F4(b))}
        un_u, un_v = np.ones(U.shape[0], bool), np.ones(V.shape[0], bool)
        un_u[u] = False
        un_v[i] = False
        un_v[j] = False
        for T, P, g, un in (("U", U, dU, un_u), ("V", V, dV, un_v)):
            P1, m1, v1 = _adam32(P, np.asarray(state["m" + T], F4), np.asarray(state["v" + T], F4), g, h, step, fault, un)
            if bf16:
                if fault == "bf16_truncate":
                    P1 = (P1.view(np.uint32) & np.uint32(0xffff0000)).view(F4)
                else:
                    P1 = bf16_round(P1)
            out[T], out["m" + T], out["v" + T] = P1, m1, v1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    """error / bound elementwise.  Where the model is NaN the output must be NaN, where it is infinite the output must
    not be finite, where it is finite so must the output be.  0 / 0 = 0: a zero bound demands equality; a broken rule
    or an error over a zero bound is inf."""
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64))
    with np.errstate(all="ignore"):
        fin = np.isfinite(want)
        err = np.abs(got - want)
        r = np.where(err == 0.0, 0.0, np.where(bound > 0.0, err / bound, np.inf))
        if fin.all() and np.isfinite(err).all():      # the usual case: nothing below applies
            return r
        out = np.zeros(want.shape)
        out[fin] = np.where(np.isfinite(got[fin]), r[fin], np.inf)
        nan = np.isnan(want)
        out[nan] = np.where(np.isnan(got[nan]), 0.0, np.inf)
        inf = np.isinf(want)
        out[inf] = np.where(np.isfinite(got[inf]), np.inf, 0.0)
    return out


def check(got, mdl, bnd, bf16=False):
    """-> dict output -> error / bound (arrays for the six tables, a float for the loss).  A step holds the model iff
    every ratio is <= 1.  bf16 tables (B): the distance from the middle of [rn(P' - dP), rn(P' + dP)] over its half
    width; an interval of one value demands that value."""
    out = {}
    for name in TABLES:
        g = np.asarray(got[name], dtype=np.float64)
        if bf16 and name in ("U", "V"):
            with np.errstate(all="ignore"):
                lo = bf16_round(mdl[name] - bnd[name]).astype(np.float64)
                hi = bf16_round(mdl[name] + bnd[name]).astype(np.float64)
            r = _ratio(g, 0.5 * (lo + hi), 0.5 * (hi - lo))
            r = np.where(bf16_round(g).astype(np.float64) == g, r, np.inf)       # and it is a bf16 value
            out[name] = np.where(np.isfinite(mdl[name]), r, _ratio(g, mdl[name], bnd[name]))
        else:
            out[name] = _ratio(g, mdl[name], bnd[name])
    out["loss"] = float(_ratio(got["loss"], mdl["loss"], bnd["loss"]))
    return out


def worst(ratios):
    """-> [7] the largest ratio per output, in the order of OUTPUTS."""
    return np.array([float(np.max(ratios[k])) for k in OUTPUTS])


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def fuzz_case(replay=False):
    """tools/fuzz_parity.py 400 61, trial 275: n = 7, m = 11, d = 16, B = 64, N = 1462, lr 1e-3, wd 1e-5,
    verbatim -> dict(U, V, u, i, j, z, B, lr, wd).  Read from tests/golden/step_fuzz61_t275.npz; replay = True draws it
    again with the fuzzer's own sequence of generator calls (tests/test_step_cpu.py holds the file to that)."""
    if not replay:
        g = dict(np.load(os.path.join(GOLDEN, "step_fuzz61_t275.npz"), allow_pickle=False))
        return {k: (g[k] if g[k].ndim else g[k].item()) for k in g}
    rng = np.random.default_rng(61)
    for t in range(276):
        d = int(rng.choice([1, 2, 3, 4, 5, 8, 12, 16, 32, 33, 64, 100, 128, 256, 300]))
        n = int(rng.integers(1, 3000)) if rng.random() < 0.8 else int(rng.integers(1, 20))
        m = int(rng.integers(2, 3000)) if rng.random() < 0.8 else int(rng.integers(2, 20))
        B = int(rng.choice([1, 7, 64, 64, 64, 100, 256]))
        N = int(rng.integers(1, 30)) * B + int(rng.integers(0, B))
        soft = bool(rng.random() < 0.3)
        U0 = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
        V0 = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
        u, i = rng.integers(0, n, N), rng.integers(0, m, N)
        if rng.random() < 0.3:
            u[rng.random(N) < 0.5] = 0
            i[rng.random(N) < 0.5] = 0
        j = (i + 1 + rng.integers(0, max(m - 1, 1), N)) % m
        z = rng.integers(0, 5, N) / 4.0 if soft else rng.integers(0, 2, N).astype(np.float64)
        lr, wd = float(rng.choice([1e-3, 1e-2])), float(rng.choice([0.0, 1e-5, 1e-3]))
        rng.integers(0, N // B + 1, 3)
    return dict(U=U0, V=V0, u=u.astype(np.int64), i=i.astype(np.int64), j=j.astype(np.int64), z=z.astype(np.float32),
                B=B, lr=lr, wd=wd)


def family(name, n, m, d, B, N, seed=0):
    """-> dict(U, V fp32 tables; u, i, j int64 [N], z fp32 [N]): N samples in stream order, cut into batches of B.
    "dense23" is the uniform recipe, meant for 2 x 3 (or smaller) tables where every row is hit many times per batch."""
    assert name in FAMILIES, name
    if name == "fuzz":
        g = fuzz_case()
        assert (g["U"].shape, g["V"].shape, g["B"], len(g["u"])) == ((n, d), (m, d), B, N)
        return {k: g[k] for k in ("U", "V", "u", "i", "j", "z")}
    rng = np.random.default_rng([FAMILIES.index(name), n, m, d, B, N, seed])
    U = rng.standard_normal((n, d)) / np.sqrt(d)
    V = rng.standard_normal((m, d)) / np.sqrt(d)
    u, i = rng.integers(0, n, N), rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, max(m - 1, 1), N)) % m
    z = rng.integers(0, 2, N).astype(np.float64)
    if name == "repeat":            # identical triplets within a batch: every sample of a batch is one of two triplets
        k = np.arange(N)
        first = (k // B) * B
        pick = np.where(k % 3 == 0, first, np.minimum(first + 1, N - 1))
        u, i, j = u[pick], i[pick], j[pick]
    elif name == "ij_cross":        # item a is i of the even samples and j of the odd ones of a batch
        a = (np.arange(N) // B) % m
        other = (a + 1 + rng.integers(0, max(m - 1, 1), N)) % m
        even = np.arange(N) % 2 == 0
        i, j = np.where(even, a, other), np.where(even, other, a)
    elif name == "one_user":        # one user for the whole batch
        u = (np.arange(N) // B) % n
    elif name == "zipf":            # a head: half of the references go to row 0 of each table
        u[rng.random(N) < 0.5] = 0
        i[rng.random(N) < 0.5] = 0
        j = (i + 1 + rng.integers(0, max(m - 1, 1), N)) % m
    elif name == "soft":
        z = rng.integers(0, 5, N) / 4.0
    elif name == "saturated":       # |x| ~ 25 |N(0,1)| for a third of the users, ~ 150 |N(0,1)| for another third
        sc = np.array([1.0, 25.0, 150.0])[np.arange(n) % 3] * np.where(np.arange(n) % 3 > 0, np.sqrt(d / 2.0), 1.0)
        U = U * sc[:, None]
    return dict(U=U.astype(np.float32), V=V.astype(np.float32), u=u.astype(np.int64), i=i.astype(np.int64),
                j=j.astype(np.int64), z=z.astype(np.float32))


def preset_state(U, V, step, seed=0):
    """Moments of realistic size for a model that has taken `step` steps: m ~ 3e-5 N(0,1), v ~ 1e-8 and positive
    -> dict(U, V, mU, vU, mV, vV) fp32."""
    rng = np.random.default_rng([7, U.shape[0], V.shape[0], U.shape[1], step, seed])
    st = {"U": np.array(U, dtype=np.float32), "V": np.array(V, dtype=np.float32)}
    for T in ("U", "V"):
        g = 1e-4 * rng.standard_normal(st[T].shape)
        st["m" + T] = (0.3 * g).astype(np.float32)
        st["v" + T] = (g * g * rng.uniform(0.5, 2.0, g.shape) + 1e-12).astype(np.float32)
    return st


def fresh_state(U, V):
    st = {"U": np.array(U, dtype=np.float32), "V": np.array(V, dtype=np.float32)}
    for T in ("U", "V"):
        st["m" + T], st["v" + T] = np.zeros_like(st[T]), np.zeros_like(st[T])
    return st


def batch_of(data, B, k):
    """Batch k of the stream."""
    s = slice(k * B, min((k + 1) * B, len(data["u"])))
    return data["u"][s], data["i"][s], data["j"][s], data["z"][s]


# ---------------------------------------------------------------------------------------------------------------------
# The chains both test files run.  start: 0 fresh, 500 / 10**6 preset moments at that step count; N = (steps - 1) B +
# (short or B); combos: the (flavour, bf16 tables) pairs the GPU test forces for the case.  seed: of the family's
# generator; a case whose first draw held an element with g within a few dg of zero in its first step (a bound above
# 0.05 lr: tests/test_step_cpu.py) was given another draw, not another condition.
# ---------------------------------------------------------------------------------------------------------------------
ALL4 = (("fast", False), ("ieee", False), ("fast", True), ("ieee", True))
COMBOS = {"streaming": (("ieee", False), ("ieee", True)), "local": (("fast", False), ("ieee", False)),
          "big": (("fast", False), ("ieee", False)), "resident": ALL4}


def _c(label, form, n, m, d, B, steps, fam="uniform", short=0, start=0, combos=None, seed=0, **hy):
    return dict(label=label, form=form, n=n, m=m, d=d, B=B, steps=steps, N=(steps - 1) * B + (short or B), family=fam,
                start=start, combos=tuple(combos or COMBOS[form]), seed=seed, hyper=hyper(**hy))


STREAMING = [
    _c("d5", "streaming", 9, 7, 5, 8, 6, "uniform", short=3),
    _c("d100", "streaming", 33, 21, 100, 64, 6, "soft", seed=6),
    _c("d256", "streaming", 20, 17, 256, 64, 6, "zipf", start=500),
    _c("B1", "streaming", 12, 9, 16, 1, 8, "uniform"),
    _c("B200", "streaming", 60, 50, 16, 200, 6, "zipf", short=77),
    _c("B300", "streaming", 40, 300, 8, 300, 6, "ij_cross", short=1),
    _c("2x3x8", "streaming", 2, 3, 8, 64, 8, "dense23", short=5),
    _c("sat", "streaming", 30, 20, 16, 32, 6, "saturated"),
    _c("wd0", "streaming", 40, 30, 8, 4, 6, "uniform", wd=0.0),
    _c("lr0", "streaming", 10, 10, 8, 16, 6, "uniform", lr=0.0, start=500),
    _c("step1e6", "streaming", 12, 10, 16, 16, 6, "one_user", start=10 ** 6),
    _c("multi_wg", "streaming", 700, 500, 16, 64, 6, "repeat"),
    _c("fuzz", "streaming", 7, 11, 16, 64, 23, "fuzz", short=54),
]
LOCAL = [
    _c("2x3x8", "local", 2, 3, 8, 64, 8, "dense23", short=5),
    _c("24x16x100", "local", 24, 16, 100, 64, 6, "soft", short=9),
    _c("50x40x16", "local", 50, 40, 16, 85, 6, "zipf", short=31),
    _c("300x212x16", "local", 300, 212, 16, 64, 6, "ij_cross"),
    _c("one_user", "local", 12, 10, 16, 16, 6, "one_user", start=500),
    _c("repeat", "local", 9, 7, 5, 8, 6, "repeat", start=10 ** 6),
    _c("sat", "local", 30, 20, 16, 32, 6, "saturated"),
    _c("wd0", "local", 40, 30, 8, 4, 6, "uniform", wd=0.0),
    _c("fuzz", "local", 7, 11, 16, 64, 23, "fuzz", short=54),
]


# resident: (Q, d) as resident.hip resident_slices gives it on 256 CUs: Q = 1 up to 262144 elements, 2 up to 524288 (and
# d = 128 below that), 4 for d = 256 up to 524288, 16 up to 2097152, 32 up to 4194304.  rows = n + m.  The look-ahead
# instantiation runs where B <= 64 and n + m >= 96 B (resident_lookahead), the generic one elsewhere.
def _res(Q, d, rows, B, fam="uniform", tag="", **kw):
    n = rows // 2
    c = _c(f"q{Q}d{d}{tag}", "resident", n, rows - n, d, B, 6, fam, **kw)
    c["Q"] = Q
    return c


def _one(k):
    return (ALL4[k % 4],)


RESIDENT = (
    [_res(1, 2, 9, 16, "zipf", "_tiny", short=5), _res(1, 4, 40, 8, "repeat"), _res(1, 8, 1000, 8, "soft"),
     _res(1, 16, 300, 64, "ij_cross", short=9), _res(1, 32, 70, 32, "one_user", start=500),
     _res(1, 64, 2000, 16, "uniform", start=10 ** 6), _res(2, 128, 50, 64, "zipf", seed=6), _res(4, 256, 1600, 8, "uniform"),
     _res(1, 16, 48, 32, "saturated", "_sat"), _res(1, 8, 60, 4, "uniform", "_wd0", wd=0.0),
     _res(1, 16, 18, 64, "fuzz", "_fuzz", short=54)]
    + [_res(2, d, 262144 // d + 64, B, fam, combos=_one(k))
       for k, (d, B, fam) in enumerate(((2, 64, "uniform"), (4, 100, "zipf"), (8, 16, "soft"), (16, 64, "repeat"),
                                        (32, 8, "uniform"), (64, 64, "zipf")))]
    + [_res(16, d, 524288 // d + 64, B, fam, combos=_one(k + 2))
       for k, (d, B, fam) in enumerate(((2, 64, "zipf"), (4, 8, "uniform"), (8, 100, "soft"), (16, 16, "uniform"),
                                        (32, 64, "zipf"), (64, 8, "soft"), (128, 64, "uniform"), (256, 100, "zipf")))]
    + [_res(32, d, 2097152 // d + 64, B, fam, combos=_one(k + 1))
       for k, (d, B, fam) in enumerate(((2, 8, "uniform"), (4, 64, "zipf"), (8, 64, "soft"), (16, 100, "zipf"),
                                        (32, 16, "uniform"), (64, 64, "zipf"), (128, 8, "soft"), (256, 64, "uniform")))]
)
RESIDENT[10].update(n=7, m=11, steps=23, N=1462)
# big: a batch may send at most mfcd_train_big_slots() = 8 row references into one wave's 64 rows (big.hip
# big_check_kernel), so tables of fewer than 64 rows take batches of at most 2 samples
BIG = [
    _c("1x2x64", "big", 1, 2, 64, 2, 8, "dense23", short=1),
    _c("40x30x64", "big", 40, 30, 64, 2, 8, "zipf", start=500),
    _c("16384x16384x64", "big", 16384, 16384, 64, 64, 8, "soft", short=11, seed=6),
]
CASES = STREAMING + LOCAL + RESIDENT + BIG
# the collision-heavy small shapes of the split-invariance test: one call of `steps` steps against `steps` calls of one
SPLIT = [
    _c("2x3x8", "streaming", 2, 3, 8, 64, 21, "dense23", short=5),
    _c("7x11x16", "streaming", 7, 11, 16, 64, 23, "fuzz", short=54),
    _c("2x3x8", "local", 2, 3, 8, 64, 21, "dense23", short=5),
    _c("50x40x16", "local", 50, 40, 16, 85, 21, "zipf", short=31),
    _c("7x11x16", "local", 7, 11, 16, 64, 23, "fuzz", short=54),
    _res(1, 2, 9, 16, "zipf", "_tiny", short=5) | {"steps": 21, "N": 20 * 16 + 5},
    _res(1, 16, 18, 64, "fuzz", "_fuzz", short=54) | {"n": 7, "m": 11, "steps": 23, "N": 1462},
    _res(1, 8, 1000, 8, "zipf", "_look", short=3) | {"steps": 37, "N": 36 * 8 + 3},
    _c("1x2x64", "big", 1, 2, 64, 2, 21, "dense23", short=1),
    _c("40x30x64", "big", 40, 30, 64, 2, 21, "zipf", short=1),
]


def case_id(case):
    return f"{case['form']}-{case['label']}"


def case_inputs(case, bf16=False):
    """-> (data, start state, first step number): the tables are bf16-rounded for bf16 tables."""
    data = family(case["family"], case["n"], case["m"], case["d"], case["B"], case["N"], case["seed"])
    U, V = data["U"], data["V"]
    if bf16:
        U, V = bf16_round(U), bf16_round(V)
    st = preset_state(U, V, case["start"]) if case["start"] else fresh_state(U, V)
    return data, st, case["start"] + 1


# =====================================================================================================================
# THE PARTS: evaluation, coefficients, dense gradient, Adam from a dense gradient, the step from given coefficients
# (csrc/eval.hip, the split entries of csrc/streaming.hip).  All "ieee": neither file has a fast path.  The derivation is
# in the module docstring ((E), (K), (DG), (AD), (AS)); the stage functions above do the arithmetic.
# =====================================================================================================================

PART_FAULTS = ("match_ge_half", "match_rounded_label", "short_batch_by_B", "divisor_ignored", "flip_j_sign",
               "drop_second_hit", "partial_block_unwritten", "seam", "bias_from_step0", "param_not_updated")
PART_FAMILIES = FAMILIES + ("half",)


def plan(n, m, d, aligned=True):
    """streaming.hip make_plan -> (vec, chunks, E): vector access needs d % 4 == 0 and 16-byte aligned arrays."""
    vec = 4 if (d % 4 == 0 and aligned) else 1
    chunks, total = 1, (n + m) * d
    while chunks < 4 and total // (256 * vec * chunks) > 2048:
        chunks *= 2
    return vec, chunks, 256 * vec * chunks


def half_family(n, m, d, B, N, seed=0):
    """The "half" family: samples whose score is exactly zero (i == j; the zero row U[0]) with labels 0, 1 and 0.5,
    samples with x = +-2^-19, +-2^-20 exactly (p - 0.5 = x / 4 is 4 and 2 times the bound: decided), and, from N = 500 on,
    two samples of batch 0 with x = +-2^-24 (inside the bound: undecided).  U rows 0 .. 6 and V rows 0, 1 are special; the
    random samples use the other users."""
    assert n >= 8 and m >= 4
    rng = np.random.default_rng([len(FAMILIES), n, m, d, B, N, seed])
    U = rng.standard_normal((n, d)) / np.sqrt(d)
    V = rng.standard_normal((m, d)) / np.sqrt(d)
    U[:7] = 0.0
    U[1:7, 0] = [2.0 ** -19, -2.0 ** -19, 2.0 ** -20, -2.0 ** -20, 2.0 ** -24, -2.0 ** -24]
    V[:2] = 0.0
    V[0, 0] = 1.0
    u, i = rng.integers(7, n, N), rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, max(m - 1, 1), N)) % m
    z = rng.integers(0, 2, N).astype(np.float64)
    t = np.arange(N)
    lab3 = np.array([0.0, 1.0, 0.5])[(t // 8) % 3]
    same, zrow, near = t % 8 == 1, t % 8 == 3, t % 8 == 5
    j = np.where(same, i, j)
    u = np.where(zrow, 0, u)
    u, i, j = np.where(near, 1 + (t // 8) % 4, u), np.where(near, 0, i), np.where(near, 1, j)
    z = np.where(same | zrow, lab3, np.where(near, ((t // 32) % 2).astype(np.float64), z))
    if N >= 500:
        for pos, row, lab in ((7, 5, 1.0), (15, 6, 1.0)):
            u[pos], i[pos], j[pos], z[pos] = row, 0, 1, lab
    return dict(U=U.astype(np.float32), V=V.astype(np.float32), u=u.astype(np.int64), i=i.astype(np.int64),
                j=j.astype(np.int64), z=z.astype(np.float32))


def part_family(name, n, m, d, B, N, seed=0):
    return half_family(n, m, d, B, N, seed) if name == "half" else family(name, n, m, d, B, N, seed)


def _ratios(got, mdl, bnd, names):
    return {k: _ratio(got[k], mdl[k], bnd[k]) for k in names if got.get(k) is not None}


# ---- evaluation ------------------------------------------------------------------------------------------------------
def _forward_parts(U, V, batch):
    """-> (fw, dp, dterm, z) with the exact-zero rule of (E) applied."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    u, i, j, z = _batch64(batch)
    fw = stage_forward(U, V, u, i, j, z)
    _, dp = bound_forward(fw["Uu"], fw["W"], fw["x"], fw["p"], fw["q"], U.shape[1])
    dp = np.where(fw["zero"], 0.0, dp)
    return fw, dp, bound_term(dp, fw["p"], fw["q"], fw["l0"], fw["l1"], z), z


def eval_model(U, V, data, B):
    """(E) -> (mdl, bnd): mdl = dict(p [N], term [N], loss [nb], correct [nb] the MIDDLE of the admissible interval,
    lo, hi [nb], decided [N], zero [N]); bnd = dict(p, term, loss, correct = half the interval's width)."""
    batch = (data["u"], data["i"], data["j"], data["z"])
    N = len(batch[0])
    fw, dp, dterm, z = _forward_parts(U, V, batch)
    decided = fw["zero"] | (np.abs(fw["p"] - 0.5) > dp)
    match = ((fw["p"] > 0.5).astype(np.float64) == z) & decided
    nb = (N + B - 1) // B
    loss, dloss, lo, hi = np.zeros(nb), np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for k in range(nb):
        s = slice(k * B, min((k + 1) * B, N))
        loss[k], dloss[k] = fw["term"][s].mean(), bound_mean(fw["term"][s], dterm[s])
        lo[k] = match[s].sum()
        hi[k] = lo[k] + (~decided[s]).sum()
    mdl = dict(p=fw["p"], term=fw["term"], loss=loss, correct=0.5 * (lo + hi), lo=lo, hi=hi, decided=decided, zero=fw["zero"])
    return mdl, dict(p=SAFETY * dp, term=SAFETY * dterm, loss=dloss, correct=0.5 * (hi - lo))


def eval_check(got, mdl, bnd):
    """got = dict(loss, and p, correct or None) -> ratios of the outputs that are present."""
    return _ratios(got, mdl, bnd, ("p", "loss", "correct"))


# ---- coefficients ----------------------------------------------------------------------------------------------------
def coef_model(U, V, batch, divisor):
    """(K) -> (mdl, bnd) with keys g, term, p."""
    fw, dp, dterm, z = _forward_parts(U, V, batch)
    co = stage_coefficient(fw, z, divisor)
    dc = bound_coefficient(fw["p"], fw["q"], co["f"], co["pz"], dp, divisor)
    return dict(g=co["c"], term=fw["term"], p=fw["p"]), dict(g=SAFETY * dc, term=SAFETY * dterm, p=SAFETY * dp)


# ---- dense gradient --------------------------------------------------------------------------------------------------
def grad_model(U, V, batch, divisor=None, g=None):
    """(DG) -> (mdl, bnd) with keys gradU, gradV (and term for the entry that computes the coefficients itself).  Give
    `divisor` for mfcd_dense_grad, or the fp32 coefficients `g` for mfcd_dense_grad_from_coefficients."""
    assert (divisor is None) != (g is None)
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    u, i, j, z = _batch64(batch)
    mdl, bnd = {}, {}
    if g is None:
        fw, dp, dterm, z = _forward_parts(U, V, batch)
        co = stage_coefficient(fw, z, divisor)
        c, dc = co["c"], bound_coefficient(fw["p"], fw["q"], co["f"], co["pz"], dp, divisor)
        mdl["term"], bnd["term"] = fw["term"], SAFETY * dterm
    else:
        fw = stage_forward(U, V, u, i, j, z)
        c = np.asarray(g, np.float64)
        dc = np.zeros(len(u))
    mdl["gradU"], mdl["gradV"] = stage_rows(np.zeros_like(U), np.zeros_like(V), u, i, j, c, fw["Uu"], fw["W"])
    for T, P in (("U", U), ("V", V)):
        bnd["grad" + T] = SAFETY * bound_rows(T, P.shape, u, i, j, dc, c, fw["Uu"], fw["W"])
    return mdl, bnd


# ---- Adam from a dense gradient, and the step from given coefficients ------------------------------------------------
def _chain(state, gU, gV, dsU, dsV, h, step):
    mdl, bnd = {}, {}
    with np.errstate(all="ignore"):
        for T, g, ds in (("U", gU, dsU), ("V", gV, dsV)):
            P, m, v = (state[k + T].astype(np.float64) for k in ("", "m", "v"))
            P1, m1, v1, den, delta = _adam64(P, m, v, g, h, step)
            mdl[T], mdl["m" + T], mdl["v" + T] = P1, m1, v1
            bnd[T], bnd["m" + T], bnd["v" + T] = bound_adam(P, m, v, g, m1, v1, den, delta, P1, ds, h, step)
    return mdl, bnd


def adam_model(state, gradU, gradV, h, step):
    """(AD) -> (mdl, bnd) of the six tables after mfcd_adam_dense from the fp32 dense gradients."""
    with np.errstate(all="ignore"):
        gU = h["wd"] * state["U"].astype(np.float64) + np.asarray(gradU, np.float64)
        gV = h["wd"] * state["V"].astype(np.float64) + np.asarray(gradV, np.float64)
    return _chain(state, gU, gV, 0.0, 0.0, h, step)


def apply_model(state, batch, g, h, step):
    """(AS) -> (mdl, bnd) of the six tables after mfcd_apply_step with the fp32 coefficients g (B = 0: empty batch)."""
    U, V = state["U"].astype(np.float64), state["V"].astype(np.float64)
    u, i, j, z = _batch64(batch)
    fw = stage_forward(U, V, u, i, j, z)
    c = np.asarray(g, np.float64)
    gU, gV = stage_rows(h["wd"] * U, h["wd"] * V, u, i, j, c, fw["Uu"], fw["W"])
    ds = [bound_rows(T, P.shape, u, i, j, np.zeros(len(u)), c, fw["Uu"], fw["W"]) for T, P in (("U", U), ("V", V))]
    return _chain(state, gU, gV, ds[0], ds[1], h, step)


def check_tables(got, mdl, bnd):
    return _ratios(got, mdl, bnd, TABLES)


# ---- fp32 emulation of the parts (the oracle's arithmetic), with the deliberate errors of PART_FAULTS ----------------
def emu_forward(U, V, batch):
    """mfcd_orc_forward -> (p, term) fp32."""
    U, V = np.ascontiguousarray(U, dtype=F4), np.ascontiguousarray(V, dtype=F4)
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    z = np.asarray(batch[3], dtype=F4)
    one = F4(1.0)
    with np.errstate(all="ignore"):
        x = _score32(U[u], V[i], V[j])
        p = (one / (one + np.exp(-x, dtype=F4)).astype(F4)).astype(F4)
        l1, l0 = np.maximum(np.log1p(-p, dtype=F4), F4(-100.0)), np.maximum(np.log(p, dtype=F4), F4(-100.0))
        term = (((z - one).astype(F4) * l1).astype(F4) - (z * l0).astype(F4)).astype(F4)
    return p, term


def _mean32(term, div):
    return F4(np.cumsum(term, dtype=F4)[-1] / F4(div))        # cumsum: the serial fp32 sum of mean_terms


def emu_eval(U, V, data, B, fault=None):
    """mfcd_orc_eval_batches -> dict(p [N], loss [nb], correct [nb])."""
    assert fault is None or fault in PART_FAULTS
    p, term = emu_forward(U, V, (data["u"], data["i"], data["j"], data["z"]))
    z = np.asarray(data["z"], dtype=F4)
    if fault == "match_rounded_label":
        z = np.rint(z).astype(F4)
    hard = ((p >= F4(0.5)) if fault == "match_ge_half" else (p > F4(0.5))).astype(F4)
    N = len(p)
    nb = (N + B - 1) // B
    loss, corr = np.zeros(nb, F4), np.zeros(nb, np.int32)
    for k in range(nb):
        s = slice(k * B, min((k + 1) * B, N))
        loss[k] = _mean32(term[s], B if fault == "short_batch_by_B" else s.stop - s.start)
        corr[k] = int((hard[s] == z[s]).sum())
    return dict(p=p, loss=loss, correct=corr)


def emu_coef(U, V, batch, divisor, fault=None):
    """The per-sample part of mfcd_orc_grad -> dict(g, term, p) fp32."""
    assert fault is None or fault in PART_FAULTS
    p, term = emu_forward(U, V, batch)
    z = np.asarray(batch[3], dtype=F4)
    one = F4(1.0)
    invb = one / F4(len(p) if fault == "divisor_ignored" else divisor)
    with np.errstate(all="ignore"):
        pq = ((one - p).astype(F4) * p).astype(F4)
        a = ((invb * (p - z).astype(F4)).astype(F4) / np.maximum(pq, F4(1e-12))).astype(F4)
        g = ((a * (one - p).astype(F4)).astype(F4) * p).astype(F4)
    return dict(g=g, term=term, p=p)


def _occurrence(idx):
    """-> for every entry of idx, how many earlier entries hold the same value."""
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    first = np.r_[True, s[1:] != s[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(s)), 0))
    occ = np.empty(len(s), dtype=np.int64)
    occ[order] = np.arange(len(s)) - start
    return occ


def _scatter32(dst, idx, contrib, drop):
    """index_put_(accumulate=True), serial in batch order, fp32: round r adds every row's hit number r."""
    if not len(idx):
        return
    occ = _occurrence(idx)
    for r in range(int(occ.max()) + 1):
        if drop and r == 1:
            continue
        sel = occ == r
        dst[idx[sel]] = (dst[idx[sel]] + contrib[sel]).astype(F4)


def emu_grad(U, V, batch, g, fault=None, E=None):
    """The scatter of mfcd_orc_grad from fp32 coefficients g -> dict(gradU, gradV) fp32.  E: elements per workgroup (for
    the fault that leaves the partial last block of a table unwritten)."""
    assert fault is None or fault in PART_FAULTS
    U, V = np.ascontiguousarray(U, dtype=F4), np.ascontiguousarray(V, dtype=F4)
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    g = np.asarray(g, dtype=F4)[:, None]
    n = U.shape[0]
    drop = fault == "drop_second_hit"
    with np.errstate(all="ignore"):
        W = (V[i] - V[j]).astype(F4)
        gu = (g * U[u]).astype(F4)
        # the seam fault: rows [n + 1) of one stacked table, hits of V row 0 land in U's last row
        dU, dVi, dVj = np.zeros((n + 1,) + U.shape[1:], F4), np.zeros_like(V), np.zeros_like(V)
        _scatter32(dU, u, (g * W).astype(F4), drop)
        if fault == "seam":
            for idx, c in ((i, gu), (j, -gu)):
                hit = idx == 0
                _scatter32(dU, np.full(int(hit.sum()), n - 1), c[hit], False)
                _scatter32(dVi, idx[~hit], c[~hit], False)
        else:
            _scatter32(dVi, i, gu, drop)
            _scatter32(dVj, j, gu if fault == "flip_j_sign" else -gu, drop)
        out = dict(gradU=dU[:n], gradV=(dVi + dVj).astype(F4))
    if fault == "partial_block_unwritten":
        for k in out:
            flat = out[k].reshape(-1)
            flat[(flat.size // E) * E:] = F4(1.0)
    return out


def emu_adam(state, gradU, gradV, h, step, fault=None, E=None):
    """mfcd_orc_adam on both tables -> dict of the six tables."""
    assert fault is None or fault in PART_FAULTS
    out = {}
    gradU, gradV = np.asarray(gradU, F4), np.asarray(gradV, F4)
    if fault == "seam":
        gradV = gradV.copy()
        gradV[0] = gradU[-1]
    for T, g in (("U", gradU), ("V", gradV)):
        P, m, v = (np.asarray(state[k + T], F4) for k in ("", "m", "v"))
        P1, m1, v1 = _adam32(P, m, v, g, h, step, fault if fault == "bias_from_step0" else None)
        if fault == "param_not_updated":
            P1 = P.copy()
        if fault == "partial_block_unwritten":
            for new, old in ((P1, P), (m1, m), (v1, v)):
                new.reshape(-1)[(new.size // E) * E:] = old.reshape(-1)[(new.size // E) * E:]
        out[T], out["m" + T], out["v" + T] = P1, m1, v1
    return out


def emu_apply(state, batch, g, h, step, fault=None, E=None):
    gr = emu_grad(state["U"], state["V"], batch, g, fault if fault in ("flip_j_sign", "drop_second_hit", "seam") else None)
    return emu_adam(state, gr["gradU"], gr["gradV"], h, step, None if fault == "seam" else fault, E)


# ---- the inputs both test files run ----------------------------------------------------------------------------------
EVAL_ROWS = {1: (300, 290), 2: (41, 40), 3: (97, 53), 63: (64, 50), 64: (70, 45), 65: (45, 60), 100: (120, 80),
             256: (60, 41), 1024: (40, 43), 8: (300, 200)}
EVAL_D = (1, 2, 3, 63, 64, 65, 100, 256, 1024)
EVAL_NB = ((1, 1), (5, 64), (15, 16), (17, 16), (64 * 9 + 5, 64), (1000, 1000))
EVAL_NB_BIG = ((2 * 8192 + 3, 8192), (16384 + 7, 16384))          # at d = 8 only
EVAL_FAMILIES = ("uniform", "soft", "saturated", "half")


def eval_cases():
    """-> [(d, N, B, family)] of the evaluation tests."""
    return [(d, N, B, fam) for d in EVAL_D for N, B in EVAL_NB for fam in EVAL_FAMILIES] + \
        [(8, N, B, fam) for N, B in EVAL_NB_BIG for fam in EVAL_FAMILIES]


# At d = 1024 the worst-case (X) gives dp ~ 1.4e-5 against scores of size sqrt(2 / d) = 0.044: about one random sample in
# 1000 is undecided there, and the first draw of these two inputs put 3 into one batch of 1000: another draw, same cap
EVAL_SEED = {(1024, 1000, 1000, "soft"): 1, (1024, 1000, 1000, "half"): 1}


def eval_input(d, N, B, fam, bf16=False):
    n, m = EVAL_ROWS[d]
    data = part_family(fam, n, m, d, B, N, EVAL_SEED.get((d, N, B, fam), 0))
    if bf16:
        data["U"], data["V"] = bf16_round(data["U"]), bf16_round(data["V"])
    return data


COEF_B = (1, 3, 4, 5, 64, 1001)
COEF_SUBSETS = tuple((bool(k & 1), bool(k & 2), bool(k & 4)) for k in (7, 1, 2, 4, 3, 5, 6, 0))    # (g, term, p) present


def coef_cases():
    """-> [(d, B, divisor, family, (g, term, p present))]: tables of 50 x 40 rows."""
    out = []
    for a, B in enumerate(COEF_B):
        for b, fam in enumerate(EVAL_FAMILIES):
            for c, mult in enumerate((1, 8)):
                k = 8 * a + 2 * b + c
                out.append(((5, 64, 100)[k % 3], B, mult * B, fam, COEF_SUBSETS[(a + 2 * b + c) % 8]))
    return out


GRAD_FAMILIES = ("uniform", "one_user", "repeat", "ij_cross", "half")
GRAD_SHAPES = {3: (300, 200, 64), 5: (300, 200, 64), 4: (300, 290, 64), 255: (37, 23, 32), 1023: (9, 8, 16),
               64: (37, 23, 32), 256: (37, 23, 32), 1024: (9, 8, 16)}        # d -> (n, m, B)


def grad_cases():
    """-> [(label, n, m, d, B, family, seed)]: one batch each.  The streaming shapes of CASES (their own family; batch =
    the whole first batch) and d in {3, 5, 255, 1023} (scalar access, rows that span workgroups) and {4, 64, 256, 1024}
    with every family of GRAD_FAMILIES; last the autograd shape (200, 150, 16) with B = 20000."""
    out = [("stream-" + c["label"], c["n"], c["m"], c["d"], c["B"], c["family"], c["seed"]) for c in STREAMING]
    out += [(f"d{d}-{fam}", n, m, d, B, fam, 0) for d, (n, m, B) in GRAD_SHAPES.items() for fam in GRAD_FAMILIES]
    return out + [("autograd", 200, 150, 16, 20000, "uniform", 0)]


def grad_input(case):
    label, n, m, d, B, fam, seed = case
    if fam == "fuzz":
        data = family("fuzz", n, m, d, B, 1462)
        return {k: (v[:B] if k in "uijz" else v) for k, v in data.items()}
    return part_family(fam, n, m, d, B, B, seed)


def signed_coefficients(B, seed=0):
    """Coefficients for mfcd_dense_grad_from_coefficients / mfcd_apply_step: N(0, 1) / B with exact zeros and values of
    size 1e4 among them."""
    rng = np.random.default_rng([11, B, seed])
    g = rng.standard_normal(B) / B
    g[rng.random(B) < 0.15] = 0.0
    big = rng.random(B) < 0.1
    g[big] = 1e4 * np.sign(rng.standard_normal(int(big.sum())))
    return g.astype(np.float32)


# mfcd_adam_dense: (label, n, m, d, start, hyper, aligned).  The small shapes take every state and both hyper-parameter
# sets; the four multi-chunk shapes (4.2 M elements at most) take one each.
ADAM_SHAPES = (("one_block", 3, 2, 4), ("partial_a", 37, 41, 12), ("partial_b", 300, 7, 100))
ADAM_BIG = (("v4c2", 4100, 4100, 256, 0, {}), ("v4c4", 8200, 8200, 256, 500, {}),
            ("v1c2", 1100, 1100, 251, 10 ** 6, {}), ("v1c4", 2100, 2100, 251, 0, {"lr": 0.0}))


def adam_cases():
    out = [(f"{lab}-s{start}-{'lr0' if hy else 'def'}", n, m, d, start, hyper(**hy), True)
           for lab, n, m, d in ADAM_SHAPES for start in (0, 500, 10 ** 6) for hy in ({}, {"lr": 0.0})]
    out += [(lab, n, m, d, start, hyper(**hy), True) for lab, n, m, d, start, hy in ADAM_BIG]
    return out + [("misaligned", 37, 41, 64, 500, hyper(), False)]


def adam_input(case):
    """-> (state, gradU, gradV, step, special): the gradient mixes normal values, exact zeros, subnormals, values next to
    -wd P and a handful of +-inf and NaN (special: their flat positions per table)."""
    label, n, m, d, start, h, aligned = case
    rng = np.random.default_rng([13, n, m, d, start])
    U = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    st = preset_state(U, V, start) if start else fresh_state(U, V)
    grads, special = [], {}
    for T in ("U", "V"):
        P = st[T]
        g = 1e-3 * rng.standard_normal(P.shape)
        kind = rng.random(P.shape)
        g[kind < 0.10] = 0.0
        sub = (kind >= 0.10) & (kind < 0.15)
        g[sub] = rng.integers(-2 ** 20, 2 ** 20, int(sub.sum())) * 2.0 ** -149
        near = (kind >= 0.15) & (kind < 0.25)
        g[near] = (-h["wd"] * P.astype(np.float64) * (1.0 + 1e-5 * rng.standard_normal(P.shape)))[near]
        g = g.astype(np.float32)
        flat = g.reshape(-1)
        pos = rng.choice(flat.size, size=min(6, flat.size // 3), replace=False)
        flat[pos] = np.array([np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf], dtype=np.float32)[:len(pos)]
        grads.append(g)
        special[T] = np.sort(pos)
    return st, grads[0], grads[1], start + 1, special
