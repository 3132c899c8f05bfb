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


def model(state, batch, h, step):
    """-> dict: U, V, mU, vU, mV, vV, loss as the step defines them (f64), and "aux": what bounds() reuses."""
    U, V = state["U"].astype(np.float64), state["V"].astype(np.float64)
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    z = np.asarray(batch[3], dtype=np.float64)
    b = len(u)
    with np.errstate(all="ignore"):
        Uu, W = U[u], V[i] - V[j]
        x = (Uu * W).sum(axis=1)
        p, q = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))
        l0, l1 = np.maximum(-np.logaddexp(0.0, -x), -100.0), np.maximum(-np.logaddexp(0.0, x), -100.0)
        term = (z - 1.0) * l1 - z * l0
        pq = p * q
        f = np.where(pq > 0.0, pq / np.maximum(pq, 1e-12), 0.0)
        pz = np.where(z > 0.5, (1.0 - z) - q, p - z)          # p - z without cancellation next to p = 1
        c = pz / b * f
        gU, gV = h["wd"] * U, h["wd"] * V
        np.add.at(gU, u, c[:, None] * W)
        np.add.at(gV, i, c[:, None] * Uu)
        np.add.at(gV, j, -c[:, None] * Uu)
        out = {"loss": float(term.mean())}
        aux = {"x": x, "p": p, "q": q, "f": f, "pz": pz, "c": c, "l0": l0, "l1": l1, "term": term, "b": b}
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


def bounds(state, batch, h, step, form, flavour="ieee", mdl=None):
    """-> dict: absolute error bounds of U, V, mU, vU, mV, vV (arrays) and loss (float) for a step in `form` under
    `flavour`; see the module docstring, whose letters the comments name."""
    mdl = mdl if mdl is not None else model(state, batch, h, step)
    fast_hit, fast_adam = fast_parts(form, flavour)
    a = mdl["aux"]
    U, V = state["U"].astype(np.float64), state["V"].astype(np.float64)
    u, i, j = (np.asarray(t, dtype=np.int64) for t in batch[:3])
    z = np.asarray(batch[3], dtype=np.float64)
    b, d, uu = a["b"], U.shape[1], U32
    x, p, q, f, pz, c = a["x"], a["p"], a["q"], a["f"], a["pz"], a["c"]
    out = {}
    with np.errstate(all="ignore"):
        Uu, W = U[u], V[i] - V[j]
        dx = gamma(d + 2) * (np.abs(Uu) * np.abs(W)).sum(axis=1)                                                  # (X)
        E = (2.0 * np.abs(x) + 2.0 * dx + 2.0) * uu if fast_hit else 2.0 * uu                                     # (S)
        dp = p * q * dx * np.exp(dx) + p * (q * E + (4.0 if fast_hit else 3.0) * uu) + 2.0 ** -124
        dlo, dhi = np.minimum(dp, p), np.minimum(dp, q)          # the interval [p - dlo, p + dhi] inside [0, 1]     (C)
        phiA, phiB = (p - dlo) * (q + dlo), (p + dhi) * (q - dhi)
        phi_lo = np.minimum(phiA, phiB)
        phi_hi = np.where((p - dlo <= 0.5) & (p + dhi >= 0.5), 0.25, np.maximum(phiA, phiB))
        f_lo, f_hi = np.minimum(1.0, phi_lo / 1e-12), np.minimum(1.0, phi_hi / 1e-12)
        cc = 11.0 if fast_hit else 10.0
        dc = (np.abs(pz) * np.maximum(f - f_lo, f_hi - f) + dp * f_hi + cc * uu * (np.abs(pz) + dp) * f_hi) / b + ETA
        ss, bc2s = _scalars(h, step)
        k, kp = (6.0, 5.0) if fast_adam else (4.0, 4.0)
        for T in ("U", "V"):
            P = U if T == "U" else V
            m, v = state["m" + T].astype(np.float64), state["v" + T].astype(np.float64)
            g, m1, v1, den, delta, P1 = a["g" + T], mdl["m" + T], mdl["v" + T], a["den" + T], a["delta" + T], mdl[T]
            S1, S2, hits = np.zeros_like(P), np.zeros_like(P), np.zeros(P.shape[0])                               # (G)
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
            ds = (1.0 + gh) * S1 + gh * S2
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
            for name, val, ref in ((T, dP, P1), ("m" + T, dm, m1), ("v" + T, dv, v1)):
                out[name] = np.where(np.isfinite(ref), SAFETY * val, np.nan)
        l0, l1, term = a["l0"], a["l1"], a["term"]                                                                # (L)
        dl0, dl1 = _dlog(dp, p, l0), _dlog(dp, q, l1)
        dterm = (1.0 - z) * dl1 + z * dl0 + 3.0 * uu * ((1.0 - z) * (np.abs(l1) + dl1) + z * (np.abs(l0) + dl0))
        out["loss"] = SAFETY * float(dterm.mean() + gamma(b + 2) * (np.abs(term) + dterm).mean())
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
