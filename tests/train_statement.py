"""The float64 statements of the association head's TRAINING path: the eight autograd Functions of gomatching_amd/training.py and
the four kernels of csrc/train.hip, each with an ELEMENTWISE derived error bound, and the inputs and case tables that
tests/test_train_statement_cpu.py (no GPU: the statements against torch's float64 autograd, an fp32 emulation inside every bound,
planted mistakes outside it) and tests/test_train_forms_gpu.py (the real Functions and the `ops` wrappers on every case) share.
No test in here.  Written from the contract in include/gomatching_hip.h ("Training of the association head", "Training-mode
dropout") and the Functions' docstrings; gomatching_amd.training is never imported.

Every statement takes float32 inputs, widens them exactly, evaluates in float64 and returns {name: (exp, bound)}.  The forward
AND the backward are written out as formulas, because a bound has to follow the steps; that the written-out backward IS the
derivative is checked against torch's float64 autograd of the forward alone (`*_autograd` below), which is the statement of
every backward.  Bounds are carried as an elementwise absolute error d through the steps, U = 2^-24:

  one fp32 operation       exact result v from operands with errors: the propagated error e, then + U (|v| + e)    (`_rnd`)
  fp32 product of depth K  y = a w^T (+ b):   d = (K + GEMM_C) U (|a| + da)(|w| + dw)^T + U |b|-part + da |w|^T + |a| dw^T + da dw^T
                           worst case and order-free: whatever the order (tile loop, split-K partial sums and their reduction,
                           MFMA accumulation) a term passes through at most K roundings.  GEMM_C = 2: the bias addition and the
                           store's own rounding of the epilogue.  K is the PADDED depth the launch runs over (pad4).
  ReLU and its mask        1-Lipschitz forward.  The backward's mask y > 0 is a discontinuity: where 0 < |pre| <= d_pre the
                           two sides may decide differently and the bound of the masked gradient is |dy| itself (`undecided`);
                           a pre-activation that is exactly 0 (a zero row against a zero bias) is exact on every side.
  dropout                  mask * scale is one more fp32 product; the mask stream is dropout_statement's (exact).
  expf                     asso_statement.EXPF (2 ulp).
  logf                     LOGF = 4 U: 2 ulp, dec_statement's figure for the same device function.
  log1pf, powf             LOG1PF = POWF = LOGF.  The rule beside EXPF is "twice the device library's documented ulp"; no document
                           available to this project states a figure for either, so the SECOND rule is used: logf's figure.
  softmax (attention)      softmax_bg64's derivation without the background: v_j = fl(scale s_j) carries E = scale d_s + U |v|;
                           rel_j = (|v_j - m| + EXPF) U + its p-weighted mean + (ceil(n / 256) + 12) U + 2 max_j E_j; the 12:
                           six butterfly steps, three additions of the waves' sums, the reciprocal, the product, one spare.
  softmax backward         dot = sum_j g_j p_j (a lane's ceil(cols / 64) fused multiply-adds + six butterfly steps), t = g - dot,
                           dS = (scale p) t: every step through `_rnd` with the errors of p and g it is handed.
  asso_ce                  gradient: asso_statement.softmax_bg64 (the same operation) times |grad_scale|, plus the subtraction of
                           the one-hot and the product with grad_scale.  loss = (m + logf(Z)) - l_target with Z = sum_j exp(l_j -
                           m) + exp(-m) in [1, n + 1]: Z's relative error (softmax_bg64's `rbar` + (ceil(n / 64) + 7) U + n 2^-126)
                           is the absolute error of its logarithm, + LOGF U |log Z|, + the two additions.
                           target > n_t is outside the contract (the host never forms one): not stated, not tested.
  sigmoid focal            s = (2t - 1) x is exact.  e = expf(-|s|), l = log1pf(e) (slope <= 1), nlp = max(-s, 0) + l,
                           pt = expf(-nlp): relative error d_nlp + EXPF U.  om = 1 - pt keeps pt's ABSOLUTE error: the
                           cancellation term.  mod = powf(om, gamma): the largest change of x^gamma over [om - d, om + d] (the
                           error of pt divided by 1 - pt, raised through powf, in closed form) + POWF U mod; gamma = 0 gives
                           exactly 1, powf(0, 0) included.  No saturated element is excluded.
  sums of losses           a product of depth pad4(count) against ones.

Nothing in a bound is measured and nothing is taken from the code under test.
"""
import math

import numpy as np
import torch

import asso_statement as A
import dropout_statement as D

U = A.U
TINY = A.TINY
EXPF = A.EXPF
LOGF = 4                                              # logf: 2 ulp = 4 U (dec_statement.py, inverse_sigmoid)
LOG1PF = LOGF                                         # no documented figure: logf's (the second rule of the issue)
POWF = LOGF                                           # the same
GEMM_C = 2
STREAM = (7, 3, 5, 1)                                 # (seed, site, iteration, rank) of the Function-level dropout cases
P_DROP = 0.3                                          # so that a 3 x 5 weight matrix holds dropped and kept elements


def pad4(n):
    return (n + 3) // 4 * 4


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _rnd(v, e=0.0):
    """The error of one fp32 operation whose exact result is v and whose operands bring the propagated error e."""
    return e + U * (np.abs(v) + e)


def _mul(a, da, b, db):
    v = a * b
    return v, _rnd(v, np.abs(a) * db + np.abs(b) * da + da * db)


def _sub(a, da, b, db):
    v = a - b
    return v, _rnd(v, da + db)


def gemm64(a, da, w, dw, bias=None, depth=None):
    """y = a w^T (+ bias): a [M, K], w [N, K] float64 with errors da, dw (arrays or 0.0) -> (y, d).  depth: the padded K."""
    K = a.shape[1]
    depth = pad4(K) if depth is None else depth
    aa, ww = np.abs(a), np.abs(w)
    da = np.broadcast_to(np.asarray(da, np.float64), a.shape)
    dw = np.broadcast_to(np.asarray(dw, np.float64), w.shape)
    y = a @ w.T
    mag = (aa + da) @ (ww + dw).T
    d = aa @ dw.T + da @ ww.T + da @ dw.T
    if bias is not None:
        y = y + bias
        mag = mag + np.abs(bias)
    return y, d + (depth + GEMM_C) * U * mag


def sum64(v, dv):
    """The sum of a handful of values as a product against ones of depth pad4(count)."""
    v, dv = np.asarray(v, np.float64).reshape(-1), np.asarray(dv, np.float64).reshape(-1)
    return v.sum(), dv.sum() + (pad4(v.size) + GEMM_C) * U * (np.abs(v) + dv).sum()


def mask_mult(shape, p, stream=STREAM):
    """mask * scale of the logical tensor `shape` on `stream`, float64 of the float32 scale; p None: ones."""
    if p is None:
        return np.ones(shape)
    n = int(np.prod(shape))
    return (D.keep_mask(*stream, n, p).astype(np.float64) * float(D.scale_f32(p))).reshape(shape)


def worst(got, exp, bound):
    """(largest |got - exp| / bound, flat index); 0 / 0 counts as 0, x / 0 with x > 0 and a NaN as infinite."""
    got, exp, bound = np.asarray(got, np.float64), np.asarray(exp, np.float64), np.asarray(bound, np.float64)
    assert got.shape == exp.shape == bound.shape, (got.shape, exp.shape, bound.shape)
    if got.size == 0:
        return 0.0, 0
    err = np.abs(got - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r).reshape(-1)
    at = int(r.argmax())
    return float(r[at]), at


# ------------------------------------------------------------------------------------------ Linear, LinearReluDrop
def linear64(x, w, b, relu, dy, mult=None, scale=1.0):
    """y = [mult *] act(x W^T + b) and the gradients of sum(y * dy): x [M, K], w [N, K], b [N] or None, dy [M, N]; mult
    [M, N] = mask * scale of LinearReluDrop (relu is then True; `scale` = the float32 1 / (1 - p)).  -> {"y", "dx", "dw", "db" (with b)}: (exp, bound).
    Depths: forward K, dx pad4(N), dw and db pad4(M).  M = 0: zeros of the right shapes, bound 0."""
    x, w, dy = f64(x), f64(w), f64(dy)
    b = None if b is None else f64(b)
    M, K = x.shape
    N = w.shape[0]
    if M == 0:
        z = lambda *s: (np.zeros(s), np.zeros(s))
        out = {"y": z(0, N), "dx": z(0, K), "dw": z(N, K)}
        if b is not None:
            out["db"] = z(N)
        return out
    pre, dpre = gemm64(x, 0.0, w, 0.0, bias=b, depth=K)
    y, dy_ = (np.maximum(pre, 0.0), dpre) if relu else (pre, dpre)
    g, dg = dy, np.zeros_like(dy)
    if mult is not None:
        y, dy_ = _mul(y, dy_, mult, 0.0)
        g, dg = _mul(dy, 0.0, np.full_like(dy, scale), 0.0)
    if relu:
        keep = (pre > 0) if mult is None else ((pre > 0) & (mult > 0))
        undecided = (pre != 0) & (np.abs(pre) <= dpre) & (True if mult is None else (mult > 0))
        dg = np.where(undecided, np.abs(g) + dg, np.where(keep, dg, 0.0))
        g = np.where(keep, g, 0.0)
    out = {"y": (y, dy_), "dx": gemm64(g, dg, w.T, 0.0, depth=pad4(N)), "dw": gemm64(g.T, dg.T, x.T, 0.0, depth=pad4(M))}
    if b is not None:
        v, d = gemm64(g.T, dg.T, np.ones((1, M)), 0.0, depth=pad4(M))
        out["db"] = (v[:, 0], d[:, 0])
    return out


def linear_autograd(x, w, b, relu, dy, mult=None):
    """torch float64 autograd of the forward alone: the statement of the backward."""
    t = lambda a: None if a is None else torch.from_numpy(f64(a)).requires_grad_()
    xt, wt, bt = t(x), t(w), t(b)
    y = xt @ wt.T
    if bt is not None:
        y = y + bt
    if relu:
        y = torch.relu(y)
    if mult is not None:
        y = y * torch.from_numpy(mult)
    (y * torch.from_numpy(f64(dy))).sum().backward()
    g = lambda a: np.zeros(tuple(a.shape)) if a.grad is None else a.grad.numpy()
    out = {"y": y.detach().numpy(), "dx": g(xt), "dw": g(wt)}
    if bt is not None:
        out["db"] = g(bt)
    return out


LINEAR_M = (0, 1, 3, 4, 5)
LINEAR_N = (1, 2, 3, 4, 5, 8)
LINEAR_K = (4, 8, 36)
LINEAR_CASES = [(M, N, K, bias, relu) for M in LINEAR_M for N in LINEAR_N for K in LINEAR_K for bias in (True, False)
                for relu in (True, False)]
SEAM = (1024, 256)                                    # (N, K) of the seam pair: N K = 2^18; M = 128 (split-K dgrad), 129 (tile)
SEAM_M = (128, 129)


def linear_inputs(M, N, K, bias, seed=0):
    """x, w, b, dy float32.  With M >= 3 row 1 of x is zero: its pre-activation is exactly b (or exactly 0 without one); b[0] = 0
    and the other biases alternate in sign, so that row holds an exact 0 and values of both signs.  The rows are a function of
    the row index alone, so that M = 128 and M = 129 of the seam pair share their first 128."""
    rows = [_rng(11, N, K, seed, i).standard_normal(K + N) for i in range(M)]
    r = np.array(rows).reshape(M, K + N)
    x, dy = r[:, :K].copy(), r[:, K:].copy()
    if M >= 3:
        x[1] = 0.0
    g = _rng(12, N, K, seed)
    w = g.standard_normal((N, K)) / math.sqrt(K)
    b = None
    if bias:
        b = 0.25 * (1 + np.arange(N) % 3) * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        b[0] = 0.0
    f = lambda a: None if a is None else a.astype(np.float32)
    return f(x), f(w), f(b), f(dy)


# ------------------------------------------------------------------------------------------ softmax and its backward
def softmax64(s, ds, scale):
    """Rows of softmax(scale s) over the last axis with the error ds of s -> (p, dp)."""
    n = s.shape[-1]
    v = s * scale
    E = _rnd(v, ds * scale).max(-1, keepdims=True)
    m = v.max(-1, keepdims=True)
    e = np.exp(v - m)
    p = e / e.sum(-1, keepdims=True)
    r = (np.abs(v - m) + EXPF) * U
    rel = r + (p * r).sum(-1, keepdims=True) + (-(-n // 256) + 12) * U + 2 * E
    return p, p * np.expm1(rel) + TINY


def softmax_bwd64(p, dp, g, dg, scale):
    """dS = scale p (g - sum_j g_j p_j) over the last axis, from p and g with errors dp, dg -> (dS, d)."""
    cols = p.shape[-1]
    dp, dg = np.broadcast_to(dp, p.shape), np.broadcast_to(dg, g.shape)
    dot = (g * p).sum(-1, keepdims=True)
    ddot = (dg * np.abs(p) + np.abs(g) * dp + dg * dp).sum(-1, keepdims=True) \
        + (-(-cols // 64) + 6) * U * ((np.abs(g) + dg) * (np.abs(p) + dp)).sum(-1, keepdims=True)
    t, dt = _sub(g, dg, dot, ddot)
    sp, dsp = _mul(p, dp, np.full_like(p, scale), 0.0)
    return _mul(sp, dsp, t, dt)


SOFTMAX_ROWS = (1, 4, 5)
SOFTMAX_COLS = (1, 63, 64, 65, 130)
SOFTMAX_CASES = [(r, c) for r in SOFTMAX_ROWS for c in SOFTMAX_COLS]
SOFTMAX_SCALE = float(np.float32(1.0 / math.sqrt(8.0)))


def softmax_ld(cols):
    return cols if cols % 4 == 0 else pad4(cols) + 4


def softmax_bwd_inputs(rows, cols):
    """P (rows of a softmax of logits x 3, rounded to float32) and dP, [rows, cols] float32."""
    g = _rng(21, rows, cols)
    s = 3 * g.standard_normal((rows, cols))
    e = np.exp(s - s.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32), g.standard_normal((rows, cols)).astype(np.float32)


def softmax_bwd_case64(P, dP, scale=SOFTMAX_SCALE):
    return softmax_bwd64(f64(P), 0.0, f64(dP), 0.0, scale)


# ------------------------------------------------------------------------------------------ Attention, AttentionDrop
def attention64(q, k, v, heads, do, mult=None):
    """softmax(q_h k_h^T / sqrt(hd)) v_h per head, heads side by side in E, and the gradients of sum(out * do).  q [Lq, E],
    k, v [Lk, E], do [Lq, E] float32; mult [heads, Lq, Lk] = mask * scale on the weights (AttentionDrop) or None.
    -> {"out", "P" [heads, Lq, pad4(Lk)] (the saved, UNDROPPED weights; padding columns 0 with bound 0), "dq", "dk", "dv"}.
    Depths: logits hd, out and dq pad4(Lk), dv and dk pad4(Lq), dP hd.  Lq = 0 or Lk = 0: zeros, bound 0."""
    q, k, v, do = f64(q), f64(k), f64(v), f64(do)
    Lq, E = q.shape
    Lk = k.shape[0]
    hd = E // heads
    Lkp, Lqp = pad4(Lk), pad4(Lq)
    scale = float(np.float32(1.0 / math.sqrt(hd)))
    z = lambda *s: [np.zeros(s), np.zeros(s)]
    out, P, dq, dk, dv = z(Lq, E), z(heads, Lq, Lkp), z(Lq, E), z(Lk, E), z(Lk, E)
    if Lq and Lk:
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            s, ds = gemm64(q[:, c], 0.0, k[:, c], 0.0, depth=hd)
            p, dp = softmax64(s, ds, scale)
            P[0][h, :, :Lk], P[1][h, :, :Lk] = p, dp
            pd, dpd = (p, dp) if mult is None else _mul(p, dp, mult[h], 0.0)
            out[0][:, c], out[1][:, c] = gemm64(pd, dpd, v[:, c].T, 0.0, depth=Lkp)
            dv[0][:, c], dv[1][:, c] = gemm64(pd.T, dpd.T, do[:, c].T, 0.0, depth=Lqp)
            g, dg = gemm64(do[:, c], 0.0, v[:, c], 0.0, depth=hd)
            if mult is not None:
                g, dg = _mul(g, dg, mult[h], 0.0)
            s_, ds_ = softmax_bwd64(p, dp, g, dg, scale)
            dq[0][:, c], dq[1][:, c] = gemm64(s_, ds_, k[:, c].T, 0.0, depth=Lkp)
            dk[0][:, c], dk[1][:, c] = gemm64(s_.T, ds_.T, q[:, c].T, 0.0, depth=Lqp)
    return {"out": tuple(out), "P": tuple(P), "dq": tuple(dq), "dk": tuple(dk), "dv": tuple(dv)}


def attention_autograd(q, k, v, heads, do, mult=None):
    t = lambda a: torch.from_numpy(f64(a)).requires_grad_()
    qt, kt, vt = t(q), t(k), t(v)
    Lq, E = qt.shape
    Lk = kt.shape[0]
    hd = E // heads
    scale = float(np.float32(1.0 / math.sqrt(hd)))
    sp = lambda a, L: a.reshape(L, heads, hd).permute(1, 0, 2)
    P = torch.softmax(sp(qt, Lq) @ sp(kt, Lk).transpose(1, 2) * scale, dim=-1)
    Pd = P if mult is None else P * torch.from_numpy(mult)
    out = (Pd @ sp(vt, Lk)).permute(1, 0, 2).reshape(Lq, E)
    (out * torch.from_numpy(f64(do))).sum().backward()
    g = lambda a: np.zeros(tuple(a.shape)) if a.grad is None else a.grad.numpy()
    return {"out": out.detach().numpy(), "P": P.detach().numpy(), "dq": g(qt), "dk": g(kt), "dv": g(vt)}


ATTN_L = ((1, 1), (3, 5), (5, 3), (4, 4), (7, 65), (65, 7))
ATTN_CASES = [(4, 8, Lq, Lk) for Lq, Lk in ATTN_L] + [(8, 128, 5, 5)]           # (heads, hd, Lq, Lk)
ATTN_EMPTY = ((4, 8, 0, 5), (4, 8, 5, 0))


def attention_inputs(heads, hd, Lq, Lk):
    """q, k, v, do float32.  Head 0's queries are x 6: a few keys hold nearly all of a row's weight there."""
    g = _rng(31, heads, hd, Lq, Lk)
    E = heads * hd
    q, k, v, do = (g.standard_normal((L, E)) for L in (Lq, Lk, Lk, Lq))
    q[:, :hd] *= 6.0
    return tuple(a.astype(np.float32) for a in (q, k, v, do))


# ------------------------------------------------------------------------------------------ asso_ce, AssoCE
def asso_ce64(logits, offs, gt, grad_scale=1.0):
    """logits [R, N] float32, offs [T + 1], gt [R, T] (index in frame | n_t = background | < 0 = not counted), grad_scale a
    float32 -> {"loss": (exp, bound) [R, T], "dlogits": (exp, bound) [R, N]}.  A pair that does not count: loss exactly 0 and
    exactly 0 over its frame's columns.  An empty frame that counts: loss log(1) = 0 (its target can only be the background)."""
    l = f64(logits)
    R, N = l.shape
    T = len(offs) - 1
    gs = float(np.float32(grad_scale))
    loss, dloss = np.zeros((R, T)), np.zeros((R, T))
    dl, ddl = np.zeros((R, N)), np.zeros((R, N))
    for t in range(T):
        lo, hi = int(offs[t]), int(offs[t + 1])
        n = hi - lo
        tg = np.asarray(gt)[:, t]
        cnt = tg >= 0
        assert bool((tg <= n).all()), "a target beyond the background: outside the contract"
        if n == 0:
            dloss[cnt, t] = TINY
            continue
        seg = l[:, lo:hi]
        a, da = A.softmax_bg64(seg)
        onehot = (np.arange(n)[None] == tg[:, None]).astype(np.float64)
        diff, ddiff = _sub(a, da, onehot, 0.0)
        gv, gd = _mul(diff, ddiff, np.full_like(diff, gs), 0.0)
        dl[:, lo:hi] = np.where(cnt[:, None], gv, 0.0)
        ddl[:, lo:hi] = np.where(cnt[:, None], gd, 0.0)
        m = np.maximum(seg.max(1), 0.0)
        e, bg = np.exp(seg - m[:, None]), np.exp(-m)
        Z = e.sum(1) + bg
        r = (np.abs(seg - m[:, None]) + EXPF) * U
        relZ = ((e * r).sum(1) + bg * EXPF * U) / Z + (-(-n // 64) + 7) * U + n * TINY
        logZ = np.log(Z)
        dlog = -np.log1p(-relZ) + LOGF * U * np.abs(logZ)
        lse, dlse = m + logZ, _rnd(m + logZ, dlog)
        tl = np.where(tg < n, seg[np.arange(R), np.clip(tg, 0, n - 1)], 0.0)
        v, d = _sub(lse, dlse, tl, 0.0)
        loss[:, t], dloss[:, t] = np.where(cnt, v, 0.0), np.where(cnt, d, 0.0)
    return {"loss": (loss, dloss), "dlogits": (dl, ddl)}


def asso_ce_autograd(logits, offs, gt, upstream=1.0):
    """torch float64: per counted (row, frame) the cross entropy of [segment | 0]; gradient of upstream * sum."""
    lt = torch.from_numpy(f64(logits)).requires_grad_()
    R, T = np.asarray(gt).shape
    loss = torch.zeros((R, T), dtype=torch.float64)
    rows = []
    for i in range(R):
        for t in range(T):
            tg = int(gt[i][t])
            if tg < 0:
                continue
            z = torch.cat([lt[i, int(offs[t]):int(offs[t + 1])], torch.zeros(1, dtype=torch.float64)])
            rows.append(((i, t), torch.logsumexp(z, 0) - z[tg]))
    total = sum(v for _, v in rows) if rows else lt.sum() * 0.0
    (total * float(np.float32(upstream))).backward()
    for (i, t), v in rows:
        loss[i, t] = v.detach()
    return {"loss": loss.numpy(), "dlogits": lt.grad.numpy(), "total": float(total.detach())}


ASSO_ROWS = (1, 4, 5)
ASSO_FRAMES = ((0,), (1,), (3, 0, 2), (64, 65), (130,), (2, 3, 2))     # the last: a not-counted frame WITH columns between two
ASSO_LOGITS = ("unit", "below-50", "plus80", "permuted")
ASSO_SCALES = (1.0, -0.37)
ASSO_CASES = [(R, fr, kind) for R in ASSO_ROWS for fr in ASSO_FRAMES for kind in ASSO_LOGITS]


def asso_inputs(R, frames, kind):
    """logits [R, N] float32, offs int32 [T + 1], gt int32 [R, T].  Targets: pair (i, t) takes kind (i + t) % 4 of (inside the
    frame, background, not counted, the frame's last column); an empty frame has no inside: background.  With three frames row 1
    counts frame 0, does not count frame 1 and counts frame 2; the last row's last frame (R >= 2, T >= 2) is not counted, behind
    counted ones.  Logits: unit scale | all below -50 (the background wins the maximum) | unit with one logit per row at +80 |
    every row a permutation of row 0."""
    offs = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    N, T = int(offs[-1]), len(frames)
    g = _rng(41, R, N, T, ASSO_LOGITS.index(kind))
    x = g.standard_normal((R, N))
    if kind == "below-50":
        x = -50.5 - np.abs(x)
    elif kind == "plus80" and N:
        x[np.arange(R), g.integers(0, N, R)] = 80.0
    elif kind == "permuted":
        for i in range(1, R):
            x[i] = x[0][g.permutation(N)]
    gt = np.zeros((R, T), np.int32)
    for i in range(R):
        for t, n in enumerate(frames):
            sel = (i + t) % 4
            gt[i, t] = (n if n == 0 else (i + 2 * t) % n) if sel == 0 else n if sel == 1 else -1 if sel == 2 else max(n - 1, 0)
    if T >= 3 and R >= 2:
        gt[1] = [0 if frames[0] else frames[0], -1, frames[2]] + [-1] * (T - 3)
    if T >= 2 and R >= 2:
        gt[R - 1, :] = [(frames[t] if frames[t] == 0 else 0) for t in range(T)]
        gt[R - 1, T - 1] = -1
    return x.astype(np.float32), offs, gt


# ------------------------------------------------------------------------------------------ sigmoid focal, FocalSum
def focal64(x, t, alpha, gamma):
    """x, t [n] float32 (t in {0, 1}) -> {"loss", "dx"}: (exp, bound) [n], per the header's formulas with p_t =
    sigmoid((2t - 1) x) and alpha_t = alpha t + (1 - alpha)(1 - t), 1 for alpha < 0."""
    x, t = f64(x), f64(t)
    alpha, gamma = float(np.float32(alpha)), float(np.float32(gamma))
    sgn = 2 * t - 1
    s = sgn * x
    e = np.exp(-np.abs(s))
    de = e * EXPF * U + TINY
    l = np.log1p(e)
    dl_ = de + LOG1PF * U * l
    nlp = np.maximum(-s, 0.0) + l
    dnlp = _rnd(nlp, dl_)
    pt = np.exp(-nlp)
    dpt = pt * np.expm1(dnlp + EXPF * U) + TINY
    om = -np.expm1(-nlp)                                # 1 - pt without the cancellation
    dom = _rnd(om, dpt)
    if gamma == 0:
        mod, dmod = np.ones_like(om), np.zeros_like(om)
    else:
        mod = om ** gamma
        hi, lo = (om + dom) ** gamma, np.maximum(om - dom, 0.0) ** gamma
        dmod = np.maximum(hi - mod, mod - lo)
        dmod = dmod + POWF * U * (mod + dmod)
    if alpha >= 0:
        a, da = np.where(t == 1, alpha, 1 - alpha), np.where(t == 1, 0.0, U * abs(1 - alpha))
    else:
        a, da = np.ones_like(s), np.zeros_like(s)
    am, dam = _mul(a, da, mod, dmod)
    loss = _mul(am, dam, nlp, dnlp)
    t1, dt1 = _mul(pt, dpt, nlp, dnlp)
    t1, dt1 = _mul(t1, dt1, np.full_like(t1, gamma), 0.0)
    inner, dinner = _sub(-t1, dt1, om, dom)
    dx, ddx = _mul(am, dam, inner, dinner)
    return {"loss": loss, "dx": (sgn * dx, ddx)}


def focal_autograd(x, t, alpha, gamma, upstream=1.0):
    xt = torch.from_numpy(f64(x)).requires_grad_()
    tt = torch.from_numpy(f64(t))
    alpha, gamma = float(np.float32(alpha)), float(np.float32(gamma))
    s = (2 * tt - 1) * xt
    nlp = torch.nn.functional.softplus(-s)
    om = torch.sigmoid(-s)
    a = (alpha * tt + (1 - alpha) * (1 - tt)) if alpha >= 0 else torch.ones_like(s)
    loss = a * torch.pow(om, gamma) * nlp
    (loss.sum() * float(np.float32(upstream))).backward()
    return {"loss": loss.detach().numpy(), "dx": xt.grad.numpy(), "total": float(loss.detach().sum())}


FOCAL_N = (1, 255, 256, 257)
FOCAL_X = (0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)
FOCAL_AG = ((0.25, 2.0), (-1.0, 2.0), (0.25, 0.0), (0.25, 1.5))
FOCAL_CASES = [(n, ag) for n in FOCAL_N for ag in FOCAL_AG]


def focal_inputs(n):
    """x, t [n] float32: every value of FOCAL_X under both targets first (as far as n reaches), then random x 3."""
    g = _rng(51, n)
    x = 3 * g.standard_normal(n)
    t = (g.random(n) < 0.5).astype(np.float64)
    fixed = [(v, tt) for tt in (1.0, 0.0) for v in FOCAL_X]
    if n == 1:
        fixed = [(-1.0, 1.0)]
    for i, (v, tt) in enumerate(fixed[:n]):
        x[i], t[i] = v, tt
    return x.astype(np.float32), t.astype(np.float32)


SUM_COUNTS = (1, 3, 4, 5)
UPSTREAM = 0.625                                       # the upstream gradient of the AssoCE / FocalSum cases: not 1, exact in fp32


def assoce_sum64(logits, offs, gt, upstream):
    """AssoCE: total = sum of the per-pair losses (depth pad4(R T)); d total / d logits with grad_scale = upstream."""
    r = asso_ce64(logits, offs, gt, upstream)
    return {"total": sum64(*r["loss"]), "dlogits": r["dlogits"]}


def focalsum64(x, t, alpha, gamma, upstream):
    r = focal64(x, t, alpha, gamma)
    up = float(np.float32(upstream))
    return {"total": sum64(*r["loss"]), "dx": _mul(r["dx"][0], r["dx"][1], np.full_like(r["dx"][0], up), 0.0)}


# ------------------------------------------------------------------------------------------ the chain
CHAIN_E, CHAIN_HEADS, CHAIN_FFN = 32, 4, 48
CHAIN_FRAMES = ((1,), (4,), (3, 0, 3), (12, 13, 12))
CHAIN_VARIANTS = ("long", "short", "shared")
CHAIN_CASES = [(v, fr, None) for v in CHAIN_VARIANTS for fr in CHAIN_FRAMES] + [("long", (12, 13, 12), 0.1)]
CHAIN_REORDERINGS = 8
CHAIN_STREAM = (7, 4, 1)                               # (seed, iteration, rank): the sites count from 0 in call order


def chain_layers(variant):
    """(matcher name, encoder layers, decoder layers, decoder FFN) of the head variants at the shipped layer counts (1 + 1)."""
    return {"long": ("long_term_matcher", 1, 1, True), "short": ("short_term_matcher", 1, 1, True),
            "shared": ("shared_matcher", 0, 1, False)}[variant]


def chain_params(variant, seed=3):
    """{state-dict key: float32 array} of one matcher at E = 32, FFN 48: weights of unit row scale / sqrt(fan-in)."""
    name, n_enc, n_dec, dec_ffn = chain_layers(variant)
    g = _rng(61, seed, CHAIN_VARIANTS.index(variant))
    E, Fw = CHAIN_E, CHAIN_FFN
    out = {}

    def lin(key, n, k, bias=True):
        out[key + ("weight" if key.endswith("_") else ".weight")] = (g.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32)
        if bias:
            out[key + ("bias" if key.endswith("_") else ".bias")] = (0.1 * g.standard_normal(n)).astype(np.float32)

    def mha(p):
        lin(p + ".in_proj_", 3 * E, E)
        lin(p + ".out_proj", E, E)

    def ffn(p):
        lin(p + "linear1", Fw, E)
        lin(p + "linear2", E, Fw)
    for i in range(n_enc):
        p = "roi_heads.%s.encoder.layers.%d." % (name, i)
        mha(p + "self_attn")
        ffn(p)
    for i in range(n_dec):
        p = "roi_heads.%s.decoder.layers.%d." % (name, i)
        mha(p + "multihead_attn")
        if dec_ffn:
            ffn(p)
    return out


def chain_inputs(frames):
    """reid [N, E] float32 (rows 2 .. 2 + N of a larger buffer on the device), offs, gt [N, T] as `_detr_asso_loss` forms them
    with NEG_UNMATCHED: every row counts every frame; row i's own track: the same index in the other frames where it exists."""
    offs = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    N, T = int(offs[-1]), len(frames)
    reid = _rng(62, N, T).standard_normal((N, CHAIN_E)).astype(np.float32)
    gt = np.zeros((N, T), np.int32)
    for i in range(N):
        j = i - int(offs[np.searchsorted(offs, i, side="right") - 1])
        for t, n in enumerate(frames):
            gt[i, t] = j if (j < n and i % 3 != 2) else n
    num = float((gt != np.asarray(frames, np.int32)[None]).sum())
    return reid, offs, gt, num


class Reorder:
    """A random reordering of every contraction axis of the chain statement: `mm(a, b)` = a b^T with the rows of a, the rows of b
    and the shared axis each permuted (so that the backward's contractions over those axes are reordered too) and the result put
    back; `perm(n)` for the softmax and loss sums.  gen None: the identity."""

    def __init__(self, seed=None):
        self.g = None if seed is None else torch.Generator().manual_seed(int(seed))

    def perm(self, n):
        return torch.arange(n) if self.g is None else torch.randperm(n, generator=self.g)

    def mm(self, a, b):
        if self.g is None:
            return a @ b.T
        pm, pn, pk = self.perm(a.shape[0]), self.perm(b.shape[0]), self.perm(a.shape[1])
        y = a[pm][:, pk] @ b[pn][:, pk].T
        return y[torch.argsort(pm)][:, torch.argsort(pn)]

    def softmax(self, s):
        pk = self.perm(s.shape[-1])
        return torch.softmax(s[..., pk], dim=-1)[..., torch.argsort(pk)]

    def total(self, v):
        """A plain sum, one addition after the other in the permuted order: what a product against a ones row is.  (torch's own
        .sum() is a cascade that lands on the nearest float32 in every order, which a depth-K accumulation does not.)"""
        acc = None
        for i in self.perm(v.shape[0]).tolist():
            acc = v[i] if acc is None else acc + v[i]
        return acc


def chain_eval(variant, frames, p, dtype, order=None, params=None):
    """The chain in torch at `dtype` (float64: the statement; float32 with a Reorder: one more correct fp32 evaluation):
    matcher_transformer's forward (dropout_statement.matcher_f64's formulas, the masks of `p` on CHAIN_STREAM), logits = feats
    memory^T, loss = sum of the per-pair cross entropies / (num + 1e-4); backward of the loss.
    -> {"feats", "memory", "logits", "loss", "d reid", "d <key>" for every parameter}: numpy float64."""
    order = order or Reorder()
    name, n_enc, n_dec, dec_ffn = chain_layers(variant)
    params = params or chain_params(variant)
    reid0, offs, gt, num = chain_inputs(frames)
    P = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in params.items()}
    reid = torch.from_numpy(reid0).to(dtype).requires_grad_()
    seed, iteration, rank = CHAIN_STREAM
    site = [0]
    heads, E = CHAIN_HEADS, CHAIN_E
    hd = E // heads

    def mask(shape):
        s = site[0]
        site[0] += 1
        if p is None:
            return None
        return torch.from_numpy(mask_mult(tuple(shape), p, (seed, s, iteration, rank))).to(dtype)

    def drop(x):
        m = mask(x.shape)
        return x if m is None else x * m

    def lin(x, key):
        return order.mm(x, P[key + ".weight"]) + P[key + ".bias"]

    def mha(q_in, kv_in, key):
        w, b = P[key + ".in_proj_weight"], P[key + ".in_proj_bias"]
        q = order.mm(q_in, w[:E]) + b[:E]
        kv = order.mm(kv_in, w[E:]) + b[E:]
        k, v = kv[:, :E], kv[:, E:]
        Lq, Lk = q.shape[0], k.shape[0]
        scale = float(np.float32(1.0 / math.sqrt(hd)))
        m = mask((heads, Lq, Lk))
        outs = []
        for h in range(heads):
            c = slice(h * hd, (h + 1) * hd)
            if Lq == 0 or Lk == 0:
                outs.append(torch.zeros((Lq, hd), dtype=dtype))
                continue
            Ph = order.softmax(order.mm(q[:, c], k[:, c]) * scale)
            if m is not None:
                Ph = Ph * m[h]
            outs.append(order.mm(Ph, v[:, c].T))
        return lin(torch.cat(outs, 1), key + ".out_proj")

    def ffn(x, pre):
        return lin(drop(torch.relu(lin(x, pre + "linear1"))), pre + "linear2")

    memory = reid
    for i in range(n_enc):
        pre = "roi_heads.%s.encoder.layers.%d." % (name, i)
        memory = memory + drop(mha(memory, memory, pre + "self_attn"))
        memory = memory + drop(ffn(memory, pre))
    tgt = reid
    for i in range(n_dec):
        pre = "roi_heads.%s.decoder.layers.%d." % (name, i)
        tgt = tgt + drop(mha(tgt, memory, pre + "multihead_attn"))
        if dec_ffn:
            tgt = tgt + drop(ffn(tgt, pre))
    logits = order.mm(tgt, memory)
    zero = torch.zeros(1, dtype=dtype)
    pairs = []
    for i in range(gt.shape[0]):
        for t in range(gt.shape[1]):
            if gt[i, t] < 0:
                continue
            z = torch.cat([logits[i, int(offs[t]):int(offs[t + 1])], zero])
            pk = order.perm(z.shape[0])
            pairs.append(torch.logsumexp(z[pk], 0) - z[int(gt[i, t])])
    loss = order.total(torch.stack(pairs)) / (num + 1e-4)
    loss.backward()
    n = lambda a: a.detach().double().numpy()
    out = {"feats": n(tgt), "memory": n(memory), "logits": n(logits), "loss": n(loss), "d reid": n(reid.grad), "sites": site[0]}
    for k2, v2 in P.items():
        out["d " + k2] = np.zeros(tuple(v2.shape)) if v2.grad is None else n(v2.grad)
    return out


_CHAIN_CACHE = {}


def chain_statement(variant, frames, p):
    """(exp, spread): the float64 chain, and per tensor the largest max|f32 - f64| over CHAIN_REORDERINGS reorderings of the
    float32 statement on the CPU.  The chain's assertion is max|got - f64| <= 2 spread: the device's tile order is one more
    reordering of the same fp32 sums.  Computed once per case and shared."""
    key = (variant, tuple(frames), p)
    if key not in _CHAIN_CACHE:
        exp = chain_eval(variant, frames, p, torch.float64)
        spread = {}
        for r in range(CHAIN_REORDERINGS):
            got = chain_eval(variant, frames, p, torch.float32, Reorder(1000 + r))
            for k, v in got.items():
                if k != "sites":
                    spread[k] = max(spread.get(k, 0.0), float(np.abs(v - exp[k]).max()) if v.size else 0.0)
        _CHAIN_CACHE[key] = (exp, spread)
    return _CHAIN_CACHE[key]
