"""No GPU: the training statements of tests/train_statement.py against torch's float64 autograd on every table case; a float32
numpy emulation of every Function and kernel that follows the padded layouts (pad4 depths, zero-padded transposes, the ones row,
[heads, Lq, pad4(Lk)] weights, the lane loops' limits) inside every bound; and planted mistakes, each ONE changed line of that
emulation, each outside the bound on the table case its entry names.  What the bounds are made of is in train_statement.py.

`HARMLESS` holds the one mistake of the list that cannot leave any bound: a ones row that is 1 in all pad4(M) places multiplies
the ZERO padding of the transposed dy (`_transpose_padded` zero-fills), so the bias gradient keeps its bits.  The test asserts
exactly that; the mistake that can be seen there (the bias gradient taken in front of the ReLU mask) is planted beside it."""
import math

import numpy as np
import pytest
import torch

import dropout_statement as D
import train_statement as S

f32 = np.float32
SCALE_P = f32(D.scale_f32(S.P_DROP))


def _z(*s):
    return np.zeros(s, f32)


def e_gemm(a, w, bias=None, relu=False):
    y = np.asarray(a, f32) @ np.asarray(w, f32).T
    if bias is not None:
        y = y + np.asarray(bias, f32)
    return np.maximum(y, f32(0)) if relu else y


def tp(x):
    """`_transpose_padded`: x [R, C] -> [C, pad4(R)], zero beyond R."""
    R, C = x.shape
    out = _z(C, S.pad4(R))
    out[:, :R] = x.T
    return out


# ------------------------------------------------------------------------------------------ the emulation
def emu_linear(x, w, b, relu, dy, mult=None, bug=None):
    M, K = x.shape
    N = w.shape[0]
    if M == 0:
        out = {"y": _z(0, N), "dx": _z(0, K), "dw": _z(N, K)}
        if b is not None:
            out["db"] = _z(N)
        return out
    y = e_gemm(x, w, b, relu)
    d = dy
    if mult is not None:
        y = y * mult.astype(f32)
        d = dy * SCALE_P
    if relu:
        gate = y > 0
        if bug == "relu-mask-from-dy":
            gate = dy > 0
        if bug == "relu-passes-at-zero":
            gate = y >= 0
        d = np.where(gate, d, f32(0))
    Np, Mp = S.pad4(N), S.pad4(M)
    dyp = _z(M, Np)
    dyp[:, :N] = d
    wT = tp(w)
    if bug == "dx-w-untransposed":
        wT[:, :N] = w                                                                  # needs N == K
    dx = e_gemm(dyp, wT)
    dyT = tp(d)
    dw = e_gemm(dyT, tp(x))
    if bug == "dw-xT-dy":
        dw = e_gemm(tp(x), dyT)                                                        # needs N == K
    ones = _z(1, Mp)
    ones[:, :M] = 1
    if bug == "ones-row-all-ones":
        ones[:] = 1
    db = e_gemm(tp(dy) if bug == "db-before-mask" else dyT, ones)[:, 0]
    out = {"y": y, "dx": dx, "dw": dw}
    if b is not None:
        out["db"] = db
    return out


def emu_softmax_rows(s, scale):
    v = s * f32(scale)
    e = np.exp(v - v.max(1, keepdims=True))
    return e * (f32(1) / e.sum(1, keepdims=True, dtype=f32))


def emu_softmax_bwd(P, dP, cols, scale, dS=None, G=None, bug=None):
    """P, dP [rows, ld]; dS: the output buffer (zeros by default); G: the masked gradient where the caller forms one."""
    ld = P.shape[1]
    dS = _z(*P.shape) if dS is None else dS
    g = dP if G is None else G
    lim = cols
    if bug == "dot-over-ld":
        lim = ld
    if bug == "no-second-lane-pass":
        cols = lim = min(cols, 64)
    dot = (g[:, :lim] * P[:, :lim]).sum(1, keepdims=True, dtype=f32)
    if bug == "no-row-dot":
        dot = f32(0)
    sc = f32(1) if bug == "no-scale" else f32(scale)
    dS[:, :cols] = sc * P[:, :cols] * (g[:, :cols] - dot)
    return dS


def emu_attention(q, k, v, heads, do, mult=None, bug=None):
    Lq, E = q.shape
    Lk = k.shape[0]
    hd = E // heads
    Lkp = S.pad4(Lk)
    scale = f32(1.0 / math.sqrt(hd))
    out, P = _z(Lq, E), _z(heads, Lq, Lkp)
    dq, dk, dv = _z(Lq, E), _z(Lk, E), _z(Lk, E)
    if Lq == 0 or Lk == 0:
        return {"out": out, "P": P, "dq": dq, "dk": dk, "dv": dv}
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        P[h][:, :Lk] = emu_softmax_rows(e_gemm(q[:, c], k[:, c]), scale)
        if bug == "p-padding-nonzero":
            P[h][:, Lk:] = f32(1e-3)
        Pd = P[h].copy()
        if mult is not None:
            Pd[:, :Lk] = P[h][:, :Lk] * mult[h].astype(f32)
        out[:, c] = e_gemm(Pd, tp(v[:, c]))
        dv[:, c] = e_gemm(tp((P[h] if bug == "dv-from-undropped-p" else Pd)[:, :Lk]), tp(do[:, c]))
        dP = _z(Lq, Lkp)
        dP[:, :Lk] = e_gemm(do[:, c], v[:, c])
        G = None
        if mult is not None:
            G = dP.copy()
            G[:, :Lk] = dP[:, :Lk] * mult[h].astype(f32)
            if bug == "mask-twice":
                G[:, :Lk] = G[:, :Lk] * mult[h].astype(f32)
        dS = emu_softmax_bwd(P[h], dP, Lk, scale, G=G)
        dq[:, c] = e_gemm(dS, tp(k[:, c]))
        dk[:, c] = e_gemm(tp(dS[:, :Lk]), tp(q[:, c]))
    return {"out": out, "P": P, "dq": dq, "dk": dk, "dv": dv}


def emu_asso_ce(logits, offs, gt, gs, bug=None):
    R, N = logits.shape
    T = len(offs) - 1
    loss, dl = _z(R, T), _z(R, N)
    with np.errstate(all="ignore"):
        for i in range(R):
            for t in range(T):
                lo, hi = int(offs[t]), int(offs[t + 1])
                n, tg = hi - lo, int(gt[i, t])
                row = logits[i, lo:hi]
                if tg < 0:
                    if bug == "zero-whole-row":
                        dl[i, :] = 0
                    if bug != "not-counted-keeps-gradient":
                        continue
                    tg = n
                mx = f32(-np.inf) if bug == "max-without-background" else f32(0)
                mx = max(mx, row.max()) if n else mx
                e = np.exp(row - mx)
                z = e.sum(dtype=f32) + (f32(0) if bug == "normaliser-without-background" else np.exp(f32(0) - mx))
                if gt[i, t] >= 0:
                    loss[i, t] = (mx + np.log(z)) - (row[tg] if tg < n else f32(0))
                col = n - 1 if (bug == "background-minus-one-on-last" and tg == n) else tg
                g = f32(1) if bug == "grad-scale-ignored" else f32(gs)
                dl[i, lo:hi] = g * (e / z - (np.arange(n) == col).astype(f32))
    return {"loss": loss, "dlogits": dl}


def emu_focal(x, t, alpha, gamma, bug=None):
    alpha, gamma = f32(alpha), f32(gamma)
    with np.errstate(all="ignore"):
        sgn = f32(2) * t - f32(1)
        s = sgn * x
        nlp = np.maximum(-s, f32(0)) + np.log1p(np.exp(-np.abs(s)))
        if bug == "unstable-log":
            nlp = -np.log(f32(1) / (f32(1) + np.exp(-s)))
        pt = np.exp(-nlp)
        a = alpha * t + (f32(1) - alpha) * (f32(1) - t)
        if bug == "alpha-exchanged":
            a = alpha * (f32(1) - t) + (f32(1) - alpha) * t
        if alpha < 0 and bug != "negative-alpha-not-honoured":
            a = np.ones_like(x)
        mod = np.power(f32(1) - pt, gamma)
        loss = a * mod * nlp
        inner = gamma * pt * (-nlp) - (f32(1) - pt)
        if bug == "no-gamma-term":
            inner = -(f32(1) - pt)
        dx = (f32(1) if bug == "sign-does-not-flip" else sgn) * a * mod * inner
    return {"loss": loss.astype(f32), "dx": dx.astype(f32)}


def emu_sum(v):
    flat = _z(1, S.pad4(v.size))
    flat[0, :v.size] = v.reshape(-1)
    return e_gemm(flat, np.ones_like(flat))[0, 0]


# ------------------------------------------------------------------------------------------ cases -> (emulation, statement, autograd)
def _drop_mult(shape):
    return S.mask_mult(shape, S.P_DROP)


def run_linear(case, drop=False, bug=None):
    M, N, K, bias, relu = case
    x, w, b, dy = S.linear_inputs(M, N, K, bias)
    mult = _drop_mult((M, N)) if drop and M else None
    return (emu_linear(x, w, b, relu, dy, mult, bug), S.linear64(x, w, b, relu, dy, mult, float(SCALE_P)),
            S.linear_autograd(x, w, b, relu, dy, mult))


def run_attention(case, drop=False, bug=None):
    heads, hd, Lq, Lk = case
    q, k, v, do = S.attention_inputs(heads, hd, Lq, Lk)
    mult = _drop_mult((heads, Lq, Lk)) if drop and Lq and Lk else None
    return (emu_attention(q, k, v, heads, do, mult, bug), S.attention64(q, k, v, heads, do, mult),
            S.attention_autograd(q, k, v, heads, do, mult))


def run_softmax_bwd(case, bug=None):
    rows, cols = case
    P, dP = S.softmax_bwd_inputs(rows, cols)
    ld = S.softmax_ld(cols)
    Pb, dPb = np.full((rows, ld), np.nan, f32), np.full((rows, ld), np.nan, f32)
    Pb[:, :cols], dPb[:, :cols] = P, dP
    got = emu_softmax_bwd(Pb, dPb, cols, S.SOFTMAX_SCALE, dS=np.full((rows, ld), -7.0, f32), bug=bug)
    exp, bound = S.softmax_bwd_case64(P, dP)
    full_e, full_b = np.full((rows, ld), -7.0), np.zeros((rows, ld))                   # the sentinel stays beyond cols
    full_e[:, :cols], full_b[:, :cols] = exp, bound
    return {"dS": got}, {"dS": (full_e, full_b)}, None


def run_asso(case, gs, bug=None):
    R, frames, kind = case
    l, offs, gt = S.asso_inputs(R, frames, kind)
    return emu_asso_ce(l, offs, gt, gs, bug), S.asso_ce64(l, offs, gt, gs), S.asso_ce_autograd(l, offs, gt, gs)


def run_focal(case, bug=None):
    n, (alpha, gamma) = case
    x, t = S.focal_inputs(n)
    return emu_focal(x, t, alpha, gamma, bug), S.focal64(x, t, alpha, gamma), S.focal_autograd(x, t, alpha, gamma)


def ratios(got, want):
    return {k: S.worst(got[k], *want[k])[0] for k in want}


def _agree(want, auto, what):
    for k, (exp, _) in want.items():
        a = auto[k]
        e = exp[..., :a.shape[-1]] if k == "P" else exp
        assert e.shape == a.shape, (what, k)
        assert np.allclose(e, a, rtol=1e-9, atol=1e-13), (what, k, float(np.abs(e - a).max()))


# ------------------------------------------------------------------------------------------ 1. statements = torch float64 autograd
def test_statements_agree_with_float64_autograd():
    for case in S.LINEAR_CASES:
        for drop in ((False, True) if case[4] else (False,)):
            _, want, auto = run_linear(case, drop)
            _agree(want, auto, ("linear", case, drop))
    for case in S.ATTN_CASES + list(S.ATTN_EMPTY):
        for drop in (False, True):
            _, want, auto = run_attention(case, drop)
            _agree(want, auto, ("attention", case, drop))
    for case in S.ASSO_CASES:
        for gs in S.ASSO_SCALES:
            _, want, auto = run_asso(case, gs)
            _agree(want, auto, ("asso_ce", case, gs))
    for case in S.FOCAL_CASES:
        _, want, auto = run_focal(case)
        _agree(want, auto, ("focal", case))
    for rows, cols in S.SOFTMAX_CASES:                                                 # dS is the Jacobian of softmax(scale s) applied to dP
        P, dP = S.softmax_bwd_inputs(rows, cols)
        s = torch.log(torch.from_numpy(S.f64(P))).div(S.SOFTMAX_SCALE).requires_grad_()
        p = torch.softmax(s * S.SOFTMAX_SCALE, -1)
        (p * torch.from_numpy(S.f64(dP))).sum().backward()
        # the float32 rows of P do not sum to exactly 1: the statement is of the kernel's formula on the P it is handed
        exp, _ = S.softmax_bwd64(p.detach().numpy(), 0.0, S.f64(dP), 0.0, S.SOFTMAX_SCALE)
        assert np.allclose(exp, s.grad.numpy(), rtol=1e-9, atol=1e-13), (rows, cols)


def test_sums_agree_with_float64_autograd():
    for count in S.SUM_COUNTS:
        frames = (2,) * count
        l, offs, gt = S.asso_inputs(1, frames, "unit")
        gt = np.maximum(gt, 0)                                                         # every pair counts: `count` summed values
        want, auto = S.assoce_sum64(l, offs, gt, S.UPSTREAM), S.asso_ce_autograd(l, offs, gt, S.UPSTREAM)
        assert abs(want["total"][0] - auto["total"]) < 1e-12 and np.allclose(want["dlogits"][0], auto["dlogits"], rtol=1e-9, atol=1e-13)
        x, t = S.focal_inputs(255)
        want, auto = S.focalsum64(x[:count], t[:count], 0.25, 2.0, S.UPSTREAM), S.focal_autograd(x[:count], t[:count], 0.25, 2.0, S.UPSTREAM)
        assert abs(want["total"][0] - auto["total"]) < 1e-12 and np.allclose(want["dx"][0], auto["dx"], rtol=1e-9, atol=1e-13)


# ------------------------------------------------------------------------------------------ 2. the emulation inside every bound
def _merge(worst_of, name, r):
    for k, v in r.items():
        worst_of[name + " " + k] = max(worst_of.get(name + " " + k, 0.0), v)


def test_emulation_stays_inside_every_bound():
    w = {}
    for case in S.LINEAR_CASES:
        got, want, _ = run_linear(case)
        _merge(w, "Linear", ratios(got, want))
        if case[4]:
            got, want, _ = run_linear(case, drop=True)
            _merge(w, "LinearReluDrop", ratios(got, want))
    for M in S.SEAM_M:
        got, want, _ = run_linear((M, S.SEAM[0], S.SEAM[1], True, False))
        _merge(w, "Linear seam", ratios(got, want))
    for case in S.ATTN_CASES + list(S.ATTN_EMPTY):
        for drop in (False, True):
            got, want, _ = run_attention(case, drop)
            _merge(w, "AttentionDrop" if drop else "Attention", ratios(got, want))
    for case in S.SOFTMAX_CASES:
        got, want, _ = run_softmax_bwd(case)
        _merge(w, "softmax_rows_backward", ratios(got, want))
    for case in S.ASSO_CASES:
        for gs in S.ASSO_SCALES:
            got, want, _ = run_asso(case, gs)
            _merge(w, "asso_ce", ratios(got, want))
    for case in S.FOCAL_CASES:
        got, want, _ = run_focal(case)
        _merge(w, "sigmoid_focal", ratios(got, want))
    for count in S.SUM_COUNTS:
        l, offs, gt = S.asso_inputs(1, (2,) * count, "unit")
        gt = np.maximum(gt, 0)
        got = emu_asso_ce(l, offs, gt, S.UPSTREAM)
        want = S.assoce_sum64(l, offs, gt, S.UPSTREAM)
        _merge(w, "AssoCE", ratios({"total": emu_sum(got["loss"]), "dlogits": got["dlogits"]}, want))
        x, t = S.focal_inputs(255)
        got = emu_focal(x[:count], t[:count], 0.25, 2.0)
        want = S.focalsum64(x[:count], t[:count], 0.25, 2.0, S.UPSTREAM)
        _merge(w, "FocalSum", ratios({"total": emu_sum(got["loss"]), "dx": got["dx"] * f32(S.UPSTREAM)}, want))
    for k in sorted(w):
        print("worst |err| / bound  %-32s %.4f" % (k, w[k]))
    assert all(v <= 1.0 for v in w.values()), {k: v for k, v in w.items() if not v <= 1.0}


def test_seam_pair_shares_its_first_rows():
    a = S.linear_inputs(128, *S.SEAM, True)
    b = S.linear_inputs(129, *S.SEAM, True)
    assert np.array_equal(a[0], b[0][:128]) and np.array_equal(a[3], b[3][:128]) and np.array_equal(a[1], b[1])
    assert S.SEAM[0] * S.SEAM[1] == 1 << 18


# ------------------------------------------------------------------------------------------ 3. planted mistakes
LIN = lambda M, N, K, bias=True, relu=True: (M, N, K, bias, relu)
MISTAKES = [
    # name, runner, case the mistake must fail on, keyword arguments of the runner
    ("relu-mask-from-dy", run_linear, LIN(5, 5, 8), {}),
    ("relu-passes-at-zero", run_linear, LIN(5, 4, 8, bias=False), {}),               # row 1 of x is zero: pre-activation exactly 0
    ("db-before-mask", run_linear, LIN(5, 5, 8), {}),
    ("dw-xT-dy", run_linear, LIN(5, 8, 8), {}),
    ("dx-w-untransposed", run_linear, LIN(5, 4, 4), {}),
    ("relu-passes-at-zero", run_linear, LIN(5, 4, 8), {"drop": True}),               # behind the dropout: y = 0 where dropped too
    ("p-padding-nonzero", run_attention, (4, 8, 3, 5), {}),
    ("p-padding-nonzero", run_attention, (4, 8, 5, 3), {"drop": True}),
    ("mask-twice", run_attention, (4, 8, 3, 5), {"drop": True}),
    ("dv-from-undropped-p", run_attention, (4, 8, 3, 5), {"drop": True}),
    ("no-scale", run_softmax_bwd, (4, 63), {}),
    ("no-row-dot", run_softmax_bwd, (4, 63), {}),
    ("dot-over-ld", run_softmax_bwd, (5, 65), {}),                                    # the padding of P and dP holds NaN
    ("no-second-lane-pass", run_softmax_bwd, (5, 65), {}),
    ("no-second-lane-pass", run_softmax_bwd, (1, 130), {}),
    ("max-without-background", run_asso, (4, (3, 0, 2), "unit"), {"gs": 1.0}),       # the empty frame: a maximum over nothing
    ("normaliser-without-background", run_asso, (4, (1,), "unit"), {"gs": 1.0}),
    ("background-minus-one-on-last", run_asso, (4, (3, 0, 2), "unit"), {"gs": 1.0}),
    ("not-counted-keeps-gradient", run_asso, (4, (2, 3, 2), "unit"), {"gs": 1.0}),
    ("zero-whole-row", run_asso, (4, (2, 3, 2), "unit"), {"gs": 1.0}),                # the last row: not counted BEHIND counted frames
    ("zero-whole-row", run_asso, (5, (64, 65), "permuted"), {"gs": -0.37}),
    ("grad-scale-ignored", run_asso, (1, (130,), "unit"), {"gs": -0.37}),
    ("alpha-exchanged", run_focal, (255, (0.25, 2.0)), {}),
    ("negative-alpha-not-honoured", run_focal, (255, (-1.0, 2.0)), {}),
    ("no-gamma-term", run_focal, (255, (0.25, 2.0)), {}),
    ("sign-does-not-flip", run_focal, (255, (0.25, 1.5)), {}),
    ("unstable-log", run_focal, (255, (0.25, 0.0)), {}),                              # s = -100, -88: sigmoid underflows, -log 0
]
HARMLESS = [("ones-row-all-ones", run_linear, LIN(5, 5, 8), {})]


@pytest.mark.parametrize("name,runner,case,kw", MISTAKES, ids=["%s-%d" % (m[0], i) for i, m in enumerate(MISTAKES)])
def test_planted_mistake_leaves_the_bound(name, runner, case, kw):
    clean, want, _ = runner(case, **kw)
    assert max(ratios(clean, want).values()) <= 1.0                                    # the same case, unchanged: inside
    got, want, _ = runner(case, bug=name, **kw)
    r = ratios(got, want)
    print("planted %-32s on %-40s worst |err| / bound per output: %s" % (
        name, case, "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
    assert max(r.values()) > 1.0, (name, case, r)


@pytest.mark.parametrize("name,runner,case,kw", HARMLESS)
def test_harmless_change_keeps_every_bit(name, runner, case, kw):
    clean, _, _ = runner(case, **kw)
    got, _, _ = runner(case, bug=name, **kw)
    for k in clean:
        assert np.array_equal(clean[k].view(np.int32), got[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------ 4. the chain statement
@pytest.mark.parametrize("variant,frames,p", S.CHAIN_CASES, ids=["%s-%s-%s" % (v, "_".join(map(str, f)), p) for v, f, p in S.CHAIN_CASES])
def test_chain_statement(variant, frames, p):
    """The float64 chain's matcher is dropout_statement.matcher_f64 (the statement the dropout tests already stand on), masks
    included; the reordered float32 evaluations differ from it, and from each other, by rounding only."""
    exp, spread = S.chain_statement(variant, frames, p)
    name, n_enc, n_dec, dec_ffn = S.chain_layers(variant)
    params = {k: torch.from_numpy(v).double() for k, v in S.chain_params(variant).items()}
    reid = torch.from_numpy(S.chain_inputs(frames)[0]).double()
    seed, iteration, rank = S.CHAIN_STREAM
    masks = D.Masks(p, seed, iteration, rank)
    feats, memory = D.matcher_f64(params, "roi_heads." + name, reid, n_enc, n_dec, S.CHAIN_HEADS, dec_ffn, masks)
    assert masks.site == exp["sites"] == (2 * n_dec if not dec_ffn else 4 * (n_enc + n_dec))
    # matcher_f64 divides by sqrt(hd) in double; the chain multiplies by the float32 1 / sqrt(hd) the kernels are handed: 6e-8 relative
    close = lambda a, b: np.allclose(a, b, rtol=1e-6, atol=1e-7 * max(float(np.abs(b).max()), 1.0))
    assert close(exp["feats"], feats.numpy()) and close(exp["memory"], memory.numpy()) and close(exp["logits"], (feats @ memory.T).numpy())
    assert np.isfinite(exp["loss"]) and len(spread) == len(exp) - 1
    for k in sorted(spread):
        scale = float(np.abs(exp[k]).max())
        print("chain %-7s %-12s p %-4s %-72s max|f64| %.3e  spread %.3e" % (variant, frames, p, k[:72], scale, spread[k]))
        assert spread[k] <= 1e-4 * max(scale, 1.0), k                                  # float32 reorderings, not a different function
