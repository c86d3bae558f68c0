"""The float64 statements of the six launches of a composite decoder layer, each with an ELEMENTWISE derived error bound, the input
kinds and the case tables shared by tests/test_dec_statement_cpu.py (no GPU: the statements against torch's own modules in
float64, an fp32 emulation of the kernels' arithmetic inside the bound, the planted mistakes outside it) and
tests/test_dec_forms_gpu.py (every form of csrc/dec_attn.hip, dec_attn2.hip, dec_inter.hip, proj_ln.hip, ffn_fused.hip,
dec_tail.hip and dec_tail2.hip on every case).

What is stated (line numbers of the reference; nothing of its text is here):
  self_attn_block64   deformable_transformer.py:386-404   q = k = x + pos, v = x, 8 heads x 32, out_proj, + x, LayerNorm
  heads64             the same block in front of out_proj (the concatenated head outputs)
  raw64               ms_deform_attn.py:117-131           (tgt + query_pos) Wraw^T + braw: 256 offsets | 128 logits
  proj_ln64 / _dot64  :406-422, :171-175                  LayerNorm(x W^T + b [+ R]); <LayerNorm(..), w> + b
  ffn_ln64            :352-369                            LayerNorm(x + W2 relu(W1 x + b1) + b2)
  mlp2_64             the 256 -> 256 -> 256 perceptrons (ref_point_head, the coordinate head's hidden layers)
  tail64              :352-369, :484-488, :470-473 + adet/modeling/model/utils.py:24-37

Every statement takes float32 inputs, widens them exactly and evaluates in float64.  Beside the expectation it returns a bound
b with |fp32 evaluation - statement| <= b per element for every evaluation that keeps the project's contracts.  The bound is
carried forward step by step as an elementwise error d (float64, same shape as the value):

  f16x3 product   y = a W^T + b (+ R):   d_y = d_a |W|^T + 2e-6 (|a| |W|^T + |b| + |R|) + 1e-7 sum_k |W[n, k]|  (+ d_R)
                  the project's contract (conv_statement.py; test_ops_gpu.py::test_gemm_split_epilogue_gather_and_extremes);
                  the last term is the absolute floor of the activation split below 0.25 (test_f16x3_cpu.py).
  ReLU            1-Lipschitz: d passes.
  attention       attention64's formula (helpers.py) with the logit error of row i
                      E_i = max_j sum_c (d_q[i,c] |k[j,c]| + |qs[i,c]| d_k[j,c] + d_q[i,c] d_k[j,c]) + (hd + 2) U max_j sum_c |qs[i,c] k[j,c]|
                  (the propagated error of both operands + attention64's own chain term), entering every weight as a factor in
                  [e^-2E, e^2E] (once directly, once through the normaliser): expm1(2 E_i) sum_j p_ij |v_j|, not its first order
                  2 E_i; + sum_j p_ij (|s_ij - m_i| + 2 Lk + 16) U |v_j| + Lk 2^-126 max |v| as there; + sum_j p_ij d_v[j].
  LayerNorm       of v with error d, s = sqrt(var + eps), z = (v - mean) / s, rho = rms(d) / s:
                      d_y[i] = |gamma_i| ((d_i + mean(d) + |z_i| mean_j(|z_j| d_j)) (1 + 2 rho) / s + 3 rho^2 |z_i|)  +  own
                  First order: dy_i = gamma_i (dv_i - mean(dv) - z_i mean(z dv)) / s.  Beyond it: s'^2 = s^2 (1 + e) with
                  |e| <= 2 rho + rho^2; (1 + e)^-1/2 leaves its linear term by at most rho^2 / 2 + 3/8 e^2 (1 - |e|)^-5/2 <= 3 rho^2
                  for rho <= 2^-4, and the product of the two first-order changes is at most 1.1 rho (d_i + mean d) / s.  The
                  statement ASSERTS rho <= 2^-4 = LN_RHO_MAX on every row: every table case must pass it.
                  own = the epilogue's rounding, counted: two-pass sums of 256 terms of depth h (terms a lane adds one after the
                  other + the cross-lane steps behind them).  Read from the six epilogues: proj_ln.hip and ffn_fused.hip 4 quads + 4
                  DPP steps, dec_tail.hip and dec_attn2.hip 64 + 2, dec_tail2.hip 16 + 2 + a pairwise tree over the waves (Chan's
                  formula: the same two-pass variance), dec_attn.hip 128 + 1.  h = LN_DEPTH = 72 for the row launches, LN_DEPTH_BLOCK =
                  136 for the attention blocks.  The mean then errs by (h + 1) U mean|v|; the variance by
                  (h + 6) U relative; + eps, rsqrt (1 ulp class: 2 U), two products and the shift:
                      own_i = |gamma_i| (h + 1) U mean|v| / s + |gamma_i z_i| (h / 2 + 9.5) U + U |y_i|
  dot             sum_i y_i w_i + b: sum_i d_y[i] |w_i| + (h + 2) U (sum |y w| + |b|).
  N = 2 layer     (the coordinate head's last, plain fmaf chains): d_h |W3|^T + (h + 2) U (|h| |W3|^T + |b3|).
  inverse_sigmoid log(max(r, 1e-5f) / max(1 - r, 1e-5f)), r = clamp(ref, 0, 1): the subtraction, the quotient (not correctly
                  rounded on the device: 2.5 ulp) and logf (2 ulp of the result): 4 U + 2 U |inv|.
  sigmoid         d times the largest slope on [|z| - d, |z| + d] (never above the 1 / 4 at z = 0; with d / 4 everywhere the saturated
                  rows of `refedge` would hold the clamp mistakes) + 6 U (expf, the sum, the reciprocal).
  sine embedding  angle = ref 2 pi / dim_t: d_angle = 2 pi d_ref / dim_t + 3 U |angle| (the two products with rounded constants
                  and the quotient; dec_tail2.hip multiplies by a Newton-refined reciprocal instead: the same class), sin and cos
                  1-Lipschitz, + SINCOS_ABS = 4 U: csrc/dec_tail.hip and dec_tail2.hip call gom_sincos_0_2pi (common.h: Cody-Waite
                  reduction exact for q <= 4, cephes kernels on [-pi/4, pi/4], "within 1 ulp of 1"), not the fast __sinf / __cosf;
                  elementwise.hip's sinf / cosf (the four-launch path) are the precise ocml functions, inside the same constant.

Nothing in the bound was fitted to a GPU result.  The one outcome that needs a decision: worst-case propagation multiplies d by
sum_k |W[n, k]| at every product, so with unit-scale weights (sum |W| ~ 13 at K = 256) the bound behind three products is wide
enough to hold a mistake of the list in test_dec_statement_cpu.py.  Where that happened the INPUT was changed, not the bound:
every weight behind the first product of a launch is drawn with sum_k |W[n, k]| of about 1 to 3 (`_lin(.., gain)`), which keeps d at
the size of the first product's own error; the kinds `lowvar` and `offset` exist for the LayerNorm mistakes (eps, one-pass variance).
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
LN_DEPTH = 72
LN_DEPTH_BLOCK = 136
LN_RHO_MAX = 2.0 ** -4
SINCOS_ABS = 4 * U
D, NH, HD = 256, 8, 32
F32 = torch.float32


def d64(t):
    return None if t is None else torch.as_tensor(t).double()


# ------------------------------------------------------------------------------------------ steps: (value, error) -> (value, error)
def lin64(a, da, W, b=None, R=None, dR=None):
    """y = a W^T + b + R in float64 with the f16x3 contract's bound.  a, da [M, K] float64 (da may be None = exact input)."""
    W = d64(W)
    aW = a.abs() @ W.abs().T
    y = a @ W.T
    d = 2e-6 * aW + 1e-7 * W.abs().sum(1)
    if da is not None:
        d = d + da @ W.abs().T
    if b is not None:
        y = y + d64(b)
        d = d + 2e-6 * d64(b).abs()
    if R is not None:
        y = y + R
        d = d + 2e-6 * R.abs()
        if dR is not None:
            d = d + dR
    return y, d


def ln64(v, d, gamma, beta, eps, depth=LN_DEPTH):
    gamma, beta = d64(gamma), d64(beta)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    s = torch.sqrt(var + eps)
    z = (v - mean) / s
    y = z * gamma + beta
    rho = torch.sqrt((d * d).mean(-1, keepdim=True)) / s
    assert float(rho.max()) <= LN_RHO_MAX, "LayerNorm input error %.3e of the row's spread: beyond the bound's derivation" % float(rho.max())
    first = (d + d.mean(-1, keepdim=True) + z.abs() * (z.abs() * d).mean(-1, keepdim=True)) / s
    own = gamma.abs() * (depth + 1) * U * v.abs().mean(-1, keepdim=True) / s + (gamma * z).abs() * (depth / 2 + 9.5) * U + U * y.abs()
    return y, gamma.abs() * (first * (1 + 2 * rho) + 3 * rho * rho * z.abs()) + own


def attn64(q, dq, k, dk, v, dv):
    """[n, heads, G, hd] float64 each -> (o, d_o): softmax(q k^T / sqrt(hd)) v with the propagated bound of the module docstring."""
    hd, Lk = q.shape[-1], k.shape[-2]
    sc = 1.0 / math.sqrt(hd)
    qs, dqs = q * sc, dq * sc
    kt = k.transpose(-1, -2)
    s = qs @ kt
    dlt = s - s.max(-1, keepdim=True).values
    e = torch.exp(dlt)
    p = e / e.sum(-1, keepdim=True)
    o = p @ v
    E = (dqs @ kt.abs() + qs.abs() @ dk.transpose(-1, -2) + dqs @ dk.transpose(-1, -2)).max(-1, keepdim=True).values \
        + (hd + 2) * U * (qs.abs() @ kt.abs()).max(-1, keepdim=True).values
    va = v.abs()
    d = torch.expm1(2 * E) * (p @ va) + U * ((p * (dlt.abs() + 2 * Lk + 16)) @ va) + Lk * 2.0 ** -126 * va.amax((-1, -2), keepdim=True) + p @ dv
    return o, d


def _heads(t, index):
    n, G = index.shape
    return t[index].view(n, G, NH, HD).transpose(1, 2)


def _qkv64(x, pos, w, index, bug=None):
    in_w, in_b = w["in_w"], w["in_b"]
    x64 = d64(x)
    u = x64 if pos is None else x64 + d64(pos)
    du = None if pos is None else U * u.abs()                  # the fp32 sum x + pos
    q, dq = lin64(u, du, in_w[:256], in_b[:256])
    k, dk = lin64(u, du, in_w[256:512], in_b[256:512])
    v, dv = lin64(x64, None, in_w[512:], in_b[512:])
    return [_heads(t, index) for t in (q, dq, k, dk, v, dv)]


def heads64(x, pos, w, index):
    """The concatenated head outputs in front of out_proj, rows in index.reshape(-1) order -> (o, d_o) [n G, 256]."""
    n, G = index.shape
    o, do = attn64(*_qkv64(x, pos, w, index))
    return o.transpose(1, 2).reshape(n * G, D), do.transpose(1, 2).reshape(n * G, D)


def self_attn_block64(x, pos, w, index, eps=1e-5):
    """One self-attention block.  x [R, 256] float32, pos [R, 256] or None, w: dict of in_w [768, 256], in_b, out_w [256, 256], out_b,
    gamma, beta; index [groups, G]: the rows of every attention group (intra: consecutive rows; inter: `inter_index`).
    -> (y, bound) [groups G, 256], rows in index.reshape(-1) order."""
    o, do = heads64(x, pos, w, index)
    pre, dpre = lin64(o, do, w["out_w"], w["out_b"], R=d64(x)[index.reshape(-1)])
    return ln64(pre, dpre, w["gamma"], w["beta"], eps, depth=LN_DEPTH_BLOCK)


def raw64(y, dy, qpos, rw, rb):
    """(y + query_pos) Wraw^T + braw on the block's output y with its bound dy -> (raw, d_raw) [rows, 384]."""
    a = y + d64(qpos)
    return lin64(a, dy + U * a.abs(), rw, rb)


def proj_ln64(x, W, b, R, gamma, beta, eps=1e-5, dx=None):
    pre, d = lin64(d64(x), dx, W, b, R=d64(R))
    return ln64(pre, d, gamma, beta, eps)


def proj_ln_dot64(x, W, b, gamma, beta, cw, cb, eps=1e-5):
    y, dy = proj_ln64(x, W, b, None, gamma, beta, eps)
    cw = d64(cw)
    return y @ cw + cb, dy @ cw.abs() + (LN_DEPTH + 2) * U * (y.abs() @ cw.abs() + abs(cb))


def mlp2_64(x, w1, b1, w2, b2, relu_out, dx=None):
    h, dh = lin64(d64(x), dx, w1, b1)
    y, dy = lin64(torch.relu(h), dh, w2, b2)
    return (torch.relu(y) if relu_out else y), dy


def ffn_ln64(x, w1, b1, w2, b2, gamma, beta, eps=1e-5, dx=None):
    x = d64(x)
    h, dh = lin64(x, dx, w1, b1)
    pre, d = lin64(torch.relu(h), dh, w2, b2, R=x, dR=dx)
    return ln64(pre, d, gamma, beta, eps)


INV_EPS = float(np.float32(1e-5))                            # the clamp acts on float32 tensors: the constant is float32's


def inverse_sigmoid64(ref):
    r = d64(ref).clamp(0, 1)
    inv = torch.log(r.clamp(min=INV_EPS) / (1 - r).clamp(min=INV_EPS))
    return inv, 4 * U + 2 * U * inv.abs()


def sine_embed64(ref, dref, dim_t):
    """ref [M, 2] -> [M, 256]: per coordinate 128 channels, (sin, cos) interleaved on a pair that shares dim_t; x-half then y-half."""
    ang = ref[:, :, None] * (2 * math.pi) / d64(dim_t)[None, None, :]
    dang = dref[:, :, None] * (2 * math.pi) / d64(dim_t)[None, None, :] + 3 * U * ang.abs()
    emb = torch.stack((ang[:, :, 0::2].sin(), ang[:, :, 1::2].cos()), dim=3).flatten(2)
    demb = torch.stack((dang[:, :, 0::2], dang[:, :, 1::2]), dim=3).flatten(2) + SINCOS_ABS
    return torch.cat((emb[:, 0], emb[:, 1]), -1), torch.cat((demb[:, 0], demb[:, 1]), -1)


def tail64(x, ffn, coord, qpos, ref, dim_t, eps=1e-5, proj=None, residual=None, p_eps=None):
    """The row-local tail.  ffn = (w1, b1, w2, b2, gamma, beta), coord = three (W, b) with the last [2, 256], qpos = two (W, b);
    proj = (Wo, bo, gamma, beta) with residual: x are the sampled rows and LayerNorm_{p_eps}(residual + x Wo^T + bo) enters the FFN.
    -> ((tgt, d), (new_ref, d), (qpos, d))."""
    t, dt = d64(x), None
    if proj is not None:
        t, dt = proj_ln64(x, proj[0], proj[1], residual, proj[2], proj[3], eps if p_eps is None else p_eps)
    y, dy = ffn_ln64(t, *ffn, eps=eps, dx=dt)
    h, dh = mlp2_64(y, coord[0][0], coord[0][1], coord[1][0], coord[1][1], True, dx=dy)
    W3, b3 = d64(coord[2][0]), d64(coord[2][1])
    dd = h @ W3.T + b3
    ddd = dh @ W3.abs().T + (LN_DEPTH + 2) * U * (h.abs() @ W3.abs().T + b3.abs())
    inv, dinv = inverse_sigmoid64(ref)
    zz = dd + inv
    nr = torch.sigmoid(zz)
    dz = ddd + dinv + U * zz.abs()
    far = torch.sigmoid((zz.abs() - dz).clamp(min=0))                      # the largest slope on [|z| - d, |z| + d]: never above 1 / 4
    dnr = dz * far * (1 - far) + 6 * U
    emb, demb = sine_embed64(nr, dnr, dim_t)
    qp, dqp = mlp2_64(emb, qpos[0][0], qpos[0][1], qpos[1][0], qpos[1][1], False, dx=demb)
    return (y, dy), (nr, dnr), (qp, dqp)


def dim_t128():
    i = torch.arange(128, dtype=F32)
    return 10000.0 ** (2 * torch.div(i, 2, rounding_mode="trunc") / 128)


def inter_index(B, nq, P):
    """Rows of the inter-instance groups of x [B, nq, P, 256] flattened: group g = (b, p), token t -> row (b nq + t) P + p."""
    return torch.arange(B * nq * P).view(B, nq, P).permute(0, 2, 1).reshape(B * P, nq)


def intra_index(groups, G):
    return torch.arange(groups * G).view(groups, G)


# ------------------------------------------------------------------------------------------ inputs (same generators and seeds on CPU and GPU)
BLOCK_KINDS = ("randn", "peaked", "overflow", "same", "edge", "lowvar")
X_SCALE = {"randn": 1.0, "peaked": 3.0, "overflow": 6.0, "same": 1.0, "edge": 1.0, "lowvar": 0.03}
LN_KINDS = ("randn", "lowvar", "offset")
TAIL_KINDS = ("randn", "lowvar", "offset", "refedge")
REF_EDGES = (0.0, 1.0, 1e-7, 1 - 1e-6, 1e-5, 1 - 1e-5, 0.5, -3.0, 4.0)      # the issue's seven + two outside [0, 1] (the clamp)


def _lin(g, n, k, gain=1.0, bscale=0.1):
    """(W [n, k], b [n]): rows of randn with sum_k |W[n, k]| of about 2 `gain`, row scales over 0.5 .. 2 (two decades ^ 0.3)."""
    W = torch.randn(n, k, generator=g) * (2.5 * gain / k) * (torch.logspace(-1, 1, n) ** 0.3)[torch.randperm(n, generator=g)].view(-1, 1)
    return W, torch.randn(n, generator=g) * bscale


@functools.lru_cache(maxsize=None)
def block_weights(kind, seed=1):
    """in_proj as test_dec_attn_gpu._weights (randn / 16, row scales over two decades ^ 0.3); out_proj and the raw product behind
    it with sum |W| ~ 2.  `edge`: k's part of in_proj equals q's.  `lowvar`: biases x 0.03."""
    g = torch.Generator().manual_seed(seed)
    bs = 0.03 if kind == "lowvar" else 1.0
    in_w = torch.randn(768, 256, generator=g) / 16 * torch.logspace(-1, 1, 768).view(-1, 1) ** 0.3
    in_b = torch.randn(768, generator=g) * 0.1 * bs
    if kind == "edge":
        in_w[256:512], in_b[256:512] = in_w[:256], in_b[:256]
    out_w, out_b = _lin(g, 256, 256, bscale=0.1 * bs)
    raw_w, raw_b = _lin(g, 384, 256, bscale=0.1 * bs)
    w = {"in_w": in_w, "in_b": in_b, "out_w": out_w, "out_b": out_b, "gamma": torch.rand(256, generator=g) + 0.5,
         "beta": torch.randn(256, generator=g) * 0.1 * bs, "raw_w": raw_w, "raw_b": raw_b}
    return {k: v.contiguous() for k, v in w.items()}


def seams(G, layout):
    """Tokens of a group at which a form changes hands.  intra: the pair of waves (0..15 | 16..G-1); inter: form 1's four and form 2's
    eight waves of ceil(G / n) tokens; heads: csrc/dec_inter.hip's ceil(G / 32) blocks of ceil(G / nblk) tokens."""
    if layout == "intra":
        cand = [0, 15, 16, 17, G - 1]
    elif layout == "inter":
        p8, p4 = -(-G // 8), -(-G // 4)
        cand = [0, 15, 16, 17, 31, 32, p8 - 1, p8, G - p8, G - 1, p4 - 1, p4]
    else:
        per = -(-G // (-(-G // 32)))
        cand = [0, G - 1] + [e for b in range(per, G, per) for e in (b - 1, b)] + [31, 32]
    out = []
    for t in cand:
        if 0 <= t < G and t not in out:
            out.append(t)
    return out[:14]


def block_inputs(kind, rows, index, with_pos, seed, layout):
    """x [rows, 256] (and pos) float32 for an attention block whose groups are `index`; rows outside index stay randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, 256, generator=g) * X_SCALE[kind]
    pos = torch.randn(rows, 256, generator=g) * 0.7 * X_SCALE[kind] if with_pos else None
    n, G = index.shape
    if kind == "same":
        x[index.reshape(-1)] = x[index[:, :1]].expand(n, G, 256).reshape(-1, 256)
        if with_pos:
            pos[index.reshape(-1)] = pos[index[:, :1]].expand(n, G, 256).reshape(-1, 256)
    elif kind == "edge" and G >= 2:
        w = block_weights("edge")
        Wq, bq = w["in_w"][:256].double(), w["in_b"][:256].double()
        sm = seams(G, layout)
        owners = [t for t in range(G) if t not in sm][:len(sm)]
        if not owners:
            owners, sm = [0], [G - 1]
        for gi in range(n):
            ug = x[index[gi]].double() if pos is None else x[index[gi]].double() + pos[index[gi]].double()
            q = ug @ Wq.T + bq                                            # = k: the same part of in_proj (the group as drawn)
            sg = torch.einsum("ihc,jhc->hij", q.view(G, NH, HD), q.view(G, NH, HD)) / math.sqrt(HD)
            for o_, j in zip(owners, sm[gi % len(sm):] + sm[:gi % len(sm)]):
                s = sg[:, o_].clone()
                s[:, j] = float("-inf")
                lse = torch.logsumexp(s, -1).mean()                       # one c for the eight heads: the mean of their targets
                A = float((q[o_] * (ug[o_] @ Wq.T)).sum()) / NH / math.sqrt(HD)
                B0 = float((q[o_] * bq).sum()) / NH / math.sqrt(HD)
                new = (float(lse) - B0) / A * ug[o_]
                x[index[gi, j]] = (new if pos is None else new - pos[index[gi, j]].double()).float()
    return x.contiguous(), None if pos is None else pos.contiguous()


@functools.lru_cache(maxsize=None)
def ln_weights(kind, F=None, seed=3):
    """proj_ln (F None): (W, b, gamma, beta, cw, cb); ffn (F): (w1, b1, w2, b2, gamma, beta).  `offset`: the FFN's w1 scaled down so
    that the hidden layer stays moderate under x = 100 + randn; `lowvar`: biases x 0.03."""
    g = torch.Generator().manual_seed(seed + (F or 0))
    bs = 0.03 if kind == "lowvar" else 1.0
    ga, be = 1.0 + 0.2 * torch.randn(256, generator=g), 0.1 * bs * torch.randn(256, generator=g)
    if F is None:
        W, b = _lin(g, 256, 256, bscale=0.1 * bs)
        return W, b, ga, be, torch.randn(256, generator=g) * 0.1, -1.25
    w1, b1 = _lin(g, F, 256, gain=0.05 if kind == "offset" else 4.0, bscale=0.1 * bs)
    w2, b2 = _lin(g, 256, F, bscale=0.1 * bs)
    return w1, b1, w2, b2, ga, be


def rows_input(kind, M, seed):
    """(x, R) [M, 256]: randn; lowvar x 0.03; offset: R = 100 + randn (x stays randn: it is a product's operand)."""
    g = torch.Generator().manual_seed(seed)
    x, R = torch.randn(M, 256, generator=g), torch.randn(M, 256, generator=g)
    if kind == "lowvar":
        x, R = x * 0.03, R * 0.03
    elif kind == "offset":
        R = R + 100.0
    return x, R


@functools.lru_cache(maxsize=None)
def tail_weights(kind, F, seed=5):
    """-> (ffn, coord, qpos, proj).  refedge: the coordinate head's last layer scaled so that h spans +-20."""
    g = torch.Generator().manual_seed(seed + F)
    bs = 0.03 if kind == "lowvar" else 1.0
    w1, b1 = _lin(g, F, 256, gain=4.0, bscale=0.1 * bs)
    w2, b2 = _lin(g, 256, F, bscale=0.1 * bs)
    ffn = (w1, b1, w2, b2, 1.0 + 0.2 * torch.randn(256, generator=g), 0.1 * bs * torch.randn(256, generator=g))
    c1, c2 = _lin(g, 256, 256), _lin(g, 256, 256)
    W3, b3 = _lin(g, 2, 256, gain=600.0 if kind == "refedge" else 1.0)
    q1, q2 = _lin(g, 256, 256), _lin(g, 256, 256)
    Wo, bo = _lin(g, 256, 256, bscale=0.1 * bs)
    # lowvar: norm_cross's gain x 0.03 too, so that the FFN's rows (and norm3's variance) stay at 0.03 behind it
    proj = (Wo, bo, bs * (1.0 + 0.2 * torch.randn(256, generator=g)), 0.1 * bs * torch.randn(256, generator=g))
    return ffn, [c1, c2, (W3, b3)], [q1, q2], proj


def tail_input(kind, M, seed):
    """(x, residual, ref): x the FFN's input (or the sampled rows in front of out_proj), residual as rows_input's R."""
    x, R = rows_input(kind if kind != "refedge" else "randn", M, seed)
    g = torch.Generator().manual_seed(seed + 1)
    ref = torch.rand((M, 2), generator=g)
    if kind == "refedge":
        n = min(M, 4 * len(REF_EDGES))
        e = torch.tensor(REF_EDGES, dtype=F32)
        ref[:n, 0] = e[torch.arange(n) % len(e)]
        ref[:n, 1] = e[(torch.arange(n) // 2 + 3) % len(e)]
    return x, R, ref


def ffn_case(kind, M):
    """The fused FFN's input rows: `offset` is its residual path (x = 100 + randn, w1 scaled down by ln_weights)."""
    x, R = rows_input(kind, M, seed_of(M, 2))
    return R if kind == "offset" else x


def tail_case(kind, M, F, with_proj):
    """(x, residual | None, ref, eps) of one dec_tail call; eps = 3e-5 on TAIL_EPS_CASE, so that a hard-coded 1e-5 shows."""
    x, R, ref = tail_input(kind, M, seed_of(M, F))
    if not with_proj and kind == "offset":
        x = R                                                            # the FFN's own residual
    return x, (R if with_proj else None), ref, (3e-5 if (M, F) == TAIL_EPS_CASE else 1e-5)


# ------------------------------------------------------------------------------------------ case tables
INTRA_CASES = [(1, 1), (2, 15), (3, 16), (4, 17), (5, 25), (9, 31), (5, 32), (1, 32), (9, 16), (2, 25), (4, 31), (3, 1)]    # (groups, G)
# (B, nq, P): every nq with inner > 1 and with B > 1 at least once
INTER_CASES = [(2, 1, 2), (3, 7, 2), (2, 8, 5), (2, 9, 2), (2, 16, 2), (3, 17, 2), (2, 57, 2), (2, 64, 2), (2, 65, 2), (2, 100, 5),
               (2, 113, 2), (2, 120, 2), (2, 127, 2), (2, 128, 2), (1, 9, 1), (1, 57, 1), (1, 128, 1), (3, 65, 5)]
HEADS_CASES = [(1, 129, 3), (2, 160, 1), (1, 161, 3), (2, 257, 1), (1, 289, 3), (1, 300, 3), (2, 321, 1), (1, 352, 3),
               (2, 1, 3), (2, 33, 3), (1, 97, 1), (2, 97, 3)]
PROJ_LN_M = [1, 15, 16, 17, 63, 64, 65, 129, 1000]
FFN_M = [1, 63, 64, 65, 127, 128, 129, 1000]
FFN_F = [32, 96, 1024]
TAIL_M = [1, 15, 16, 17, 79, 80, 81, 127, 128, 129, 161, 1000]
TAIL_FORMS = {"form1": {"form": 1}, "form2-4waves": {"form": 2, "waves": 4}, "form2-8waves": {"form": 2, "waves": 8}}
TAIL_EPS_CASE = (81, 128)                                     # (M, F) run with DecTail(..., eps=3e-5) once per form


def tail_F(form):
    return (128, 1024, 96) if form == "form1" else (128, 1024)


def seed_of(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


def worst(got, exp, bound):
    """(largest |got - exp| / bound, its index): what a failing test prints.  A NaN counts as infinite."""
    r = (torch.as_tensor(got).double() - exp).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    at = int(r.reshape(-1).argmax()) if r.numel() else 0
    return (float(r.reshape(-1)[at]) if r.numel() else 0.0), at
