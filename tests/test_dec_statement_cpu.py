"""No GPU: what tests/dec_statement.py states, checked three ways.
  1. every statement against an independent float64 evaluation built from torch.nn.MultiheadAttention, nn.LayerNorm and F.linear;
  2. an fp32 EMULATION of the kernels' arithmetic (every product through test_f16x3_cpu's three-plane product, everything else in
     float32, the two-pass LayerNorm the kernels use) stays inside the bound on every table case and kind -- the bound does not
     refuse a correct implementation; the worst |err| / bound per op is printed;
  3. every planted mistake -- one changed line of the emulation, selected by `bug` -- breaks the bound on the case named beside it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dec_statement as S
from test_f16x3_cpu import gemm_f16x3, split

f32 = lambda a: np.asarray(a, np.float32)
npy = lambda t: None if t is None else t.detach().cpu().numpy()
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(RATIOS.items()):
        print("decoder emulation worst |err| / bound  %-14s %.4f" % (k, v))


def _note(op, r):
    RATIOS[op] = max(RATIOS.get(op, 0.0), r)


# ------------------------------------------------------------------------------------------ the emulation
def lin_emu(a, W, b=None, R=None, bug=None):
    a, W = f32(a), f32(npy(W) if torch.is_tensor(W) else W)
    if bug == "drop_low":
        a = split(a)[0].astype(np.float32)                               # a0 b0 + a0 b1 only
    y = f32(gemm_f16x3(a, W))
    if b is not None:
        y = y + f32(npy(b) if torch.is_tensor(b) else b)
    if R is not None:
        y = y + f32(R)
    return y


def prod3(a, b):
    """a [.., m, k] b^T [.., n, k] as the three-plane product without row scales (the attention core's operands are activations)."""
    a0, a1 = split(a)
    b0, b1 = split(b)
    d = lambda t: t.astype(np.float64)
    bt = lambda t: np.swapaxes(d(t), -1, -2)
    return f32(d(a1) @ bt(b0) + d(a0) @ bt(b1) + d(a0) @ bt(b0))


def ln_emu(v, gamma, beta, eps, bug=None):
    v, gamma, beta = f32(v), f32(npy(gamma)), f32(npy(beta))
    n = np.float32(v.shape[-1])
    mean = v.sum(-1, keepdims=True, dtype=np.float32) / n
    c = v - mean
    if bug == "onepass":
        var = (v * v).sum(-1, keepdims=True, dtype=np.float32) / n - mean * mean
    else:
        var = (c * c).sum(-1, keepdims=True, dtype=np.float32) / (n - 1 if bug == "var_dm1" else n)
    e = {"no_eps": 0.0, "eps1e-6": 1e-6}.get(bug, eps)
    rstd = np.float32(1) / np.sqrt(var + np.float32(e))
    return c * rstd * gamma + beta


def _gather_heads(t, index):
    n, G = index.shape
    return np.swapaxes(t[index.reshape(-1)].reshape(n, G, S.NH, S.HD), 1, 2)


def block_emu(x, pos, w, index, eps=1e-5, bug=None, heads_only=False, inner=1):
    """-> (y [n G, 256], raw_input) in index order; heads_only: the concatenated head outputs."""
    x = f32(npy(x))
    u = x if pos is None else x + f32(npy(pos))
    iw, ib = npy(w["in_w"]), npy(w["in_b"])
    q = lin_emu(u, iw[:256], ib[:256])
    k = lin_emu(x if bug == "no_pos_on_k" else u, iw[256:512], ib[256:512])
    v = lin_emu(u if bug == "pos_on_v" else x, iw[512:], ib[512:])
    idx = index.numpy()
    n, G = idx.shape
    if bug == "swap_inner":
        g, t = np.arange(n)[:, None], np.arange(G)[None, :]
        idx = (((g % inner) * G + t) * inner + g // inner) % x.shape[0]
    qh, kh, vh = (_gather_heads(t, idx) for t in (q, k, v))
    if bug == "other_head_v":
        vh = np.roll(vh, 1, axis=1)
    if bug == "key16_next_group":
        kh = kh.copy()
        kh[:, :, 16] = np.roll(kh, -1, axis=0)[:, :, 16]
    scale = np.float32(1.0 / math.sqrt(32.0))
    s = prod3(qh, kh) * (np.float32(1) if bug == "no_scale" else scale * scale if bug == "scale_twice" else scale)
    if bug == "drop_last_key":
        s[..., -1] = -np.inf
    m = np.zeros_like(s[..., :1]) if bug == "no_max" else s.max(-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(s - m, dtype=np.float32)
        l = e.sum(-1, keepdims=True, dtype=np.float32)
        o = prod3(e, np.swapaxes(vh, -1, -2)) / l
    o = np.swapaxes(o, 1, 2).reshape(n * G, 256)
    if heads_only:
        return o
    res = (u if bug == "res_x_plus_pos" else x)[idx.reshape(-1)]
    pre = lin_emu(o, w["out_w"], w["out_b"], R=res)
    return ln_emu(pre, w["gamma"], w["beta"], eps, bug), pre


def ffn_emu(x, ffn, eps=1e-5, bug=None):
    w1, b1, w2, b2, ga, be = ffn
    h = np.maximum(lin_emu(x, w1, b1), 0)
    if bug == "ffn_drop32":
        h[:, -32:] = 0
    return ln_emu(lin_emu(h, w2, b2, R=f32(x)), ga, be, eps, bug)


def mlp2_emu(x, w1, b1, w2, b2, relu_out, bug=None):
    y = lin_emu(np.maximum(lin_emu(x, w1, b1), 0), w2, b2)
    return np.maximum(y, 0) if (relu_out and bug != "relu_out_ignored") else y


def tail_emu(x, ffn, coord, qpos, ref, dim_t, eps=1e-5, proj=None, residual=None, p_eps=None, bug=None):
    x = f32(npy(x))
    p_eps = eps if p_eps is None else p_eps
    if bug == "swap_eps":
        eps, p_eps = p_eps, eps
    if bug == "swap_norms" and proj is not None:
        proj, ffn = proj[:2] + ffn[4:], ffn[:4] + proj[2:]
    if proj is not None:
        x = ln_emu(lin_emu(x, proj[0], proj[1], R=f32(npy(residual))), proj[2], proj[3], p_eps)
    y = ffn_emu(x, ffn, eps, bug if bug in ("ffn_drop32", "no_eps", "eps1e-6") else None)
    h = mlp2_emu(y, coord[0][0], coord[0][1], coord[1][0], coord[1][1], True, bug)
    W3, b3 = f32(npy(coord[2][0])), f32(npy(coord[2][1]))
    dd = h @ W3.T + b3
    r = f32(npy(ref))
    if bug != "no_ref_clamp":
        r = np.clip(r, np.float32(0), np.float32(1))
    lo = np.float32(1e-3 if bug == "clamp1e-3" else 1e-5)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.log(np.maximum(r, lo) / np.maximum(np.float32(1) - r, lo))
        nr = np.float32(1) / (np.float32(1) + np.exp(-(dd + inv), dtype=np.float32))
    dt = f32(npy(dim_t))
    if bug == "dim_t_i":
        dt = f32(10000.0 ** (np.arange(128, dtype=np.float64) / 128))
    ang = nr[:, :, None] * np.float32(1.0 if bug == "no_2pi" else 2 * math.pi) / dt[None, None, :]
    a, c = (np.cos, np.sin) if bug == "swap_sincos" else (np.sin, np.cos)
    emb = np.stack((a(ang[:, :, 0::2]), c(ang[:, :, 1::2])), axis=3).reshape(x.shape[0], 2, 128)
    emb = np.concatenate((emb[:, 1], emb[:, 0]) if bug == "swap_xy" else (emb[:, 0], emb[:, 1]), -1)
    return y, nr, mlp2_emu(emb, qpos[0][0], qpos[0][1], qpos[1][0], qpos[1][1], False)


def _ratio(got, eb):
    assert bool(torch.isfinite(eb[1]).all()) and float(eb[1].min()) > 0
    return S.worst(torch.from_numpy(np.ascontiguousarray(got)), eb[0], eb[1])[0]


# ------------------------------------------------------------------------------------------ 1. the statements against torch's modules
def _mha_block(x, pos, w, index):
    mha = torch.nn.MultiheadAttention(256, 8, batch_first=True).double()
    ln = torch.nn.LayerNorm(256, eps=1e-5).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(w["in_w"]); mha.in_proj_bias.copy_(w["in_b"])
        mha.out_proj.weight.copy_(w["out_w"]); mha.out_proj.bias.copy_(w["out_b"])
        ln.weight.copy_(w["gamma"]); ln.bias.copy_(w["beta"])
        t = x.double()[index]
        qk = t if pos is None else t + pos.double()[index]
        return ln(t + mha(qk, qk, t)[0]).reshape(-1, 256)


@pytest.mark.parametrize("layout,case", [("intra", (3, 17)), ("intra", (1, 1)), ("inter", (2, 9, 2)), ("inter", (3, 65, 5)), ("heads", (1, 129, 3))])
def test_block_statement_against_multihead_attention(layout, case):
    index = S.intra_index(*case) if layout == "intra" else S.inter_index(*case)
    rows = index.numel()
    for kind in ("randn", "peaked", "edge"):
        w = S.block_weights(kind)
        x, pos = S.block_inputs(kind, rows, index, layout == "intra", S.seed_of(*case), layout)
        y, _ = S.self_attn_block64(x, pos, w, index)
        ref = _mha_block(x, pos, w, index)
        assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        raw, _ = S.raw64(y, torch.zeros_like(y), x, w["raw_w"], w["raw_b"])
        assert float((raw - F.linear(ref + x.double(), w["raw_w"].double(), w["raw_b"].double())).abs().max()) <= 1e-12 * float(raw.abs().max())


@pytest.mark.parametrize("kind", S.TAIL_KINDS)
def test_row_statements_against_functional(kind):
    M = 81
    d = lambda t: t.double()
    W, b, ga, be, cw, cb = S.ln_weights(kind)
    x, R = S.rows_input(kind, M, 5)
    k = kind if kind in S.LN_KINDS else "randn"
    ref = F.layer_norm(F.linear(d(x), d(W), d(b)) + d(R), (256,), d(ga), d(be), 1e-5)
    assert float((S.proj_ln64(x, W, b, R, ga, be)[0] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    ref = F.layer_norm(F.linear(d(x), d(W), d(b)), (256,), d(ga), d(be), 1e-5)
    assert float((S.proj_ln_dot64(x, W, b, ga, be, cw, cb)[0] - (ref @ d(cw) + cb)).abs().max()) <= 1e-12 * float(ref.abs().max()) * 16
    ffn, coord, qpos, proj = S.tail_weights(kind, 128)
    x, R, ref_pts = S.tail_input(kind, M, 7)
    (y, _), (nr, _), (qp, _) = S.tail64(x, ffn, coord, qpos, ref_pts, S.dim_t128(), proj=proj, residual=R)
    t = F.layer_norm(d(R) + F.linear(d(x), d(proj[0]), d(proj[1])), (256,), d(proj[2]), d(proj[3]), 1e-5)
    t = F.layer_norm(t + F.linear(F.relu(F.linear(t, d(ffn[0]), d(ffn[1]))), d(ffn[2]), d(ffn[3])), (256,), d(ffn[4]), d(ffn[5]), 1e-5)
    h = t
    for i, (w_, b_) in enumerate(coord):
        h = F.linear(h, d(w_), d(b_))
        h = F.relu(h) if i < 2 else h
    r = ref_pts.clamp(0, 1)                                               # in float32, as the reference computes it
    inv = torch.log(r.clamp(min=1e-5).double() / (1 - d(r)).clamp(min=float(np.float32(1e-5))))
    want = torch.sigmoid(h + inv)
    assert float((y - t).abs().max()) <= 1e-12 * float(t.abs().max())
    assert float((nr - want).abs().max()) <= 1e-12
    pos = want[:, :, None] * (2 * math.pi) / d(S.dim_t128())
    px = torch.stack((pos[:, 0, 0::2].sin(), pos[:, 0, 1::2].cos()), dim=2).flatten(1)
    py = torch.stack((pos[:, 1, 0::2].sin(), pos[:, 1, 1::2].cos()), dim=2).flatten(1)
    q = F.linear(F.relu(F.linear(torch.cat((px, py), -1), d(qpos[0][0]), d(qpos[0][1]))), d(qpos[1][0]), d(qpos[1][1]))
    assert float((qp - q).abs().max()) <= 1e-12 * float(q.abs().max())


# ------------------------------------------------------------------------------------------ 2. the emulation inside the bound
def _block_case(layout, case, kind):
    index = S.intra_index(*case) if layout == "intra" else S.inter_index(*case)
    rows = index.numel() + (3 if layout == "intra" else 0)
    x, pos = S.block_inputs(kind, rows, index, layout == "intra", S.seed_of(*case), layout)
    return index, x, pos, S.block_weights(kind)


@pytest.mark.parametrize("layout,cases", [("intra", S.INTRA_CASES), ("inter", S.INTER_CASES), ("heads", S.HEADS_CASES)])
@pytest.mark.parametrize("kind", S.BLOCK_KINDS)
def test_block_emulation_stays_inside_the_bound(layout, cases, kind):
    for case in cases:
        index, x, pos, w = _block_case(layout, case, kind)
        y, pre = block_emu(x, pos, w, index)
        exp = S.self_attn_block64(x, pos, w, index)
        _note(layout, _ratio(y, exp))
        if layout == "heads":
            _note("heads alone", _ratio(block_emu(x, pos, w, index, heads_only=True), S.heads64(x, pos, w, index)))
        if layout == "inter":
            qp = S.rows_input(kind if kind == "lowvar" else "randn", index.numel(), 11)[1] * 0.7
            raw = lin_emu(y + f32(npy(qp)), w["raw_w"], w["raw_b"])
            _note("raw", _ratio(raw, S.raw64(exp[0], exp[1], qp, w["raw_w"], w["raw_b"])))
    assert all(v <= 1.0 for v in RATIOS.values()), RATIOS


@pytest.mark.parametrize("kind", S.LN_KINDS)
def test_row_op_emulations_stay_inside_the_bound(kind):
    W, b, ga, be, cw, cb = S.ln_weights(kind)
    for M in S.PROJ_LN_M:
        x, R = S.rows_input(kind, M, S.seed_of(M, 1))
        _note("proj_ln", _ratio(ln_emu(lin_emu(x, W, b, R=npy(R)), ga, be, 1e-5), S.proj_ln64(x, W, b, R, ga, be)))
        if kind != "offset":                                              # offset is the residual path's kind
            y = ln_emu(lin_emu(x, W, b), ga, be, 1e-5)
            _note("proj_ln none", _ratio(y, S.proj_ln64(x, W, b, None, ga, be)))
            _note("proj_ln_dot", _ratio(y @ f32(npy(cw)) + np.float32(cb), S.proj_ln_dot64(x, W, b, ga, be, cw, cb)))
    for M in S.FFN_M:
        x, xin = S.rows_input(kind, M, S.seed_of(M, 2))[0], S.ffn_case(kind, M)
        for Fh in S.FFN_F:
            ffn = S.ln_weights(kind, Fh)
            _note("ffn_ln", _ratio(ffn_emu(npy(xin), ffn), S.ffn_ln64(xin, *ffn)))
        if kind != "offset":
            w1, b1, w2, b2 = S.ln_weights(kind, 256)[:4]
            for ro in (False, True):
                _note("mlp2", _ratio(mlp2_emu(npy(x), w1, b1, w2, b2, ro), S.mlp2_64(x, w1, b1, w2, b2, ro)))
    assert all(v <= 1.0 for v in RATIOS.values()), RATIOS


@pytest.mark.parametrize("with_proj", [False, True], ids=["plain", "proj"])
@pytest.mark.parametrize("kind", S.TAIL_KINDS)
def test_tail_emulation_stays_inside_the_bound(kind, with_proj):
    dim_t = S.dim_t128()
    for Fh in S.tail_F("form1"):
        ffn, coord, qpos, proj = S.tail_weights(kind, Fh)
        for M in S.TAIL_M:
            x, R, ref, eps = S.tail_case(kind, M, Fh, with_proj)
            kw = dict(proj=proj, residual=R) if with_proj else {}
            got = tail_emu(x, ffn, coord, qpos, ref, dim_t, eps=eps, **kw)
            exp = S.tail64(x, ffn, coord, qpos, ref, dim_t, eps=eps, **kw)
            for name, g_, e_ in zip(("tail tgt", "tail ref", "tail qpos"), got, exp):
                _note(name, _ratio(g_, e_))
            if kind == "refedge" and M == 1000:                           # the kind is what it says: the sigmoid saturates on both sides
                assert float(exp[1][0].min()) < 1e-4 and float(exp[1][0].max()) > 1 - 1e-4
    assert all(RATIOS[k] <= 1.0 for k in ("tail tgt", "tail ref", "tail qpos")), RATIOS


# ------------------------------------------------------------------------------------------ 3. the planted mistakes
BLOCK_BUGS = [  # bug, layout, table case, kind
    ("no_eps", "intra", (5, 25), "lowvar"), ("eps1e-6", "inter", (2, 100, 5), "lowvar"), ("var_dm1", "intra", (4, 17), "randn"),
    ("no_max", "inter", (2, 64, 2), "overflow"), ("no_max", "intra", (5, 32), "overflow"),
    ("no_scale", "intra", (5, 25), "randn"), ("scale_twice", "inter", (2, 57, 2), "peaked"),
    ("pos_on_v", "intra", (4, 17), "randn"), ("no_pos_on_k", "intra", (9, 31), "randn"), ("res_x_plus_pos", "intra", (2, 15), "randn"),
    ("drop_last_key", "inter", (2, 65, 2), "edge"), ("drop_last_key", "heads", (2, 257, 1), "edge"),
    ("key16_next_group", "intra", (4, 17), "edge"), ("swap_inner", "inter", (2, 8, 5), "randn"), ("other_head_v", "inter", (3, 7, 2), "randn"),
]


@pytest.mark.parametrize("bug,layout,case,kind", BLOCK_BUGS, ids=["%s-%s" % (b[0], b[1]) for b in BLOCK_BUGS])
def test_planted_block_mistake_breaks_the_bound(bug, layout, case, kind):
    index, x, pos, w = _block_case(layout, case, kind)
    if layout == "heads":
        got, exp = block_emu(x, pos, w, index, bug=bug, heads_only=True), S.heads64(x, pos, w, index)
    else:
        got, exp = block_emu(x, pos, w, index, bug=bug, inner=case[-1])[0], S.self_attn_block64(x, pos, w, index)
    r = _ratio(got, exp)
    print("planted %-18s caught on %s %s %s: |err| / bound = %.3g" % (bug, layout, case, kind, r))
    assert r > 1.0


def test_planted_raw_mistakes_break_the_bound():
    case, kind = (2, 16, 2), "randn"
    index, x, _, w = _block_case("inter", case, kind)
    qp = S.rows_input("randn", index.numel(), 11)[1] * 0.7
    y, pre = block_emu(x, None, w, index)
    exp = S.self_attn_block64(x, None, w, index)
    want = S.raw64(exp[0], exp[1], qp, w["raw_w"], w["raw_b"])
    assert _ratio(lin_emu(y + f32(npy(qp)), w["raw_w"], w["raw_b"]), want) <= 1.0
    for bug, a in (("raw without query_pos", y), ("raw from the pre-norm rows", pre + f32(npy(qp)))):
        r = _ratio(lin_emu(a, w["raw_w"], w["raw_b"]), want)
        print("planted %-28s caught on inter %s %s: %.3g" % (bug, case, kind, r))
        assert r > 1.0


ROW_BUGS = [  # bug, op, M, F, kind
    ("no_eps", "proj_ln", 65, None, "lowvar"), ("eps1e-6", "ffn_ln", 129, 96, "lowvar"), ("var_dm1", "proj_ln", 17, None, "randn"),
    ("onepass", "proj_ln", 1000, None, "offset"), ("onepass", "ffn_ln", 128, 1024, "offset"),
    ("ffn_drop32", "ffn_ln", 65, 1024, "randn"), ("ffn_drop32", "ffn_ln", 63, 96, "randn"), ("relu_out_ignored", "mlp2", 64, None, "randn"),
    ("drop_low", "proj_ln", 129, None, "randn"),
]


@pytest.mark.parametrize("bug,op,M,Fh,kind", ROW_BUGS, ids=["%s-%s" % (b[0], b[1]) for b in ROW_BUGS])
def test_planted_row_op_mistake_breaks_the_bound(bug, op, M, Fh, kind):
    if op == "proj_ln":
        W, b, ga, be, _, _ = S.ln_weights(kind)
        x, R = S.rows_input(kind, M, S.seed_of(M, 1))
        got, exp = ln_emu(lin_emu(x, W, b, R=npy(R), bug=bug), ga, be, 1e-5, bug), S.proj_ln64(x, W, b, R, ga, be)
    elif op == "ffn_ln":
        xin, ffn = S.ffn_case(kind, M), S.ln_weights(kind, Fh)
        got, exp = ffn_emu(npy(xin), ffn, bug=bug), S.ffn_ln64(xin, *ffn)
    else:
        x, _ = S.rows_input(kind, M, S.seed_of(M, 2))
        w1, b1, w2, b2 = S.ln_weights(kind, 256)[:4]
        got, exp = mlp2_emu(npy(x), w1, b1, w2, b2, True, bug), S.mlp2_64(x, w1, b1, w2, b2, True)
    r = _ratio(got, exp)
    print("planted %-18s caught on %s M=%d F=%s %s: |err| / bound = %.3g" % (bug, op, M, Fh, kind, r))
    assert r > 1.0


TAIL_BUGS = [  # bug, M, F, kind, with_proj, eps, p_eps, which output shows it (0 tgt, 1 ref, 2 qpos)
    ("swap_eps", 81, 128, "lowvar", True, 3e-5, 1e-5, 0), ("no_eps", 129, 128, "lowvar", False, 1e-5, None, 0),
    ("eps1e-6", 80, 1024, "lowvar", False, 1e-5, None, 0), ("ffn_drop32", 17, 128, "randn", False, 1e-5, None, 0),
    ("relu_out_ignored", 79, 128, "refedge", False, 1e-5, None, 1), ("swap_norms", 16, 128, "randn", True, 1e-5, None, 0),
    ("clamp1e-3", 81, 128, "refedge", False, 1e-5, None, 1), ("no_ref_clamp", 127, 128, "refedge", False, 1e-5, None, 1),
    ("swap_sincos", 15, 128, "randn", False, 1e-5, None, 2), ("swap_xy", 15, 1024, "randn", False, 1e-5, None, 2),
    ("no_2pi", 128, 128, "randn", False, 1e-5, None, 2), ("dim_t_i", 161, 128, "randn", False, 1e-5, None, 2),
]


@pytest.mark.parametrize("bug,M,Fh,kind,with_proj,eps,p_eps,out", TAIL_BUGS, ids=[b[0] for b in TAIL_BUGS])
def test_planted_tail_mistake_breaks_the_bound(bug, M, Fh, kind, with_proj, eps, p_eps, out):
    ffn, coord, qpos, proj = S.tail_weights(kind, Fh)
    x, R, ref = S.tail_input(kind, M, S.seed_of(M, Fh))
    kw = dict(proj=proj, residual=R, p_eps=p_eps) if with_proj else {}
    exp = S.tail64(x, ffn, coord, qpos, ref, S.dim_t128(), eps=eps, **kw)
    good = tail_emu(x, ffn, coord, qpos, ref, S.dim_t128(), eps=eps, **kw)
    assert all(_ratio(g_, e_) <= 1.0 for g_, e_ in zip(good, exp))
    got = tail_emu(x, ffn, coord, qpos, ref, S.dim_t128(), eps=eps, bug=bug, **kw)
    r = _ratio(got[out], exp[out])
    print("planted %-18s caught on tail M=%d F=%d %s%s, output %d: |err| / bound = %.3g" % (bug, M, Fh, kind, " +proj" if with_proj else "", out, r))
    assert r > 1.0
