"""Shared builders for the parity tests (configs/weights identical to oracle/gen_golden.py)."""
import os

import numpy as np
import torch

from gomatching_amd.config import setup_cfg
from gomatching_amd.weights import synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MINI_NQ = 12


def mini_cfg(builtin="icdar15", nq=MINI_NQ, voc=None, device="cpu"):
    cfg = setup_cfg(builtin=builtin)
    cfg.MODEL.DEVICE = device
    cfg.MODEL.TRANSFORMER.NUM_QUERIES = nq
    if voc is not None:
        cfg.MODEL.TRANSFORMER.VOC_SIZE = voc
    return cfg


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def e2e_state_dict(cfg, gold):
    bias = {"detection_transformer.ctrl_point_class.0.bias": float(gold["cls_bias"][0])}
    if cfg.MODEL.ROI_HEADS.WITH_RESR:
        bias["roi_heads.rescoring_head.bias"] = float(gold["cls_bias"][1])
    return synth_state_dict(cfg, seed=7, cls_bias=bias)


def t(x):
    return torch.from_numpy(np.asarray(x))


TIE_EPS = 1e-4


def track_clip_tie_aware(sd, cfg, raw, want_ids, eps=TIE_EPS, max_runs=24):
    """The oracle's tracker over the detections `raw` (a list of oracle `Inst`s: copied for every replay), compared with
    `want_ids` (per frame, the ids another implementation gave the SAME detections).  north_star's bar is identical track
    assignment; the tracker's decisions are discrete (linear-sum assignment on -traj, then `traj > thr`:
    gom_lstmatcher.py:434-452, 521-554), so two correct fp32 evaluations can part at a near-tie.  Rule (the tracker's twin of
    test_clips_fullsize_gpu._rank_swaps): the ids must be identical, OR every decision at which they part sits on a gap below `eps`
    in the ORACLE's own traj matrix (assignment total vs the best different assignment, or |traj - thr|), and the oracle replayed
    with exactly those decisions taken the other way reproduces EVERY id of every later frame.
    -> (instances, id_count, report); report["forced"] lists the decisions taken the other way with their gaps (empty = plain
    identity), report["margins"] the smallest assignment gap / threshold margin over the clip."""
    import copy
    from oracle import gom_oracle as O
    want = [list(map(int, w)) for w in want_ids]
    runs = [0]

    def replay(script):
        runs[0] += 1
        log = O.MatchLog(eps=eps, script=script)
        with torch.no_grad():
            inst, count = O.track_clip(sd, cfg, copy.deepcopy(raw), log=log)
        got = [x["track_ids"].tolist() for x in inst]
        bad = [f for f, (g, w) in enumerate(zip(got, want)) if g != w]
        return inst, count, log, (bad[0] if bad else None)

    def search(script):
        inst, count, log, f = replay(script)
        if f is None:
            return inst, count, log
        for idx, c in enumerate(log.calls):                             # a decision of the first frame that differs, not yet forced
            if c["frame"] != f or idx in script:
                continue
            for k in range(1, c["n_alt"] + 1):
                if runs[0] >= max_runs:
                    return None
                res = search({**script, idx: k})
                if res is not None:
                    return res
        return None

    first = replay({})
    res = (first[0], first[1], first[2]) if first[3] is None else search({})
    assert res is not None, ("track ids differ from the oracle's at frame %d and no decision of that frame sits on a gap below %g "
                             "(margins of that frame: %s)" % (first[3], eps, [c for c in first[2].calls if c["frame"] == first[3]]))
    inst, count, log = res
    forced = [dict(c, call=i) for i, c in enumerate(log.calls) if c["picked"]]
    assert all(c["picked_gap"] < eps for c in forced)
    return inst, count, {"forced": forced, "margins": first[2].summary(), "replays": runs[0]}


# ------------------------------------------------------------------------------------------ MSDA statement
def msda64(value, shapes, lsi, loc, w, q_chunk=256):
    """fp64 statement of the native MSDA op, the reference's kernel (ms_deform_im2col_cuda.cuh:33-84 bilinear, :237-299;
    restated in oracle.gom_oracle.ms_deform_attn_forward): value [B,S,M,D], shapes [L,2] (H, W), lsi [L], loc [B,Lq,M,L,P,2]
    float32 (x, y), w [B,Lq,M,L,P] -> [B,Lq,M*D] float64.

    The pixel coordinates h_im = y*H - 0.5 and w_im = x*W - 0.5 are computed in fp32, one rounding per operation, as the
    reference's kernel writes them.  Everything after that is float64: the acceptance window (-1, H) x (-1, W), floor, corner
    validity, corner weights and the accumulation over levels and points.  A sample outside the window adds nothing, NaN and
    inf coordinates included (the kernel branches around it).  Queries are processed `q_chunk` at a time (rows are independent)."""
    value = torch.as_tensor(value).double()
    loc = torch.as_tensor(loc)
    assert loc.dtype == torch.float32, "the pixel coordinates are an fp32 computation: loc must be float32"
    w = torch.as_tensor(w).double()
    B, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    hw = [(int(h), int(w_)) for h, w_ in torch.as_tensor(shapes).tolist()]
    starts = [int(s) for s in torch.as_tensor(lsi).tolist()]
    vflat = value.reshape(B * S * M, D)
    bm = (torch.arange(B).view(B, 1, 1, 1) * S) * M + torch.arange(M).view(1, 1, M, 1)   # row of (b, s = 0, m)
    out = torch.zeros((B, Lq, M, D), dtype=torch.float64)
    for q0 in range(0, Lq, q_chunk):
        q1 = min(Lq, q0 + q_chunk)
        n = q1 - q0
        for l, (H, W) in enumerate(hw):
            lc = loc[:, q0:q1, :, l]                                      # B,n,M,P,2 float32
            w_im = (lc[..., 0] * W - 0.5).double()                        # fp32 multiply, fp32 subtract, then exact widening
            h_im = (lc[..., 1] * H - 0.5).double()
            inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)  # False for NaN
            h_im = torch.where(inside, h_im, torch.zeros_like(h_im))
            w_im = torch.where(inside, w_im, torch.zeros_like(w_im))
            h_low, w_low = torch.floor(h_im), torch.floor(w_im)
            lh, lw = h_im - h_low, w_im - w_low
            hh, hw_ = 1 - lh, 1 - lw
            h_low, w_low = h_low.long(), w_low.long()
            acc = torch.zeros((B, n, M, P, D), dtype=torch.float64)
            for dy, dx, wt in ((0, 0, hh * hw_), (0, 1, hh * lw), (1, 0, lh * hw_), (1, 1, lh * lw)):
                yy, xx = h_low + dy, w_low + dx
                ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                idx = starts[l] + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
                v = vflat.index_select(0, (idx * M + bm).reshape(-1)).view(B, n, M, P, D)
                acc += v * torch.where(ok, wt, torch.zeros_like(wt))[..., None]
            out[:, q0:q1] += (acc * w[:, q0:q1, :, l, :, None]).sum(3)
    return out.reshape(B, Lq, M * D)


def msda_locations32(raw, ref, shapes, vr=None):
    """Sampling locations of the fused MSDA forms, IEEE fp32 in numpy (ms_deform_attn.py:141-147; the valid ratios of a padded
    batch scale the reference point first, deformable_transformer.py:262-263 / 470-472):
        loc = fl32(fl32(ref * vr_l) + fl32(off / (W_l, H_l)))
    raw [Q, >=384] (8 heads x 4 levels x 4 points x (x, y) offsets | 128 logits), ref [Q, 2] or [Q, Lr, 2] (Lr = 1 or 4),
    vr [4, 2] (x, y) or None -> [Q, 8, 4, 4, 2] float32."""
    raw = np.asarray(raw, dtype=np.float32)
    Q = raw.shape[0]
    off = raw[:, :256].reshape(Q, 8, 4, 4, 2)
    norm = np.array([[w_, h] for h, w_ in np.asarray(shapes).tolist()], dtype=np.float32)       # (W_l, H_l)
    r = np.asarray(ref, dtype=np.float32).reshape(Q, 1, -1, 1, 2)
    if vr is not None:
        r = r * np.asarray(vr, dtype=np.float32).reshape(1, 1, 4, 1, 2)
    return r + off / norm[None, None, :, None, :]


def msda_softmax64(raw):
    """Attention weights of the fused MSDA forms: the softmax of each head's 16 logits in float64.  raw [Q, >=384] ->
    (w [Q, 8, 4, 4] float64, d [Q, 8, 4, 4] = logit - the head's largest logit)."""
    raw = np.asarray(raw, dtype=np.float32)
    Q = raw.shape[0]
    lg = raw[:, 256:384].reshape(Q, 8, 16).astype(np.float64)
    d = lg - lg.max(-1, keepdims=True)
    e = np.exp(d)
    return (e / e.sum(-1, keepdims=True)).reshape(Q, 8, 4, 4), d.reshape(Q, 8, 4, 4)


def msda64_fused(value, shapes, lsi, raw, ref, B, Lq, vr=None):
    """fp64 statement of the fused MSDA forms: msda64 on msda_locations32 and msda_softmax64.  value [B,S,8,32],
    raw [B*Lq, >=384], ref [B*Lq, 2] -> [B*Lq, 256] float64."""
    loc = torch.from_numpy(msda_locations32(raw, ref, shapes, vr)).view(B, Lq, 8, 4, 4, 2)
    w = torch.from_numpy(msda_softmax64(raw)[0]).view(B, Lq, 8, 4, 4)
    return msda64(value, shapes, lsi, loc, w).view(B * Lq, 256)


# ------------------------------------------------------------------------------------------ attention statement
ATTN_U = 2.0 ** -24


def attention64(q, k, v, head_dim):
    """fp64 statement of the softmax attention core (csrc/attn.hip, mha_tiny128_task of csrc/tracker_tasks.h) with its element-wise
    error bound.  q [..., Lq, hd], k and v [..., Lk, hd] float32 (leading dimensions = independent (batch, head) problems) ->
    (exp, bound) float64 [..., Lq, hd].

        qs = fp32(q * fp32(1 / sqrt(head_dim))), widened  (the kernels pre-scale q in fp32; for 32 and 128 that constant has the
             bits of the kernels' 1.0f / sqrtf(head_dim))
        s = qs k^T,  m = rowmax(s),  p = exp(s - m) / sum,  exp = p v                      all float64

        bound[i,d] = sum_j p_ij |v_jd| (2 E_i + (|s_ij - m_i| + 2 Lk + 16) U) + Lk 2^-126 max|v|,      U = 2^-24
        E_i = (head_dim + 2) U max_j sum_d |qs_id k_jd|

    E_i: one fmaf chain of head_dim terms plus the pre-scale rounding -- an absolute error of a logit, which enters every p_j once
    directly and once through the normaliser (2 E_i).  |s - m| U: the rounding of expf's argument.  2 Lk: the sequential sum of
    the exponentials (the row-per-lane kernel's) plus the sequential P V fmaf chain.  16: expf, the reciprocal, the product, the
    butterflies.  Last term: weights below fp32's normal range.  Derived from the operation count; nothing in it was measured."""
    q, k, v = torch.as_tensor(q), torch.as_tensor(k), torch.as_tensor(v)
    assert q.dtype == k.dtype == v.dtype == torch.float32, "the pre-scale is an fp32 computation: inputs must be float32"
    Lk = k.shape[-2]
    qs = (q * torch.tensor(1.0 / np.sqrt(head_dim), dtype=torch.float32)).double()
    k64, va = k.double(), v.double().abs()
    s = qs @ k64.transpose(-1, -2)
    d = s - s.max(-1, keepdim=True).values
    e = torch.exp(d)
    p = e / e.sum(-1, keepdim=True)
    exp = p @ v.double()
    E = (head_dim + 2) * ATTN_U * (qs.abs() @ k64.abs().transpose(-1, -2)).max(-1, keepdim=True).values      # [..., Lq, 1]
    bound = 2 * E * (p @ va) + ATTN_U * ((p * (d.abs() + 2 * Lk + 16)) @ va) + Lk * 2.0 ** -126 * va.amax((-1, -2), keepdim=True)
    return exp, bound


def attn_index(offset, bo, bi, ss, outer, inner, heads, hd, L, size=None):
    """Element indices [outer * inner, heads, L, hd] of one operand of the op: batch b = (b // inner, b % inner) with strides
    (bo, bi), sequence stride ss, head h at column h * hd.  `size`: wrap the indices into a buffer of that many elements (only
    the planted stride mistake of the CPU file walks out of its buffer)."""
    b = torch.arange(outer * inner)
    idx = (offset + (b // inner) * bo + (b % inner) * bi).view(-1, 1, 1, 1) + (torch.arange(heads) * hd).view(1, -1, 1, 1) \
        + (torch.arange(L) * ss).view(1, 1, -1, 1) + torch.arange(hd).view(1, 1, 1, -1)
    return idx if size is None else idx % size


def attention64_views(qbuf, kbuf, vbuf, outer, inner, heads, hd, Lq, Lk, strides, offsets=(0, 0, 0)):
    """attention64 over batch and heads on the op's own views: flat float32 buffers, the 12 strides gom_mha_core_f32 takes (q, k, v,
    o x (outer, inner, sequence)) and the element offset of each operand in its buffer -> (exp, bound) [outer*inner, heads, Lq, hd].
    What the views address must be finite: the statement reads exactly the elements the op may read."""
    got = []
    for buf, off, st, L in ((qbuf, offsets[0], strides[0:3], Lq), (kbuf, offsets[1], strides[3:6], Lk), (vbuf, offsets[2], strides[6:9], Lk)):
        x = buf[attn_index(off, st[0], st[1], st[2], outer, inner, heads, hd, L)]
        assert bool(torch.isfinite(x).all())
        got.append(x)
    return attention64(got[0], got[1], got[2], hd)


# ---- inputs of tests/test_attn_forms_gpu.py, shared with tests/test_attn_statement_cpu.py (same generators, same seeds, same bits)
ATTN_KINDS = ("randn", "peaked", "overflow", "same", "widev", "edge")


def attn_edges(Lk):
    """Keys on which a tail tile, a 64-key tile edge or the first / last key goes wrong, the ones a planted mistake needs first."""
    out = []
    for e in (Lk - 1, 63, 64, 0, 65, Lk - 65, Lk - 64):
        if 0 <= e < Lk and e not in out:
            out.append(e)
    return out


def attn_inputs(kind, nb, heads, hd, Lq, Lk, seed):
    """q [nb, heads, Lq, hd], k and v [nb, heads, Lk, hd] float32.
      randn     unit normal
      peaked    q x 8: a few keys hold a row's weight
      overflow  q x 40, k x 3: logits in the hundreds -- exp without the max subtraction overflows
      same      every key of a (batch, head) identical: the output is the mean of v
      widev     v x e^U(-10, 10), element-wise: nine decades of magnitude in one sum
      edge      randn, then the first rows of every (batch, head) each own one key of attn_edges(Lk), cycling over (batch, head,
                row) so that every edge key is owned somewhere: the key is set to alpha q_i sqrt(hd) / |q_i|^2, its logit alpha =
                the log-sum-exp of the row's other randn logits, so that it holds about half of the row's weight (about: the
                keys that other rows of the same (batch, head) own are set afterwards and take a little of it).  Dropping, misplacing or
                mis-scaling that key then moves the row by a large part of |v| -- where a one-hot row or a row of Lk equal weights
                moves by nothing, or by 1 / Lk."""
    assert kind in ATTN_KINDS
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nb, heads, Lq, hd, generator=g)
    k = torch.randn(nb, heads, Lk, hd, generator=g)
    v = torch.randn(nb, heads, Lk, hd, generator=g)
    if kind == "peaked":
        q = q * 8
    elif kind == "overflow":
        q, k = q * 40, k * 3
    elif kind == "same":
        k = k[:, :, :1].expand(nb, heads, Lk, hd).contiguous()
    elif kind == "widev":
        v = v * torch.exp(torch.rand(nb, heads, Lk, hd, generator=g) * 20 - 10)
    elif kind == "edge" and Lk >= 2:
        edges = attn_edges(Lk)
        n = min(Lq, len(edges))
        qs = (q[:, :, :n] * torch.tensor(1.0 / np.sqrt(hd), dtype=torch.float32)).double()
        s = qs @ k.double().transpose(-1, -2)                             # the randn keys' logits [nb, heads, n, Lk]
        own = (torch.arange(n).view(1, 1, n) + (torch.arange(nb).view(nb, 1, 1) * heads + torch.arange(heads).view(1, heads, 1)) * n) % len(edges)
        own = torch.tensor(edges)[own]                                    # [nb, heads, n] the key row i owns
        alpha = torch.logsumexp(s.scatter(-1, own.unsqueeze(-1), float("-inf")), -1)
        q64 = q[:, :, :n].double()
        new = (alpha * np.sqrt(hd) / (q64 * q64).sum(-1)).unsqueeze(-1) * q64                      # [nb, heads, n, hd]
        k = k.scatter(2, own.unsqueeze(-1).expand(nb, heads, n, hd), new.float())
    return q.contiguous(), k.contiguous(), v.contiguous()


def attn_layout(view, outer, inner, heads, hd, Lq, Lk, odd_out=False):
    """Where q, k, v and the output live for one call.  -> dict: sizes {buffer: floats}, where {q|k|v: (buffer, offset)}, strides
    (the op's 12), out_size.  Everything a buffer holds beside the operands is NaN (attn_pack), everything the output buffer holds
    beside the [Lq, heads * hd] block of each batch a sentinel: gap columns, and rows past Lq / Lk inside the allocation.
      plain    q [nb, Lq, E], k and v [nb, Lk, E], contiguous
      wide     the same three, each inside wider rows (ld = E + 8 | E + 4 | E + 12, at column 4 | 0 | 8) with 2 | 2 | 1 rows past the end
      qkv      packed [nb, Lk + 1, 3 E]: q = f, k = f[E:], v = f[2E:], ld 3 E (roi_heads._attend); the queries are the first Lq rows
      kv       q [nb, Lq, E]; k = f, v = f[E:] of [nb, Lk, 2 E] (the matcher decoder's cross attention)
      swapped  packed [outer, Lk, inner, 3 E]: sequences run over dim 1, batched over (outer, inner) with different strides and no
               transpose (the DeepSolo decoder's inter-instance attention); the output likewise
    The output has rows of E + 4 floats (E + 1 with odd_out) and one row past Lq per batch."""
    E, nb = heads * hd, outer * inner
    if view in ("plain", "wide"):
        ld, col, extra = ((E, E, E), (0, 0, 0), (0, 0, 0)) if view == "plain" else ((E + 8, E + 4, E + 12), (4, 0, 8), (2, 2, 1))
        rows = (Lq + extra[0], Lk + extra[1], Lk + extra[2])
        sizes = {n: nb * r * l for n, r, l in zip("qkv", rows, ld)}
        where = {n: (n, c) for n, c in zip("qkv", col)}
        st = [x for r, l in zip(rows, ld) for x in (inner * r * l, r * l, l)]
    elif view == "kv":
        sizes = {"q": nb * Lq * E, "f": nb * Lk * 2 * E}
        where = {"q": ("q", 0), "k": ("f", 0), "v": ("f", E)}
        st = [inner * Lq * E, Lq * E, E] + [inner * Lk * 2 * E, Lk * 2 * E, 2 * E] * 2
    elif view == "qkv":
        assert Lq <= Lk
        ld, R = 3 * E, Lk + 1
        sizes = {"f": nb * R * ld}
        where = {"q": ("f", 0), "k": ("f", E), "v": ("f", 2 * E)}
        st = [inner * R * ld, R * ld, ld] * 3
    else:
        assert view == "swapped" and Lq <= Lk
        ld = 3 * E
        sizes = {"f": outer * Lk * inner * ld}
        where = {"q": ("f", 0), "k": ("f", E), "v": ("f", 2 * E)}
        st = [Lk * inner * ld, ld, inner * ld] * 3
    ldo, Ro = E + (1 if odd_out else 4), Lq + 1
    st += [Ro * inner * ldo, ldo, inner * ldo] if view == "swapped" else [inner * Ro * ldo, Ro * ldo, ldo]
    return {"sizes": sizes, "where": where, "strides": st, "out_size": nb * Ro * ldo}


def attn_pack(lay, q, k, v, outer, inner):
    """The layout's buffers {name: flat float32}, NaN outside the operands."""
    bufs = {n: torch.full((s,), float("nan")) for n, s in lay["sizes"].items()}
    for i, (n, x) in enumerate((("q", q), ("k", k), ("v", v))):
        name, off = lay["where"][n]
        st = lay["strides"][3 * i:3 * i + 3]
        _, heads, L, hd = x.shape
        bufs[name][attn_index(off, st[0], st[1], st[2], outer, inner, heads, hd, L).reshape(-1)] = x.reshape(-1)
    return bufs


class AttnCase:
    """One call of the GPU file: `form` is the kernel the shape is meant to reach (csrc/attn.hip, gom_mha_core_f32)."""

    def __init__(self, form, hd, Lq, Lk, view, heads=2, outer=2, inner=1, odd_out=False, kinds=ATTN_KINDS):
        if view == "swapped":                                             # the decoder's view: batch = outer x inner = 2 x 3
            outer, inner = 2, 3
        self.form, self.hd, self.Lq, self.Lk, self.view, self.heads = form, hd, Lq, Lk, view, heads
        self.outer, self.inner, self.odd_out, self.kinds = outer, inner, odd_out, kinds
        self.id = "%s-%dx%d-%s%s%s" % (form, Lq, Lk, view, "-odd" if odd_out else "", "-b%d" % outer if outer != 2 else "")

    def inputs(self, kind):
        seed = 1000 * ATTN_KINDS.index(kind) + 7 * self.Lq + 13 * self.Lk + self.hd + len(self.view)
        return attn_inputs(kind, self.outer * self.inner, self.heads, self.hd, self.Lq, self.Lk, seed)

    def layout(self):
        return attn_layout(self.view, self.outer, self.inner, self.heads, self.hd, self.Lq, self.Lk, self.odd_out)


def _attn_cases():
    """Per form, the smallest shapes on either side of every limit of gom_mha_core_f32's choice (launch<HD, QT>'s LDS formula
    4 (QT HD + 64 (HD + 4) + QT Lkp) <= 160 KiB, Lkp = Lk rounded up to 64: <32,32> to Lk 1152, <32,8> to 4800, <128,32> to 832,
    <128,8> to 3904; the row-per-lane kernel to Lq 512 and Lk 512, its 64 KiB attribute call from Lk 257), on the tile edges
    63 / 64 / 65, and on every view of attn_layout at least once per form."""
    C = AttnCase
    rows = [C("rows32", 32, 1, 1, "swapped"), C("rows32", 32, 25, 25, "qkv"), C("rows32", 32, 25, 25, "swapped"),
            C("rows32", 32, 63, 5, "kv"), C("rows32", 32, 64, 64, "wide"), C("rows32", 32, 65, 65, "swapped"),
            C("rows32", 32, 512, 7, "plain"), C("rows32", 32, 7, 256, "wide"), C("rows32", 32, 7, 257, "qkv"),
            C("rows32", 32, 3, 512, "kv")]
    t3232 = [C("tile32x32", 32, 513, 5, "kv"), C("tile32x32", 32, 3, 513, "wide"), C("tile32x32", 32, 33, 1152, "qkv"),
             C("tile32x32", 32, 25, 25, "plain", odd_out=True), C("tile32x32", 32, 25, 25, "swapped", odd_out=True)]
    t328 = [C("tile32x8", 32, 9, 1153, "wide"), C("tile32x8", 32, 9, 1153, "swapped"), C("tile32x8", 32, 3, 4800, "kv"),
            C("tile32x8", 32, 3, 4800, "qkv")]
    tiny = [C("tiny128", 128, 1, 1, "swapped", heads=8), C("tiny128", 128, 9, 9, "qkv", heads=8),
            C("tiny128", 128, 53, 53, "swapped", heads=8), C("tiny128", 128, 5, 63, "kv", heads=8),
            C("tiny128", 128, 5, 64, "wide", heads=8), C("tiny128", 128, 70, 64, "plain", heads=8),
            C("tiny128", 128, 64, 64, "plain", heads=8, outer=128, kinds=("randn", "edge"))]          # 65536 waves: the last tiny
    t12832 = [C("tile128x32", 128, 5, 65, "kv"), C("tile128x32", 128, 33, 128, "qkv"), C("tile128x32", 128, 31, 129, "swapped"),
              C("tile128x32", 128, 3, 832, "wide"),
              C("tile128x32", 128, 64, 64, "plain", heads=8, outer=129, kinds=("randn", "edge"))]    # 66048 waves > 65536
    t1288 = [C("tile128x8", 128, 9, 833, "wide"), C("tile128x8", 128, 9, 833, "swapped"), C("tile128x8", 128, 3, 3904, "kv"),
             C("tile128x8", 128, 3, 3904, "qkv")]
    return rows + t3232 + t328 + tiny + t12832 + t1288


ATTN_CASES = _attn_cases()
# gom_mha_core_segments_f32: (Lq, Lk) of the ragged call's segments; an empty query range and an empty key range among them
ATTN_SEGMENTS = [(14, 14), (1, 10), (71, 103), (33, 33), (0, 5), (4, 0)]
ATTN_SEGMENT_KINDS = ("randn", "overflow", "edge")


def attn_segment_inputs(kind, s):
    """Segment s of ATTN_SEGMENTS: attn_inputs for one batch, 2 heads x 128."""
    Lq, Lk = ATTN_SEGMENTS[s]
    return attn_inputs(kind, 1, 2, 128, Lq, Lk, 500 + 10 * s + ATTN_KINDS.index(kind))
