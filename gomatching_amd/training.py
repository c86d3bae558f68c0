"""Training of the association head on MI355X (gom_lstmatcher.py:213-266, lstmatcher.py:237-330,384-475).

Two halves.  Host: the integer ground-truth logic that turns proposals + annotated instances into association targets and the
Hungarian matching of `loss_res` (numpy + the library's LSA).  Device (second half of this file): the training forward of
the trainable head with saved activations, its backward on HIP kernels, the loss dict of `GoMatching.forward`, and the
gradient all-reduce.  Losses AND gradients are pinned against the reference's own (`tests/golden/train_*.npz`), at
`MODEL.ASSO_HEAD.DROPOUT 0`; with dropout the forward follows the reference's sites and torch's semantics on a mask stream of its
own (`DropoutState`, csrc/dropout.hip; INTEGRATION.md "Dropout"), pinned by a float64 restatement (tests/dropout_statement.py).

`association_targets` mirrors `LSTMatcher._get_asso_gt` (lstmatcher.py:388-433; identical in shared_ffn_crsattn.py) on
numpy arrays: it is bookkeeping over at most a few hundred boxes per clip and stays on the host, as the id logic of the
tracker does.
"""
import numpy as np


def normalised_boxes_and_times(boxes_per_frame, image_sizes):
    """`_get_boxes_time` (lstmatcher.py:478-496): boxes [n_t,4] px per frame -> ([N,4] float32 in image units, [N] frame index)."""
    out, times = [], []
    for t, (b, (h, w)) in enumerate(zip(boxes_per_frame, image_sizes)):
        b = np.array(b, dtype=np.float32).reshape(-1, 4).copy()
        b[:, [0, 2]] /= np.float32(w)
        b[:, [1, 3]] /= np.float32(h)
        out.append(b)
        times.append(np.full((b.shape[0],), t, np.int64))
    return (np.concatenate(out) if out else np.zeros((0, 4), np.float32)), \
        (np.concatenate(times) if times else np.zeros((0,), np.int64))


def pairwise_iou(a, b):
    """detectron2.structures.pairwise_iou in float32: inter / (area_a + area_b - inter), 0 where the boxes do not overlap."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = np.clip(np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area_a[:, None] + area_b[None, :] - inter)
    return np.where(inter > 0, iou, np.float32(0)).astype(np.float32)


def association_targets(pred_box, pred_time, target_box, target_time, target_inst_id, n_t):
    """(gt [K,T] int64, match_cues [N] int64).  gt[k, t] = index (within frame t) of the proposal overlapping track k's
    annotated box in frame t, or n_t[t] ("background") when the track is absent or unmatched there; match_cues[j] = the
    track proposal j belongs to, or -1.  Tracks are the sorted distinct positive instance ids."""
    pred_time, target_time = np.asarray(pred_time), np.asarray(target_time)
    target_inst_id = np.asarray(target_inst_id, np.int64)
    ious = pairwise_iou(pred_box, target_box)
    ious[pred_time[:, None] != target_time[None, :]] = -1.0
    inst_ids = np.unique(target_inst_id[target_inst_id > 0])
    K, N, T = len(inst_ids), len(pred_time), len(n_t)
    cues = np.full((N,), -1, np.int64)
    gt = np.zeros((K, T), np.int64)
    starts = np.concatenate([[0], np.cumsum(n_t)]).astype(np.int64)
    for k, inst in enumerate(inst_ids):
        sel = target_inst_id == inst
        for t in range(T):
            block = ious[starts[t]:starts[t + 1]][:, sel]
            if block.size == 0:
                gt[k, t] = n_t[t]
                continue
            val, ind = block.max(axis=0), block.argmax(axis=0)      # per annotated box of the track: its best proposal
            hit = ind[val > 0.0]
            if len(hit) > 1:
                raise ValueError("track %d has %d overlapping proposals' maxima in frame %d (the reference asserts <= 1)"
                                 % (int(inst), len(hit), t))
            if len(hit) == 1:
                gt[k, t] = int(hit[0])
                cues[starts[t] + int(hit[0])] = k
            else:
                gt[k, t] = n_t[t]
    return gt, cues


def point_matching(re_logits, pred_ctrl_points, target_ctrl_points, focal_alpha=0.25, focal_gamma=2.0, class_weight=1.0,
                   coord_weight=1.0):
    """`CtrlPointHungarianMatcher4GM.forward` (third_party/adet/modeling/model/matcher.py:175-198) for ONE image on numpy
    arrays: re_logits [nq, P, 1] (rescoring head), pred_ctrl_points [nq, P, 2], target_ctrl_points [g, P, 2] (normalised) ->
    (query indices [min(nq,g)], target indices) of the minimum-cost assignment, solved by the library's host LSA
    (`gom_linear_sum_assignment`, SciPy's tie-breaking)."""
    from . import ops
    x = np.asarray(re_logits, np.float32)
    prob = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    neg = (1 - focal_alpha) * (prob ** focal_gamma) * (-np.log(1 - prob + np.float32(1e-8)))
    pos = focal_alpha * ((1 - prob) ** focal_gamma) * (-np.log(prob + np.float32(1e-8)))
    cost_class = (pos[..., 0] - neg[..., 0]).mean(-1, keepdims=True)                    # [nq, 1]
    a = np.asarray(pred_ctrl_points, np.float32).reshape(x.shape[0], -1)
    b = np.asarray(target_ctrl_points, np.float32).reshape(-1, a.shape[1])
    cost_pts = np.abs(a[:, None, :] - b[None, :, :]).sum(-1)                             # torch.cdist(p=1)
    cost = class_weight * cost_class + coord_weight * cost_pts
    return ops.linear_sum_assignment(cost.astype(np.float64))


# =====================================================================================================================
# Device side: the training forward / backward of the trainable head on HIP kernels.
#
# Only `roi_heads` trains in the reference (gomatching/modeling/freeze_layers.py:20-37; train_net.py:111-131): FCHead4Query,
# the matcher transformer(s) and the rescoring head.  Every contraction of the forward AND of the backward (dgrad = dY W,
# wgrad = dY^T X, bias grad = dY^T 1) runs on the library's exact-fp32 MFMA GEMM (`gom_gemm_f32` / its split-K form) with
# transposed operands made by `gom_transpose_f32`; attention is the same GEMM per head around `gom_softmax_rows_scaled_f32`
# and its backward kernel; MODEL.ASSO_HEAD.DROPOUT is applied at the reference's sites by the kernels of csrc/dropout.hip on
# a counter-based mask stream (`DropoutState`: the reference's distribution, a stream of our own); the losses are
# `gom_asso_ce_f32` / `gom_sigmoid_focal_f32` (csrc/train.hip).  torch supplies device memory, the autograd tape that strings the kernels together, and the glue around them (concatenation, zero-padded
# copies, the arithmetic on the 0-d loss values).
# Pinned by the reference's own losses AND gradients (tests/golden/train_asso_*.npz, train_res_ic15.npz;
# tests/test_training_gpu.py).
# =====================================================================================================================
def _torch():
    import torch
    return torch


class DropoutState:
    """Where the training forward is in the dropout mask stream ("Dropout"; csrc/dropout.hip).  The mask of a
    dropout application is a pure function of (seed, site, iteration, rank) and the logical element index: `site` counts the
    applications of one `forward_losses` call in call order, from 0; `iteration` is the trainer's; `rank` is
    torch.distributed's (0 in a single process).  Nothing is stored: the backward regenerates each mask from the tuple that
    the forward kept, a resumed run (same seed, same iteration) reproduces an uninterrupted one, ranks draw different masks."""

    def __init__(self, p, seed, iteration=0, rank=0):
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError("DropoutState: p = %r is not in [0, 1)" % (p,))
        self.p, self.seed, self.rank = p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank)
        self.begin_forward(iteration)

    def begin_forward(self, iteration):
        """Start the sites of a forward at 0, in iteration `iteration`."""
        self.iteration, self.site = int(iteration), 0

    def next_site(self):
        site = self.site
        self.site += 1
        return site

    def next_stream(self):
        """(p, seed, site, iteration, rank) of the next dropout application: what `ops.dropout` and its kin take."""
        return (self.p, self.seed, self.next_site(), self.iteration, self.rank)

    @property
    def active(self):
        return self.p > 0.0


def _active(dropout):
    return dropout if (dropout is not None and dropout.active) else None


def new_dropout_seed():
    """A seed for a run whose config gives none (SEED < 0 or absent): 63 bits from the operating system, drawn once."""
    import os
    return int.from_bytes(os.urandom(8), "little") >> 1


def distributed_rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _pad4(n):
    return (n + 3) // 4 * 4


def _transpose_padded(x):
    """x [R, C] (row-strided) -> x^T as [C, pad4(R)] with zero columns beyond R (the GEMM wants K % 4 == 0)."""
    torch = _torch()
    from . import ops
    R, C = x.shape
    out = torch.zeros((C, _pad4(R)), dtype=torch.float32, device=x.device)
    if R and C:
        ops.transpose_into(x, out)
    return out


def _make_functions():
    """autograd Functions are created lazily so that importing this module never needs torch or the GPU library."""
    torch = _torch()
    from . import ops

    def linear_grads(ctx, x, w, dy, extra):
        """dgrad / wgrad / bias grad of y = x W^T + b for the incoming (activation-corrected) dy; `extra` Nones follow."""
        M, N = dy.shape
        dx = dw = db = None
        if M == 0:
            return (torch.zeros_like(x), torch.zeros_like(w), (torch.zeros((N,), device=w.device) if ctx.has_b else None)) + extra
        if ctx.needs_input_grad[0]:
            dyp = dy
            if N % 4:                                                                             # the GEMM wants K % 4 == 0
                dyp = torch.zeros((M, _pad4(N)), dtype=torch.float32, device=dy.device)
                dyp[:, :N] = dy
            dx = ops.gemm(dyp, _transpose_padded(w))                                              # dY W   (K = pad4(N))
        dyT = _transpose_padded(dy)                                                               # [N, Mp]
        if ctx.needs_input_grad[1]:
            dw = ops.gemm(dyT, _transpose_padded(x))                                              # dY^T X (K = Mp)
        if ctx.has_b and ctx.needs_input_grad[2]:
            ones = torch.zeros((1, dyT.shape[1]), dtype=torch.float32, device=dy.device)
            ones[:, :M] = 1.0
            db = ops.gemm(dyT, ones).view(N)
        return (dx, dw, db) + extra

    class Linear(torch.autograd.Function):
        """y = act(x W^T + b); x [M, K] row-strided, W [N, K]."""

        @staticmethod
        def forward(ctx, x, w, b, relu):
            y = ops.gemm(x, w, bias=b, relu=bool(relu))
            ctx.save_for_backward(x, w, y if relu else None)
            ctx.relu, ctx.has_b = bool(relu), b is not None
            return y

        @staticmethod
        def backward(ctx, dy):
            x, w, y = ctx.saved_tensors
            dy = dy.contiguous()
            if ctx.relu:
                dy = ops.relu_backward(dy, y)
            return linear_grads(ctx, x, w, dy, (None,))

    class LinearReluDrop(torch.autograd.Function):
        """y = dropout(relu(x W^T + b)) (the FFN's `dropout(activation(linear1(.)))`): the dropout runs in place on the GEMM's
        output, and that DROPPED y is all the backward needs -- it is positive exactly where the unit was active and kept, so
        d = dy * scale * (y > 0) regenerates no mask."""

        @staticmethod
        def forward(ctx, x, w, b, stream):
            y = ops.gemm(x, w, bias=b, relu=True)
            if y.numel():
                ops.dropout(y, stream, out=y)
            ctx.save_for_backward(x, w, y)
            ctx.has_b, ctx.drop_scale = b is not None, ops.dropout_args(*stream)[5]
            return y

        @staticmethod
        def backward(ctx, dy):
            x, w, y = ctx.saved_tensors
            dy = ops.relu_backward_scaled(dy.contiguous(), y, ctx.drop_scale)
            return linear_grads(ctx, x, w, dy, (None,))

    class DropAdd(torch.autograd.Function):
        """r + dropout(x) in one pass (`src + dropoutN(x)`; r = None: dropout(x) alone); the backward hands dy to r and
        mask * scale * dy, the mask regenerated from the stream tuple, to x."""

        @staticmethod
        def forward(ctx, r, x, stream):
            ctx.stream = stream
            x = x.contiguous()
            r = None if r is None else r.contiguous()
            if x.numel() == 0:
                return x.clone() if r is None else r.clone()
            return ops.dropout(x, stream, residual=r)

        @staticmethod
        def backward(ctx, g):
            g = g.contiguous()
            return (g if ctx.needs_input_grad[0] else None), (ops.dropout(g, ctx.stream) if g.numel() else g), None

    class Attention(torch.autograd.Function):
        """softmax(q k^T / sqrt(hd)) v per head for ONE sequence pair: q [Lq, E], k, v [Lk, E] (nn.MultiheadAttention core,
        transformer.py:208,287 of the reference's matcher), heads laid side by side in E."""

        @staticmethod
        def forward(ctx, q, k, v, heads):
            Lq, E = q.shape
            Lk = k.shape[0]
            hd = E // heads
            Lkp = _pad4(Lk)
            out = torch.zeros((Lq, E), dtype=torch.float32, device=q.device)
            P = torch.zeros((heads, Lq, Lkp), dtype=torch.float32, device=q.device)
            scale = 1.0 / math.sqrt(hd)
            if Lq and Lk:
                for h in range(heads):
                    c = slice(h * hd, (h + 1) * hd)
                    ops.gemm(q[:, c], k[:, c], out=P[h][:, :Lk])                                       # q_h k_h^T
                    ops.softmax_rows_scaled_(P[h], Lk, scale)
                    ops.gemm(P[h], _transpose_padded(v[:, c]), out=out[:, c])                         # P v_h   (K = Lkp)
            ctx.save_for_backward(q, k, v, P)
            ctx.heads, ctx.scale = heads, scale
            return out

        @staticmethod
        def backward(ctx, do):
            q, k, v, P = ctx.saved_tensors
            heads, scale = ctx.heads, ctx.scale
            Lq, E = q.shape
            Lk = k.shape[0]
            hd = E // heads
            dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
            if Lq == 0 or Lk == 0:
                return dq, dk, dv, None
            do = do.contiguous()
            for h in range(heads):
                c = slice(h * hd, (h + 1) * hd)
                Ph = P[h]
                ops.gemm(_transpose_padded(Ph[:, :Lk]), _transpose_padded(do[:, c]), out=dv[:, c])    # P^T dO  (K = Lqp)
                dP = torch.zeros_like(Ph)
                ops.gemm(do[:, c], v[:, c], out=dP[:, :Lk])                                           # dO v_h^T
                dS = ops.softmax_rows_backward(Ph, dP, Lk, scale)
                ops.gemm(dS, _transpose_padded(k[:, c]), out=dq[:, c])                                # dS k_h   (K = Lkp)
                ops.gemm(_transpose_padded(dS[:, :Lk]), _transpose_padded(q[:, c]), out=dk[:, c])     # dS^T q_h (K = Lqp)
            return dq, dk, dv, None

    class AttentionDrop(torch.autograd.Function):
        """`Attention` with dropout on the weights after the softmax (inside nn.MultiheadAttention): out = P~ v with
        P~ = mask * scale * P over the logical [heads, Lq, Lk] tensor -- ONE stream for all heads, each head its own slice of
        it.  The softmax of all heads is one launch that leaves both P (saved: the softmax backward needs the undropped
        weights) and P~; the backward regenerates P~ from P and applies the mask to the incoming dP~ inside its kernel."""

        @staticmethod
        def forward(ctx, q, k, v, heads, stream):
            Lq, E = q.shape
            Lk = k.shape[0]
            hd = E // heads
            Lkp = _pad4(Lk)
            out = torch.zeros((Lq, E), dtype=torch.float32, device=q.device)
            P = torch.zeros((heads, Lq, Lkp), dtype=torch.float32, device=q.device)
            scale = 1.0 / math.sqrt(hd)
            if Lq and Lk:
                for h in range(heads):
                    c = slice(h * hd, (h + 1) * hd)
                    ops.gemm(q[:, c], k[:, c], out=P[h][:, :Lk])                                       # q_h k_h^T
                Pd = ops.softmax_dropout_rows_(P.view(heads * Lq, Lkp), Lk, scale, stream).view(heads, Lq, Lkp)
                for h in range(heads):
                    c = slice(h * hd, (h + 1) * hd)
                    ops.gemm(Pd[h], _transpose_padded(v[:, c]), out=out[:, c])                        # P~ v_h  (K = Lkp)
            ctx.save_for_backward(q, k, v, P)
            ctx.heads, ctx.scale, ctx.stream = heads, scale, stream
            return out

        @staticmethod
        def backward(ctx, do):
            q, k, v, P = ctx.saved_tensors
            heads, scale = ctx.heads, ctx.scale
            Lq, E = q.shape
            Lk = k.shape[0]
            hd = E // heads
            Lkp = _pad4(Lk)
            dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
            if Lq == 0 or Lk == 0:
                return dq, dk, dv, None, None
            do = do.contiguous()
            P2 = P.view(heads * Lq, Lkp)
            Pd = torch.zeros_like(P)
            ops.dropout(P2[:, :Lk], ctx.stream, out=Pd.view(heads * Lq, Lkp)[:, :Lk])                 # P~ again, from P
            dPd = torch.zeros_like(P)
            for h in range(heads):
                c = slice(h * hd, (h + 1) * hd)
                ops.gemm(_transpose_padded(Pd[h][:, :Lk]), _transpose_padded(do[:, c]), out=dv[:, c])  # P~^T dO (K = Lqp)
                ops.gemm(do[:, c], v[:, c], out=dPd[h][:, :Lk])                                       # dO v_h^T
            dS = ops.softmax_dropout_rows_backward(P2, dPd.view(heads * Lq, Lkp), Lk, scale, ctx.stream).view(heads, Lq, Lkp)
            for h in range(heads):
                c = slice(h * hd, (h + 1) * hd)
                ops.gemm(dS[h], _transpose_padded(k[:, c]), out=dq[:, c])                             # dS k_h   (K = Lkp)
                ops.gemm(_transpose_padded(dS[h][:, :Lk]), _transpose_padded(q[:, c]), out=dk[:, c])  # dS^T q_h (K = Lqp)
            return dq, dk, dv, None, None

    class Add(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            return ops.add(a.contiguous(), b.contiguous())

        @staticmethod
        def backward(ctx, g):
            return g, g

    class AssoCE(torch.autograd.Function):
        """sum over (row, frame) of the per-frame cross entropy with background (detr_asso_loss, lstmatcher.py:436-475)."""

        @staticmethod
        def forward(ctx, logits, offs, gt):
            loss, _ = ops.asso_ce(logits, offs, gt)
            ctx.save_for_backward(logits, offs, gt)
            # the sum of a handful of values: one GEMM against a ones row (K padded to 4)
            flat = torch.zeros((1, _pad4(loss.numel())), dtype=torch.float32, device=logits.device)
            flat[0, :loss.numel()] = loss.view(-1)
            return ops.gemm(flat, torch.ones_like(flat)).view(())

        @staticmethod
        def backward(ctx, g):
            logits, offs, gt = ctx.saved_tensors
            _, dl = ops.asso_ce(logits, offs, gt, want_loss=False, grad_scale=g.reshape(1).contiguous().float())
            return dl, None, None

    class FocalSum(torch.autograd.Function):
        """sum of the sigmoid focal loss over every element (loss_res, lstmatcher.py:237-268)."""

        @staticmethod
        def forward(ctx, x, target, alpha, gamma):
            loss, dx = ops.sigmoid_focal(x, target, alpha, gamma)
            ctx.save_for_backward(dx)
            flat = torch.zeros((1, _pad4(loss.numel())), dtype=torch.float32, device=x.device)
            flat[0, :loss.numel()] = loss.view(-1)
            return ops.gemm(flat, torch.ones_like(flat)).view(())

        @staticmethod
        def backward(ctx, g):
            (dx,) = ctx.saved_tensors
            return dx * g, None, None, None

    return {"Linear": Linear, "Attention": Attention, "Add": Add, "AssoCE": AssoCE, "FocalSum": FocalSum,
            "LinearReluDrop": LinearReluDrop, "DropAdd": DropAdd, "AttentionDrop": AttentionDrop}


_FN = None


def _fn():
    global _FN
    if _FN is None:
        _FN = _make_functions()
    return _FN


import math  # noqa: E402


def _linear(x, params, name, relu=False):
    return _fn()["Linear"].apply(x, params[name + ".weight"], params.get(name + ".bias"), relu)


def _mha(q_in, kv_in, params, name, heads, dropout=None):
    """nn.MultiheadAttention(q, k = v = kv_in) with packed in_proj (transformer.py:208,287).  `dropout`: a DropoutState that
    drops the attention weights after the softmax (one site); None or p = 0: the eval-mode path, launch for launch."""
    E = q_in.shape[1]
    w, b = params[name + ".in_proj_weight"], params[name + ".in_proj_bias"]
    L = _fn()["Linear"]
    q = L.apply(q_in, w[:E], b[:E], False)
    kv = L.apply(kv_in, w[E:], b[E:], False)
    dropout = _active(dropout)
    if dropout is None:
        a = _fn()["Attention"].apply(q, kv[:, :E], kv[:, E:], heads)
    else:
        a = _fn()["AttentionDrop"].apply(q, kv[:, :E], kv[:, E:], heads, dropout.next_stream())
    return L.apply(a, params[name + ".out_proj.weight"], params[name + ".out_proj.bias"], False)


def _ffn(x, params, p, dropout):
    """linear2(dropout(relu(linear1(x)))) (transformer.py:203, 283); without dropout: the two Linear launches as before."""
    if dropout is None:
        h = _linear(x, params, p + "linear1", relu=True)
    else:
        h = _fn()["LinearReluDrop"].apply(x, params[p + "linear1.weight"], params.get(p + "linear1.bias"), dropout.next_stream())
    return _linear(h, params, p + "linear2")


def matcher_transformer(params, cfg, reid, short_term, prefix="roi_heads.", dropout=None):
    """Training forward of the matcher (roi_heads/transformer.py:60-96 with norm = Identity, every proposal a query):
    returns (feats [N, F], memory [N, F]).  `dropout`: a DropoutState (MODEL.ASSO_HEAD.DROPOUT in training mode) -- the sites of
    the reference's `forward_post` layers, in call order: per encoder layer the attention weights, `src + dropout1(attn)`, the
    FFN's inner dropout, `src + dropout2(ffn)`; per decoder layer the cross-attention weights, `tgt + dropout2(attn)` and, unless
    the head is SHA_FFN_CRSATTN (`only_dec_crs_attn`), the FFN's inner dropout and `tgt + dropout3(ffn)`.  None or p = 0 takes
    the path without dropout exactly: the same launches, the same bits."""
    A = cfg.MODEL.ASSO_HEAD
    shared = cfg.MODEL.ROI_HEADS.NAME == "SHA_FFN_CRSATTN"
    name = prefix + ("shared_matcher" if shared else ("short_term_matcher" if short_term else "long_term_matcher"))
    dropout = _active(dropout)
    if dropout is None:
        add = _fn()["Add"].apply
    else:
        add = lambda r, x: _fn()["DropAdd"].apply(r, x, dropout.next_stream())
    memory = reid
    n_enc = 0 if shared else A.NUM_ENCODER_LAYERS
    for i in range(n_enc):
        p = "%s.encoder.layers.%d." % (name, i)
        memory = add(memory, _mha(memory, memory, params, p + "self_attn", A.NUM_HEADS, dropout))
        memory = add(memory, _ffn(memory, params, p, dropout))
    tgt = reid
    for i in range(A.NUM_DECODER_LAYERS):
        p = "%s.decoder.layers.%d." % (name, i)
        tgt = add(tgt, _mha(tgt, memory, params, p + "multihead_attn", A.NUM_HEADS, dropout))
        if not shared:
            tgt = add(tgt, _ffn(tgt, params, p, dropout))
    return tgt, memory


def _detr_asso_loss(logits, gt, cues, n_t, neg_unmatched):
    """detr_asso_loss (lstmatcher.py:436-475) on the device: logits [N, N]; gt [K, T] / cues [N] from association_targets."""
    torch = _torch()
    N, T = logits.shape[0], len(n_t)
    tgt = np.full((N, T), -1, np.int32)
    src = np.nonzero(cues >= 0)[0]
    if neg_unmatched:
        tgt[:] = np.asarray(n_t, np.int32)[None, :]
    if len(src):
        tgt[src] = gt[cues[src]].astype(np.int32)
    counted = tgt >= 0
    num = float(((tgt != np.asarray(n_t, np.int32)[None, :]) & counted).sum())
    offs = np.concatenate([[0], np.cumsum(n_t)]).astype(np.int32)
    dev = logits.device
    total = _fn()["AssoCE"].apply(logits.contiguous(), torch.from_numpy(offs).to(dev), torch.from_numpy(tgt).to(dev))
    return total / (num + 1e-4)


def asso_losses(params, cfg, frames, targets, prefix="roi_heads.", dropout=None):
    """`_forward_asso`, training branch (lstmatcher.py:271-330 = shared_ffn_crsattn.py), on the device.
    params: {state-dict key: CUDA tensor (nn.Parameter)}; frames: per frame {"image_size", "proposal_boxes" [n,4] px,
    "objectness_logits" [n], "query_features" [n,25,256]} (CUDA); targets: per frame {"image_size", "gt_boxes" [g,4] px,
    "gt_instance_ids" [g]} (host or device).  Returns {"loss_long_asso", "loss_short_asso"} with autograd history.
    `dropout`: the DropoutState of the matchers (`matcher_transformer`); FCHead4Query and ATTWeightHead have no dropout."""
    torch = _torch()
    A = cfg.MODEL.ASSO_HEAD
    dev = params[prefix + "asso_head.fc1.weight"].device
    keep = [(f["objectness_logits"] > A.ASSO_THRESH).nonzero().flatten() for f in frames]
    boxes = [f["proposal_boxes"][k].detach().cpu().numpy() for f, k in zip(frames, keep)]
    n_t = [int(len(k)) for k in keep]
    sizes = [tuple(f["image_size"]) for f in frames]
    width = int(np.prod(frames[0]["query_features"].shape[1:]))                 # 25 points x 256 channels
    qf = [f["query_features"][k].reshape(len(k), width) for f, k in zip(frames, keep)]
    x = torch.cat(qf).to(dev).float().contiguous()
    for i in range(A.NUM_FC):
        x = _linear(x, params, prefix + "asso_head.fc%d" % (i + 1), relu=True)
    reid = x
    tb = [np.asarray(t["gt_boxes"].cpu() if hasattr(t["gt_boxes"], "cpu") else t["gt_boxes"], np.float32).reshape(-1, 4)
          for t in targets]
    tids = [np.asarray(t["gt_instance_ids"].cpu() if hasattr(t["gt_instance_ids"], "cpu") else t["gt_instance_ids"], np.int64)
            for t in targets]
    zero = reid.sum() * 0.0 if reid.numel() else torch.zeros((), device=dev)
    if sum(len(b) for b in tb) == 0 or max(int(i.max()) for i in tids if len(i)) == 0:
        return {"loss_long_asso": zero, "loss_short_asso": zero}

    def one(lo_f, hi_f, reid_sl, short):
        feats, memory = matcher_transformer(params, cfg, reid_sl, short, prefix, dropout)
        logits = _fn()["Linear"].apply(feats, memory, None, False)                 # ATTWeightHead, 0 layers: q . k^T
        pb, pt = normalised_boxes_and_times(boxes[lo_f:hi_f], sizes[lo_f:hi_f])
        gb, gtime = normalised_boxes_and_times(tb[lo_f:hi_f], [tuple(t["image_size"]) for t in targets[lo_f:hi_f]])
        ids = np.concatenate([i for i in tids[lo_f:hi_f] if len(i)]) if any(len(i) for i in tids[lo_f:hi_f]) else np.zeros((0,), np.int64)
        gt, cues = association_targets(pb, pt, gb, gtime, ids, n_t[lo_f:hi_f])
        return _detr_asso_loss(logits, gt, cues, n_t[lo_f:hi_f], A.NEG_UNMATCHED)

    loss_long = one(0, len(frames), reid, False)
    loss_short, eff = zero, 0
    for c in range(1, len(frames)):
        ids_sl = [i for i in tids[c - 1:c + 1] if len(i)]
        if not ids_sl or max(int(i.max()) for i in ids_sl) == 0:
            continue
        eff += 1
        lo, hi = sum(n_t[:c - 1]), sum(n_t[:c + 1])
        loss_short = loss_short + one(c - 1, c + 1, reid[lo:hi], True)
    loss_short = loss_short / (eff + 1e-4)
    return {"loss_long_asso": A.ASSO_WEIGHT * loss_long, "loss_short_asso": A.ASSO_WEIGHT_LOCAL * loss_short}


def loss_res(params, cfg, query_features, pred_ctrl_points, targets, prefix="roi_heads."):
    """`LSTMatcher.loss_res` (lstmatcher.py:237-268): rescoring head (Linear 256 -> 1 on every point feature) under the sigmoid
    focal loss against the Hungarian-matched queries.  query_features [B,nq,P,256], pred_ctrl_points [B,nq,P,2] (frozen detector,
    CUDA); targets: per image {"labels" [g], "ctrl_points" [g,P,2]}."""
    torch = _torch()
    Lc = cfg.MODEL.TRANSFORMER.LOSS
    B, nq, P, C = query_features.shape
    logits = _linear(query_features.reshape(-1, C).float().contiguous(), params, prefix + "rescoring_head")     # [B*nq*P, 1]
    lg_host = logits.detach().view(B, nq, P, 1).cpu().numpy()
    pts_host = pred_ctrl_points.detach().cpu().numpy()
    onehot = np.zeros((B, nq, P, 1), np.float32)
    num_inst = 0
    for b, t in enumerate(targets):
        tc = np.asarray(t["ctrl_points"].cpu() if hasattr(t["ctrl_points"], "cpu") else t["ctrl_points"], np.float32)
        num_inst += len(tc)
        if len(tc) == 0:
            continue
        src, _ = point_matching(lg_host[b], pts_host[b], tc, Lc.FOCAL_ALPHA, Lc.FOCAL_GAMMA, Lc.POINT_CLASS_WEIGHT,
                                Lc.POINT_COORD_WEIGHT)
        onehot[b, src] = 1.0                                      # one text class: label 0 of NUM_CLASSES = 1
    target = torch.from_numpy(onehot.reshape(-1, 1)).to(logits.device)
    total = _fn()["FocalSum"].apply(logits, target, float(Lc.FOCAL_ALPHA), float(Lc.FOCAL_GAMMA))
    return {"loss_res": total / (P * max(float(num_inst), 1.0))}


def allreduce_gradients(parameters, group=None):
    """Data-parallel training of the head (train_net.py runs under DistributedDataParallel): ONE all-reduce (RCCL over xGMI with
    backend "nccl"; gloo in the CPU test) of all gradients flattened into one bucket, averaged over the ranks.  The head has
    12-33 M parameters (47-131 MB): one bucket is latency-optimal on the point-to-point xGMI ring.
    The bucket is RANK-INVARIANT: every parameter with `requires_grad`, in the order given, zeros where this rank has no
    gradient (a clip without ground-truth ids returns the zero loss, a clip whose short-term matcher had no rows leaves that
    matcher's parameters without one -- on that rank only); the averaged gradient is written back to every parameter that had a
    gradient on AT LEAST ONE rank, as DistributedDataParallel does.  A parameter no rank used keeps `grad = None` (one
    "has a gradient" word per parameter travels at the end of the bucket), so weight decay / momentum treat it exactly as a
    single-process run does.  No rank ever skips the collective."""
    torch = _torch()
    import torch.distributed as dist
    params = [p for p in parameters if p.requires_grad]
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return 0
    if not params:
        return 0                                                 # rank-invariant: `requires_grad` is a property of the model
    has = torch.tensor([0.0 if p.grad is None else 1.0 for p in params], dtype=params[0].dtype, device=params[0].device)
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params] + [has])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    used = flat[-len(params):].cpu() > 0
    flat = flat[:-len(params)]
    flat /= dist.get_world_size(group)
    o = 0
    for p, u in zip(params, used.tolist()):
        n = p.numel()
        if not u:
            pass                                                 # unused on every rank: stays None
        elif p.grad is None:
            p.grad = flat[o:o + n].view_as(p).clone()
        else:
            p.grad.copy_(flat[o:o + n].view_as(p.grad))
        o += n
    return flat.numel()


def detect_for_training(impl, params, batched_inputs, taps=None, whole_batch=False):
    """The no-grad detector part of `forward_losses`: the frozen detector on the HIP inference kernels, the rescoring product,
    and the training proposals (no NMS, kept by the score threshold).  -> {"frames": per frame {"image_size",
    "proposal_boxes", "objectness_logits", "query_features", "keep_rows"}, "sizes": per frame (h, w), "padded_hw",
    "query_features" [B,nq,P,C], "pred_ctrl_points" [B,nq,P,2], "groups": [(hw, frame indices)]}, all in FRAME order.

    Frames of one size (every video clip) are one group: one backbone pass, one `detection_transformer.forward`, today's
    launches.  The frames of a motion clip (`GoMatching._raw_motion`) are padded to one size but differ in their own: they are
    grouped by (OH, OW) in order of first appearance, and each group runs the backbone on its (still padded) frames and the
    transformer with `image_hw` = the group's size, the rescoring product, `argmax_rows` and `detect_post` with that size.
    `keep_idx` of a group indexes the group's flattened query axis; results are scattered back to frame order.  Geometry
    tables built for a motion step are not kept (`DeepSolo._geom_transient`): every clip brings new sizes.
    `taps`: a list that receives, per group, the transformer's tap dict (`DeepSolo.forward(taps=...)`) -- a test's window.

    `whole_batch`: a motion clip runs as ONE padded batch with per-frame valid extents inside the kernels (the reference's own
    form: one batch, per-image masks) -- one backbone pass, one `forward(image_sizes=sizes)`, one rescoring product, one
    `argmax_rows`, one `detect_post` with a size per frame.  `groups` is then the single entry (padded_hw, [0..B-1]); every frame
    keeps its own `image_size`.  A step that is not a motion step issues the launches it issues without the flag."""
    torch = _torch()
    from . import ops
    cfg = impl.cfg
    T = cfg.MODEL.TRANSFORMER
    B, nq, P = len(batched_inputs), T.NUM_QUERIES, T.NUM_POINTS
    tr = impl.detection_transformer
    with torch.no_grad():
        raw, kind = impl._raw_input(batched_inputs)
        x = impl._normalise(raw, kind)
        motion = kind[0] in ("u8motion", "f32motion")
        sizes = [tuple(int(v) for v in s) for s in kind[4]] if motion else [tuple(kind[1])] * B
        whole = bool(whole_batch) and motion
        groups = {}
        for t, hw in enumerate(sizes):
            groups.setdefault(hw, []).append(t)
        groups = [(tuple(int(v) for v in kind[1]), list(range(B)))] if whole else list(groups.items())
        parts = []
        tr._geom_transient = motion
        try:
            for hw, members in groups:
                Bg = len(members)
                xg = x if Bg == B else x.index_select(0, torch.tensor(members, dtype=torch.int64, device=x.device))
                feats = impl.backbone.forward(xg)
                feats = [feats[k] for k in impl.feature_names]
                kw = {}
                if whole:
                    kw["image_sizes"] = sizes
                elif motion:
                    kw["image_hw"] = hw
                if taps is not None:
                    taps.append({})
                    kw["taps"] = taps[-1]
                out = tr.forward(feats, **kw)
                re = None
                if impl.with_rescore:
                    re = ops.gemm(out["query_features"], params["roi_heads.rescoring_head.weight"].detach(),
                                  bias=params["roi_heads.rescoring_head.bias"].detach())
                recs = ops.argmax_rows(out["pred_text_logits"])
                # training proposals: no NMS (gom_lstmatcher.py:231-258 builds them straight from `detection`), kept by the score threshold
                if whole:
                    det = ops.detect_post(out["pred_logits"], re, out["pred_ctrl_points"], out["pred_bd_points"], recs, Bg, nq, P,
                                          None, None, impl.test_score_threshold, 2.0, -1.0,
                                          frame_sizes=torch.tensor(sizes, dtype=torch.float32).to(x.device))
                else:
                    det = ops.detect_post(out["pred_logits"], re, out["pred_ctrl_points"], out["pred_bd_points"], recs, Bg, nq, P,
                                          hw[0], hw[1], impl.test_score_threshold, 2.0, -1.0)
                parts.append((out, det))
        finally:
            tr._geom_transient = False
        torch.cuda.current_stream().synchronize()
        if ops.GEMM_MODE == "f16x3":
            # the range flag of the f16x3 kernels (`detect_launch` reads and clears it per inference step): an activation beyond
            # fp16's range during a TRAINING forward must not feed the losses silently, nor stay set for the next inference step
            ops.check_range_flag(x.device)
        frames = [None] * B
        for (hw, members), (out, det) in zip(groups, parts):
            Bg = len(members)
            qf_g = out["query_features"].view(Bg * nq, P, -1)
            counts = det["count"].cpu().numpy()
            keep = det["keep_idx"].cpu().numpy()
            for j, t in enumerate(members):
                n = int(counts[j])
                rows = torch.from_numpy(keep[j, :n].astype(np.int64)).to(qf_g.device)   # rows of the GROUP's flattened [Bg*nq] query axis
                frames[t] = {"image_size": sizes[t], "proposal_boxes": det["boxes"][j, :n], "objectness_logits": det["scores"][j, :n],
                             "query_features": qf_g.index_select(0, rows), "keep_rows": rows - j * nq}
        if len(groups) == 1:
            out = parts[0][0]
            qf = out["query_features"].view(B, nq, P, -1)
            ctrl = out["pred_ctrl_points"].view(B, nq, P, 2)
        else:
            order = torch.tensor([t for _, members in groups for t in members], dtype=torch.int64, device=x.device)
            qf = torch.empty((B, nq, P, parts[0][0]["query_features"].shape[-1]), dtype=torch.float32, device=x.device)
            ctrl = torch.empty((B, nq, P, 2), dtype=torch.float32, device=x.device)
            qf.index_copy_(0, order, torch.cat([o["query_features"].view(-1, nq, P, qf.shape[-1]) for o, _ in parts]))
            ctrl.index_copy_(0, order, torch.cat([o["pred_ctrl_points"].view(-1, nq, P, 2) for o, _ in parts]))
    return {"frames": frames, "sizes": sizes, "padded_hw": tuple(kind[1]), "query_features": qf, "pred_ctrl_points": ctrl,
            "groups": groups}


def forward_losses(model, batched_inputs, motion_whole_batch=None):
    """`GoMatching.forward` in training (gom_lstmatcher.py:213-266) for the META_ARCH wrapper (`compat/d2_register.py`): the
    frozen detector runs on the HIP inference kernels without a tape (`detect_for_training`); the losses of the trainable head
    carry autograd history onto `model.roi_heads`' parameters.  batched_inputs: the reference's list of {"image" [3,H,W],
    "instances": ground truth with gt_boxes / gt_instance_ids / (for loss_res) normalised ctrl points under `polyline` or
    `ctrl_points`}; in a motion clip every frame keeps its own `image_size` (the reference's per-image `image_sizes`).
    `motion_whole_batch`: `detect_for_training(whole_batch=...)`; None reads `model.motion_whole_batch` (False when absent)."""
    torch = _torch()
    if hasattr(model, "impl"):                                   # the META_ARCH wrapper: live nn.Parameters
        impl = model.impl(for_training=True)
        params = {k: p for k, p in model.named_parameters() if k.startswith("roi_heads.")}
    else:                                                        # the HIP model itself: its own trainable copies
        impl = model
        params = model.trainable_parameters()
    cfg = model.cfg
    P = cfg.MODEL.TRANSFORMER.NUM_POINTS
    if motion_whole_batch is None:
        motion_whole_batch = getattr(model, "motion_whole_batch", False)
    det = detect_for_training(impl, params, batched_inputs, whole_batch=motion_whole_batch)
    frames, targets, res_targets = [], [], []
    for b, inp in enumerate(batched_inputs):
        hw = det["sizes"][b]
        frames.append({k: v for k, v in det["frames"][b].items() if k != "keep_rows"})
        gt = inp["instances"]
        get = (lambda k: gt.get(k)) if hasattr(gt, "get") else (lambda k: gt[k])
        boxes = get("gt_boxes")
        boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
        targets.append({"image_size": hw, "gt_boxes": boxes, "gt_instance_ids": get("gt_instance_ids")})
        if impl.with_rescore:
            pts = get("ctrl_points") if (hasattr(gt, "has") and gt.has("ctrl_points")) or (isinstance(gt, dict) and "ctrl_points" in gt) \
                else get("polyline")
            pts = torch.as_tensor(pts).float().reshape(-1, P, 2) / torch.tensor([hw[1], hw[0]], dtype=torch.float32)
            res_targets.append({"labels": np.zeros((pts.shape[0],), np.int64), "ctrl_points": pts})
    dropout = _active(getattr(model, "dropout_state", None))    # Trainer / the META_ARCH wrapper attach it when DROPOUT > 0
    if dropout is not None:
        dropout.begin_forward(dropout.iteration)                # sites count from 0 in every forward
    losses = asso_losses(params, cfg, frames, targets, dropout=dropout)
    if impl.with_rescore:
        losses.update(loss_res(params, cfg, det["query_features"], det["pred_ctrl_points"], res_targets))
    return losses
