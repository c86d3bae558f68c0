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
