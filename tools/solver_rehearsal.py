"""CPU rehearsal of tests/test_solver_gpu.py::test_trainer_lowers_the_loss_on_one_clip: the same mini config, weights, clip
and ground truth, the detector and the head's training losses from the CPU restatements (oracle/gom_oracle.py,
oracle/train_oracle.py), the update from torch.optim.AdamW + clip_grad_norm_ -- to choose BASE_LR and the number of steps so
that the loss decreases with room to spare before the GPU test asserts it.

    python tools/solver_rehearsal.py [BASE_LR] [STEPS]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import mini_cfg  # noqa: E402
from oracle import gom_oracle as O, train_oracle  # noqa: E402
from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip  # noqa: E402
from gomatching_amd.weights import synth_state_dict  # noqa: E402


def main():
    base_lr = float(sys.argv[1]) if len(sys.argv) > 1 else 2e-4
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    torch.manual_seed(0)
    cfg = mini_cfg("icdar15")
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    for leaf in ("weight", "bias"):                              # train_net.py:97-101: the rescoring head starts as the classifier
        sd["roi_heads.rescoring_head." + leaf] = sd["detection_transformer.ctrl_point_class.0." + leaf].clone()
    batch = make_training_clip()
    hw = tuple(batch[0]["image"].shape[-2:])
    T = cfg.MODEL.TRANSFORMER
    with torch.no_grad():                                        # the frozen detector (gom_oracle.detect_frames up to the head)
        mean, std = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1), torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
        x = torch.stack([(b["image"] - mean) / std for b in batch])
        feats = O.resnet50(x, sd)
        feats = [feats[k] for k in ("res3", "res4", "res5")]
        masks = O.mask_out_padding([f.shape for f in feats], [hw] * len(batch))
        pos = [O.pos_encoding_2d(m, T.HIDDEN_DIM // 2, T.TEMPERATURE) for m in masks]
        out = O.deepsolo_forward(sd, cfg, feats, masks, pos)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("roi_heads.")}
    opt = torch.optim.AdamW([{"params": [p]} for p in params.values()], lr=base_lr, weight_decay=1e-4)
    targets = [{"image_size": hw, "gt_boxes": b["instances"]["gt_boxes"], "gt_instance_ids": b["instances"]["gt_instance_ids"]} for b in batch]
    res_targets = [{"labels": torch.zeros((2,), dtype=torch.long),
                    "ctrl_points": b["instances"]["ctrl_points"] / torch.tensor([hw[1], hw[0]], dtype=torch.float32)} for b in batch]
    print("BASE_LR %g, %d steps, WARMUP_ITERS 0 (multiplier = cosine over MAX_ITER 30000, ~1)" % (base_lr, steps))
    for it in range(steps + 1):
        full = {**sd, **params}
        with torch.no_grad():                                    # training proposals: score threshold, no NMS (gom_lstmatcher.py:231-258)
            re = O.linear(out["query_features"], full, "roi_heads.rescoring_head")
            det = O.detection(cfg, out, re, [hw] * len(batch))
        frames = []
        for r in det:
            pts = r["bd"].reshape(len(r), -1, 2)
            boxes = torch.cat([pts[:, :, 0].min(-1)[0][:, None], pts[:, :, 1].min(-1)[0][:, None], pts[:, :, 0].max(-1)[0][:, None],
                               pts[:, :, 1].max(-1)[0][:, None]], -1) if len(r) else torch.zeros((0, 4))
            frames.append({"image_size": hw, "proposal_boxes": boxes, "objectness_logits": r["scores"], "query_features": r["query_features"]})
        losses = train_oracle.asso_losses(full, cfg, frames, targets)
        losses.update(train_oracle.loss_res(full, cfg, out["query_features"], out["pred_ctrl_points"], res_targets))
        total = sum(losses.values())
        print("step %2d  total %.6f  %s  proposals %s" % (it, float(total), "  ".join("%s %.6f" % (k, float(v)) for k, v in sorted(losses.items())),
                                                           [len(f["proposal_boxes"]) for f in frames]))
        if it == steps:
            break
        opt.zero_grad()
        total.backward()
        norm = torch.nn.utils.clip_grad_norm_(list(params.values()), 0.1)
        opt.step()
        print("         grad norm %.4f" % float(norm))


if __name__ == "__main__":
    main()
