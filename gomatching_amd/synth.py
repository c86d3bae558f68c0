"""Synthetic clips for parity tests and the benchmark (SURVEY.md §8-d "Synthetic inputs").

Frames are uint8 RGB: seed-indexed smooth noise plus K moving high-contrast rectangles so that
detections persist across frames.  Generator: numpy Philox keyed by 0x60A7 + clip_id.
"""
import numpy as np


def make_clip(num_frames, height, width, clip_id=0, num_rects=6):
    rng = np.random.Generator(np.random.Philox(key=0x60A7 + clip_id))
    # smooth background: low-res noise upsampled by pixel replication + a gradient
    gh, gw = max(2, height // 32), max(2, width // 32)
    low = rng.uniform(60, 160, size=(gh, gw, 3)).astype(np.float32)
    yy = (np.arange(height) * gh // height).clip(0, gh - 1)
    xx = (np.arange(width) * gw // width).clip(0, gw - 1)
    base = low[yy][:, xx]
    base += np.linspace(0, 30, width, dtype=np.float32)[None, :, None]
    rects = []
    for _ in range(num_rects):
        w = int(rng.integers(width // 10, width // 4))
        h = int(rng.integers(height // 14, height // 6))
        x = float(rng.uniform(0, width - w))
        y = float(rng.uniform(0, height - h))
        vx, vy = rng.uniform(-0.01, 0.01, size=2) * (width, height)
        fg = rng.uniform(200, 255, size=3).astype(np.float32)
        bg = rng.uniform(0, 40, size=3).astype(np.float32)
        rects.append((x, y, w, h, vx, vy, fg, bg))
    frames = []
    for t in range(num_frames):
        img = base + rng.uniform(-3, 3, size=base.shape).astype(np.float32)
        for (x, y, w, h, vx, vy, fg, bg) in rects:
            x0 = int(np.clip(x + vx * t, 0, width - w))
            y0 = int(np.clip(y + vy * t, 0, height - h))
            img[y0:y0 + h, x0:x0 + w] = bg
            # "glyph" stripes
            for s in range(x0 + 2, x0 + w - 2, max(4, w // 8)):
                img[y0 + h // 5: y0 + h - h // 5, s:s + max(2, w // 16)] = fg
        frames.append(np.clip(img, 0, 255).astype(np.uint8))
    return frames


# Calibration of the synthetic weights for the training clip below: detector and rescoring biases that let detections pass
TRAINING_CLS_BIAS = {"detection_transformer.ctrl_point_class.0.bias": 0.8, "roi_heads.rescoring_head.bias": 0.8}


def make_training_clip(num_frames=4, height=96, width=128, clip_id=2):
    """`make_clip` frames as mapped training inputs: per frame {"image" [3,H,W] float32 tensor, "instances": two moving
    ground-truth boxes with instance ids 1 and 2 and their 25 control points (pixels)}.  The ONE clip that the trainer test,
    tools/solver_rehearsal.py and tools/solver_bench.py use, so that the rehearsal's chosen learning rate stays valid."""
    import torch
    batch = []
    for t, fr in enumerate(make_clip(num_frames, height, width, clip_id=clip_id)):
        boxes = np.array([[10 + 3 * t, 12, 40 + 3 * t, 30], [60, 40 + 2 * t, 100, 62 + 2 * t]], np.float32)
        ctrl = np.stack([np.stack([np.linspace(b[0], b[2], 25), np.full(25, (b[1] + b[3]) / 2)], -1) for b in boxes]).astype(np.float32)
        batch.append({"image": torch.as_tensor(fr.astype("float32").transpose(2, 0, 1)),
                      "instances": {"gt_boxes": torch.as_tensor(boxes), "gt_instance_ids": torch.tensor([1, 2]),
                                    "ctrl_points": torch.as_tensor(ctrl)}})
    return batch
