"""Writes tests/golden/clip_motion.npz: what the REFERENCE's mapper computes for a still image under
INPUT.VIDEO.GEN_IMAGE_MOTION.  CPU only; needs the reference tree (oracle/ref_shim.py names its place).

`GoMDatasetMapper` (gomatching/data/vts_dataset_mapper.py) cannot be imported without Detectron2, so the two blocks that hold
the rule are cut out of the reference file's TEXT at generation time, compiled and executed unmodified -- nothing of that
text is written here:

  * the `if self.gen_image_motion and is_train:` block of `__init__` (which builds `motion_augmentations` from
    `augmentations[0].target_size[0]`), and
  * the `if gen_image_motion:` block of `__call__` (the two transforms and the interpolation over the frames).

They run against the reference's own `EfficientDetResizeCrop` / `EfficientDetResizeCropTransform`, imported as
tools/gen_golden_clip_aug.py imports them.  The stand-ins hold no arithmetic: `utils.read_image` returns a zero image of the
record's size, and `T.StandardAugInput.apply_augmentations` asks each augmentation for its transform and applies it to the
input's image IN PLACE, as Detectron2's published `AugInput.transform` does -- so the second `apply_augmentations` of the
block sees the first one's crop.  That reading of Detectron2 is the one thing this file does not pin.

Recorded for every case (h, w, TRAIN_SIZE, TRAIN_H, TRAIN_W, TRAIN_LEN, seed k), after `numpy.random.seed(k)`: per frame
scaled_h, scaled_w, offset_y, offset_x and img_scale, and the motion augmentation's target size.

    python tools/gen_golden_clip_motion.py
"""
import copy
import importlib
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden_clip_aug import install_stand_ins  # noqa: E402
from oracle import ref_shim  # noqa: E402

# (h, w, size, train_h, train_w, train_len, seeds)
SHAPES = [(96, 128, 96, -1, -1, 4, 24), (128, 96, 96, -1, -1, 4, 24), (720, 1280, 1280, -1, -1, 6, 8),
          (3000, 4000, 1280, -1, -1, 6, 3), (37, 53, 48, -1, -1, 4, 24), (64, 64, 64, -1, -1, 4, 12), (40, 300, 64, -1, -1, 5, 24),
          (96, 128, 640, 96, 128, 4, 24),       # TRAIN_H != TRAIN_W: the motion target is still the square (TRAIN_H, TRAIN_H)
          (45, 80, 640, 40, 72, 2, 8),          # two frames: st and ed themselves
          (97, 131, 64, -1, -1, 8, 12)]
CASES = [(h, w, size, th, tw, n, 1000 * i + k) for i, (h, w, size, th, tw, n, seeds) in enumerate(SHAPES) for k in range(seeds)]


def cut(lines, first, stop):
    """The lines from the one that reads `first` up to (not including) the next one that starts with `stop`, dedented."""
    a = next(i for i, ln in enumerate(lines) if ln.strip() == first)
    b = next(i for i in range(a + 1, len(lines)) if lines[i].strip().startswith(stop))
    return textwrap.dedent("".join(lines[a:b])), a + 1, b


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not present at %s" % ref_shim.REF_ROOT)
    install_stand_ins()
    aug = importlib.import_module("gomatching.data.transforms.custom_augmentation_impl")
    path = os.path.join(ref_shim.REF_ROOT, "gomatching", "data", "vts_dataset_mapper.py")
    with open(path) as f:
        lines = f.readlines()
    init_src, a0, b0 = cut(lines, "if self.gen_image_motion and is_train:", "@classmethod")
    call_src, a1, b1 = cut(lines, "if gen_image_motion:", "elif self.sample_range")
    print("executing %s lines %d-%d and %d-%d" % (os.path.basename(path), a0, b0, a1, b1))
    init_code = compile(init_src, path, "exec")
    call_code = compile(call_src, path, "exec")

    class StandardAugInput:
        def __init__(self, image):
            self.image = image

        def apply_augmentations(self, augmentations):
            tfms = []
            for a in augmentations:
                t = a.get_transform(self.image)
                self.image = t.apply_image(self.image)           # Detectron2 `AugInput.transform`: in place
                tfms.append(t)
            return tfms

    T = types.SimpleNamespace(StandardAugInput=StandardAugInput)

    ints, scales, targets = [], [], []
    for h, w, size, th, tw, n, k in CASES:
        mapper = types.SimpleNamespace(gen_image_motion=True, train_len=n, image_format="BGR")
        exec(init_code, {"self": mapper, "is_train": True, "EfficientDetResizeCrop": aug.EfficientDetResizeCrop,
                         "augmentations": [aug.EfficientDetResizeCrop(size, (0.1, 2.0), h=th, w=tw)]})
        utils = types.SimpleNamespace(read_image=lambda name, format=None: np.zeros((h, w, 3), np.uint8))
        ns = {"self": mapper, "gen_image_motion": True, "copy": copy, "utils": utils, "T": T,
              "video_dict": {"images": [{"file_name": "still.png", "height": h, "width": w}]}}
        np.random.seed(k)
        exec(call_code, ns)
        tl = ns["transforms_list"]
        assert len(tl) == n == len(ns["images_dict"])
        ints.append([[t[0].scaled_h, t[0].scaled_w, t[0].offset_y, t[0].offset_x] for t in tl] + [[0] * 4] * (8 - n))
        scales.append([float(t[0].img_scale) for t in tl] + [0.0] * (8 - n))
        targets.append(list(mapper.motion_augmentations[0].target_size))
    out = {"cases": np.array(CASES, dtype=np.int64), "ints": np.array(ints, dtype=np.int64),
           "img_scale": np.array(scales, dtype="float64"), "target": np.array(targets, dtype=np.int64)}
    dst = os.path.join(ROOT, "tests", "golden", "clip_motion.npz")
    np.savez_compressed(dst, **out)
    back = sum(1 for r, c in zip(ints, CASES) if r[c[5] - 1][2] < r[0][2] or r[c[5] - 1][3] < r[0][3])
    print("wrote %s: %d clips (%d with an offset that decreases), %d bytes" % (dst, len(CASES), back, os.path.getsize(dst)))


if __name__ == "__main__":
    main()
