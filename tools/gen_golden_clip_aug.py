"""Writes tests/golden/clip_aug.npz: what the REFERENCE's training augmentation computes.  CPU only; needs the reference tree
(oracle/ref_shim.py names its place).

The reference's `EfficientDetResizeCrop` (gomatching/data/transforms/custom_augmentation_impl.py) and
`EfficientDetResizeCropTransform` (custom_transform.py) are imported unmodified.  They subclass fvcore's `Transform` and
Detectron2's `Augmentation`, neither of which is installed: minimal stand-ins (a `Transform` with `_set_attributes`, an empty
`Augmentation`) are put in `sys.modules` for the import -- no arithmetic lives in them.

Recorded, for every case (h, w, TRAIN_SIZE, TRAIN_H, TRAIN_W, scale range, seed k): after `numpy.random.seed(k)`, the
transform's scaled_h, scaled_w, offset_y, offset_x, img_scale, and `apply_coords` of POINTS.  For four tiny uint8 images:
`apply_image`'s output under the transform of one of the cases.

    python tools/gen_golden_clip_aug.py
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

POINTS = np.array([[0.0, 0.0], [1.0, 2.0], [17.25, 3.5], [639.0, 359.0], [1279.5, 719.5]], dtype="float64")

# (h, w, size, train_h, train_w, scale lo, scale hi, seed)
CASES = []
for k, (h, w) in enumerate([(720, 1280), (1080, 1920), (480, 640), (97, 131), (361, 203), (96, 128)]):
    for j, (size, th, tw, lo, hi) in enumerate([(1280, -1, -1, 0.1, 2.0), (640, -1, -1, 0.1, 2.0), (1280, -1, -1, 0.5, 2.0),
                                                (640, 384, 640, 0.1, 2.0), (640, 512, 320, 0.8, 1.2)]):
        CASES.append((h, w, size, th, tw, lo, hi, 100 * k + j))
# the ends of the scale range, exactly: no crop at 0.1 (smaller than the target in both axes), a crop in both axes at 2.0
CASES += [(720, 1280, 1280, -1, -1, 0.1, 0.1, 7), (720, 1280, 1280, -1, -1, 2.0, 2.0, 8), (97, 131, 640, -1, -1, 0.1, 0.1, 9),
          (97, 131, 640, -1, -1, 2.0, 2.0, 10),
          # larger than the target in ONE axis only: a wide source on a tall target, and the reverse
          (96, 256, 640, 128, 64, 1.0, 1.0, 11), (256, 96, 640, 64, 128, 1.0, 1.0, 12),
          (45, 80, 64, -1, -1, 1.5, 1.5, 13), (45, 80, 64, 40, 72, 1.0, 2.0, 14), (37, 53, 64, -1, -1, 0.1, 2.0, 15),
          (37, 53, 32, -1, -1, 2.0, 2.0, 16)]

# tiny images: (h, w, the case whose transform is applied); small sources and targets keep the file to tens of KB
IMAGES = [(33, 47, (33, 47, 48, -1, -1, 1.5, 1.5, 17)),        # odd source, upscaled by 1.53 to 50x72, a 48x48 window
          (45, 80, (45, 80, 64, 40, 72, 1.0, 2.0, 14)),        # non-square target
          (37, 53, (37, 53, 32, -1, -1, 2.0, 2.0, 16)),        # upscaled by 1.2, cropped in both axes
          (40, 64, (40, 64, 64, -1, -1, 0.1, 0.1, 18))]        # downscaled by 10 to 4x6 (21 taps), no crop
CASES += [c for _, _, c in IMAGES if c not in CASES]


def install_stand_ins():
    class Transform:
        def _set_attributes(self, params=None):
            if params:
                for k, v in params.items():
                    if k != "self" and not k.startswith("_"):
                        setattr(self, k, v)

    class Augmentation:
        pass

    names = ("BlendTransform", "CropTransform", "HFlipTransform", "NoOpTransform", "VFlipTransform", "TransformList")
    t = types.ModuleType("fvcore.transforms.transform")
    t.Transform = Transform
    for n in names:
        setattr(t, n, type(n, (Transform,), {}))
    for name in ("fvcore", "fvcore.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["fvcore.transforms.transform"] = t
    a = types.ModuleType("detectron2.data.transforms.augmentation")
    a.Augmentation = Augmentation
    for name in ("detectron2", "detectron2.data", "detectron2.data.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["detectron2.data.transforms.augmentation"] = a
    R = ref_shim.REF_ROOT
    for name, path in (("gomatching", "gomatching"), ("gomatching.data", "gomatching/data"),
                       ("gomatching.data.transforms", "gomatching/data/transforms")):     # skip the reference's __init__ files
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(R, path)]
        sys.modules[name] = m


def main():
    if not ref_shim.reference_available():
        raise SystemExit("reference tree not present at %s" % ref_shim.REF_ROOT)
    install_stand_ins()
    aug = importlib.import_module("gomatching.data.transforms.custom_augmentation_impl")

    def transform_of(case):
        h, w, size, th, tw, lo, hi, k = case
        np.random.seed(k)
        return aug.EfficientDetResizeCrop(size, (lo, hi), h=th, w=tw).get_transform(np.zeros((h, w, 3), np.uint8))

    ints, scales, coords = [], [], []
    for case in CASES:
        t = transform_of(case)
        ints.append([t.scaled_h, t.scaled_w, t.offset_y, t.offset_x, t.target_size[0], t.target_size[1]])
        scales.append(t.img_scale)
        coords.append(t.apply_coords(POINTS.copy()))
    out = {"cases": np.array(CASES, dtype="float64"), "ints": np.array(ints, dtype=np.int64),
           "img_scale": np.array(scales, dtype="float64"), "points": POINTS, "coords": np.array(coords, dtype="float64")}
    rng = np.random.Generator(np.random.Philox(key=0xC11A))
    for i, (h, w, case) in enumerate(IMAGES):
        j = CASES.index(case)
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        res = transform_of(CASES[j]).apply_image(img)
        out["image_%d" % i] = img
        out["image_%d_case" % i] = np.int64(j)
        out["image_%d_out" % i] = np.ascontiguousarray(res)
    path = os.path.join(ROOT, "tests", "golden", "clip_aug.npz")
    np.savez_compressed(path, **out)
    n_crop = sum(1 for r in ints if r[2] or r[3])
    print("wrote %s: %d cases (%d with a non-zero offset), %d bytes" % (path, len(CASES), n_crop, os.path.getsize(path)))
    for i in range(len(IMAGES)):
        print(" image %d: case %d %s -> %s" % (i, out["image_%d_case" % i], ints[int(out["image_%d_case" % i])], out["image_%d_out" % i].shape))


if __name__ == "__main__":
    main()
