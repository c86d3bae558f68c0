"""The raw annotation trees of tests/golden/prepare_raw/ as the prepare command reads them (shared by test_prepare_cpu.py
and test_prepare_gpu.py; no test in here).  The annotation files are committed (tools/gen_golden_prepare.py made them and ran
the reference's converter scripts over them); the .jpg frames are regenerated here from frames.json = {frame directory:
[count, H, W]}."""
import io
import json
import os
import shutil

from helpers import GOLDEN

RAW = os.path.join(GOLDEN, "prepare_raw")
# dataset -> (annotation directory, frame directory) below the tree's root, and the reference's output for it
LAYOUT = {"icdar15": ("ICDAR15/ICDAR15_train", "ICDAR15/frame"),
          "dstext": ("DSText/Train_annotation", "DSText/frame"),
          "bovtext": ("BOVText/Train/train_annotation", "BOVText/frame")}


def video_order():
    with open(os.path.join(RAW, "video_order.json")) as f:
        return json.load(f)


def reference_json(name):
    with open(os.path.join(RAW, name + "_train.json"), "rb") as f:
        return f.read()


def build_tree(root):
    """Copies the annotation files below `root` and writes the frames -> {dataset: (annotations, frames)} absolute paths."""
    from PIL import Image
    for ann, _ in LAYOUT.values():
        shutil.copytree(os.path.join(RAW, ann), os.path.join(root, ann))
    with open(os.path.join(RAW, "frames.json")) as f:
        frames = json.load(f)
    for rel, (count, H, W) in frames.items():
        d = os.path.join(root, rel)
        os.makedirs(d)
        buf = io.BytesIO()
        Image.new("RGB", (W, H), (90, 120, 150)).save(buf, format="JPEG")
        for k in range(1, count + 1):
            with open(os.path.join(d, "%d.jpg" % k), "wb") as f:
                f.write(buf.getvalue())
    return {name: (os.path.join(root, ann), os.path.join(root, fr)) for name, (ann, fr) in LAYOUT.items()}
