"""A tiny video dataset on disk for the data-pipeline tests: `make_clip` frames as PNG files plus the json that
`data.load_video_json` reads, with the boxes of `synth.make_training_clip` and straight-edged `bezier_pts`."""
import json
import os

import numpy as np
from PIL import Image

from gomatching_amd.synth import make_clip


def box_bezier(b):
    """16 numbers: the top edge left to right, then the bottom edge right to left, as cubic control points."""
    xs = np.linspace(b[0], b[2], 4)
    top = [(x, b[1]) for x in xs]
    bottom = [(x, b[3]) for x in xs[::-1]]
    return [float(v) for p in top + bottom for v in p]


def training_boxes(t):
    """The two moving boxes of `synth.make_training_clip` at frame t (XYXY)."""
    return [[10 + 3 * t, 12, 40 + 3 * t, 30], [60, 40 + 2 * t, 100, 62 + 2 * t]]


def write_dataset(root, num_videos=1, num_frames=4, height=96, width=128, clip_id=2):
    """-> (json path, image root).  Video v holds `num_frames` frames of make_clip(clip_id + v); instance ids are
    100 * (v + 1) + 7 and 100 * (v + 1) + 3 (so the loader's remap to 1..N is visible)."""
    image_root = os.path.join(root, "frame")
    images, annotations = [], []
    for v in range(num_videos):
        os.makedirs(os.path.join(image_root, "video_%d" % v), exist_ok=True)
        for t, fr in enumerate(make_clip(num_frames, height, width, clip_id=clip_id + v)):
            name = os.path.join("video_%d" % v, "%d.png" % (t + 1))
            Image.fromarray(fr).save(os.path.join(image_root, name))
            image_id = 1000 * v + t + 1
            images.append({"id": image_id, "file_name": name, "height": height, "width": width, "video_id": v + 1})
            for j, b in enumerate(training_boxes(t)):
                annotations.append({"id": len(annotations) + 1, "image_id": image_id, "category_id": 1, "iscrowd": 0,
                                    "bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]], "instance_id": 100 * (v + 1) + (7, 3)[j],
                                    "transcription": ("text", "Ab9")[j], "bezier_pts": box_bezier(b)})
    path = os.path.join(root, "train.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "text"}]}, f)
    return path, image_root


# the augmentation of the GPU tests: a 96x128 source scaled by exactly 1.5 (144x192), of which a 96x128 window is kept --
# the frame size the trainer tests already run the detector at
AUG_OPTS = ["INPUT.TRAIN_H", "96", "INPUT.TRAIN_W", "128", "INPUT.SCALE_RANGE", "[1.5, 1.5]"]
