"""Still images for the GEN_IMAGE_MOTION tests: the video dataset of `clip_data_fixture.write_dataset` with records that have
no `video_id` appended -- `make_clip` frames as PNG files, the two boxes of `training_boxes(0)` with straight-edged
`bezier_pts` and NO instance ids (`get_video_dataset_dicts(gen_inst_id=True)` numbers them)."""
import json
import os

from PIL import Image

from clip_data_fixture import box_bezier, training_boxes, write_dataset
from gomatching_amd.synth import make_clip


def write_stills(root, num_videos=0, num_stills=1, height=96, width=128, num_frames=4):
    """-> (json path, image root): `num_videos` videos of `write_dataset` (possibly none) followed by `num_stills` stills with
    image ids 9001, 9002, ..."""
    if num_videos:
        path, image_root = write_dataset(root, num_videos=num_videos, num_frames=num_frames, height=height, width=width)
        with open(path) as f:
            doc = json.load(f)
    else:
        path, image_root = os.path.join(root, "train.json"), os.path.join(root, "frame")
        doc = {"images": [], "annotations": [], "categories": [{"id": 1, "name": "text"}]}
    os.makedirs(os.path.join(image_root, "stills"), exist_ok=True)
    for s in range(num_stills):
        name = os.path.join("stills", "%d.png" % s)
        Image.fromarray(make_clip(1, height, width, clip_id=40 + s)[0]).save(os.path.join(image_root, name))
        image_id = 9001 + s
        doc["images"].append({"id": image_id, "file_name": name, "height": height, "width": width})
        sx, sy = width / 128.0, height / 96.0
        for j, b in enumerate(training_boxes(0)):
            b = [b[0] * sx, b[1] * sy, b[2] * sx, b[3] * sy]
            doc["annotations"].append({"id": 5000 + 10 * s + j, "image_id": image_id, "category_id": 1, "iscrowd": 0,
                                       "bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]], "transcription": ("still", "Zq4")[j],
                                       "bezier_pts": box_bezier(b)})
    with open(path, "w") as f:
        json.dump(doc, f)
    return path, image_root
