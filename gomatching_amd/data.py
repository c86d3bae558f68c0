"""Training data: the reference's dataset, sampler, mapper and loader modules under their own names, without Detectron2,
fvcore, pycocotools, cv2 or shapely.

  * `load_video_json`            gomatching/data/datasets/vts.py:24-187 over plain `json`;
  * `get_video_dataset_dicts`    gomatching/data/vts_dataset_dataloader.py:96-136;
  * `resize_crop_params`         `EfficientDetResizeCrop.get_transform` (data/transforms/custom_augmentation_impl.py:47-66) as a
                                 pure function of its three uniform draws; `apply_coords` / `apply_box` / `apply_image` are the
                                 transform's (data/transforms/custom_transform.py:46-84);
  * `sample_clip`                the frame choice of `GoMDatasetMapper.__call__` (data/vts_dataset_mapper.py:157-210) as a pure
                                 function of a `numpy.random.Generator`;
  * `GoMDatasetMapper`           data/vts_dataset_mapper.py:94-259 + `custom_transform_instance_annotations`
                                 (data/custom_dataset_mapper.py:41-103);
  * `build_vts_train_loader`     data/vts_dataset_dataloader.py:27-71, as an iterator whose clip at iteration i is a pure
                                 function of (seed, i, rank, world_size).

With `device_ingest` the mapper hands the decoded u8 frames and the augmentation's numbers to the model, whose input stage
resizes, crops and normalises the whole clip in one launch (`ops.ingest_crop`, csrc/ingest.hip); without it the mapper does
the reference's Pillow resize and slice on the host.  Both give the same bits.

PINNED against the reference's own classes (tests/golden/clip_aug.npz, tools/gen_golden_clip_aug.py): the augmentation's
numbers, `apply_coords`, `apply_image`.  UNPINNED -- restated from published source, no Detectron2 here to run them against:
Detectron2's `Transform.apply_box` (corners through `apply_coords`, then min / max), `filter_empty_instances` (boxes wider
and taller than 1e-5) and `TrainingSampler` (an endless stream of shuffled epochs, position p of it served by rank
p % world_size); pycocotools' grouping of annotations by `image_id` in file order; the frame-sampling logic itself, which is
read off vts_dataset_mapper.py but cannot be executed without Detectron2 (and draws from a `Generator` handed in, not from
numpy's global state: the reference's stream of draws is not reproduced, its distribution is); decoding with Pillow instead
of `detection_utils.read_image` (no EXIF transposition; JPEG decoders differ in IDCT and chroma upsampling).

Still images (`INPUT.VIDEO.GEN_IMAGE_MOTION`, vts_dataset_mapper.py:137-140, 162-163, 181-202, 218-220) are OPT-IN:
`GoMDatasetMapper(..., image_motion=True)` / `train --image-motion` turn a one-image video into a clip of TRAIN_LEN copies of
the image, frame x under numbers of its own (`motion_clip_params`).  The rule: two `EfficientDetResizeCrop(size, (0.8, 1.2))`
transforms on the SQUARE target (size, size), size = `target_size_of(INPUT)[0]`, are drawn -- `st` for the image, `ed` for the
image AS `st` LEFT IT (its crop, not the source: Detectron2 applies an augmentation to its `AugInput` in place) -- and offsets
(floor division) and scale (float64) are interpolated linearly over the frames, the scaled size taken from the SOURCE size.  A
3000x4000 source on a 1280 target therefore zooms in about threefold over the clip: the reference's behaviour, kept.  The
frames of such a clip differ in resized size and window, so the model pads them into one batch (`ops.ingest_motion`: one
image upload, one table upload, one launch) and runs the detector per group of equal sizes (`training.forward_losses`).
Without the flag a one-image video is refused as before: the refusals are what existing callers and tests rely on, and making
motion the default under GEN_IMAGE_MOTION is a later, separate change.
PINNED: the interpolation, by executing the reference's own lines 181-202 (tools/gen_golden_clip_motion.py compiles them from
the reference file's text at generation time; tests/golden/clip_motion.npz).  UNPINNED: that `ed` sees `st`'s crop -- the
generator's `StandardAugInput` stand-in applies a transform in place as Detectron2's published source does, but Detectron2
is not here to run.

Deliberately not built (each raises, naming what it met): `poly` quads and 14-gons (they need `cv2.minAreaRect`, shapely and
a Bezier fit: such an annotation loads without its point fields, and a WITH_RESR config fails on it at mapping time),
`GEN_IMAGE_MOTION` on one-image videos unless asked for with `image_motion`, `MultiDatasetSampler`,
`RepeatFactorTrainingSampler`, the `ResizeShortestEdge` training augmentation.
"""
import collections
import copy
import itertools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .config import _merge, _unwrap, _wrap
from .predictor import CTLABELS_37

# character -> class id of the 37-way recogniser: the table the predictor decodes with, read the other way
CTLABELS = {ch: k for k, ch in enumerate(CTLABELS_37)}
TEXT_LEN, TEXT_UNKNOWN, TEXT_PAD = 25, 36, 37

# datasets/vts.py:216-226, under "datasets/" (:232-233): name -> (image root, json file)
PREDEFINED_SPLITS = {
    "icdar15_train": ("ICDAR15/frame/", "ICDAR15/train.json"),
    "dstext_train": ("DSText/frame/", "DSText/train.json"),
    "artvideo_train": ("ArTVideo/Train/frame/", "ArTVideo/Train/train.json"),
    "bov_train": ("BOVText/frame/", "BOVText/train.json"),
}

# gomatching/config.py:48-64 (INPUT) and Detectron2 v0.6's DATALOADER defaults (UNPINNED, as solver._D2_DEFAULTS)
_INPUT_DEFAULTS = {"FORMAT": "BGR", "CUSTOM_AUG": "", "TRAIN_SIZE": 640, "TRAIN_H": -1, "TRAIN_W": -1, "SCALE_RANGE": (0.1, 2.0),
                   "NOT_CLAMP_BOX": False,
                   "VIDEO": {"TRAIN_LEN": 8, "SAMPLE_RANGE": 2.0, "DYNAMIC_SCALE": True, "GEN_IMAGE_MOTION": True}}
_DATALOADER_DEFAULTS = {"SAMPLER_TRAIN": "TrainingSampler", "NUM_WORKERS": 4}
MAX_DECODE_THREADS = 16
LOOKAHEAD_CLIPS = 3


def data_cfg(cfg):
    """The INPUT and DATALOADER blocks of `cfg` over the defaults above -> CfgNode {INPUT, DATALOADER}.  `cfg` is left as it is
    (`config._DEFAULTS` holds inference-path keys only), as `solver.solver_cfg` does for SOLVER."""
    if not isinstance(cfg, dict):
        raise TypeError("data_cfg: expected a config node or dict, got %s" % type(cfg).__name__)
    d = {"INPUT": copy.deepcopy(_INPUT_DEFAULTS), "DATALOADER": copy.deepcopy(_DATALOADER_DEFAULTS)}
    _merge(d["INPUT"], _unwrap(cfg.get("INPUT") or {}))
    _merge(d["DATALOADER"], _unwrap(cfg.get("DATALOADER") or {}))
    return _wrap(d)


def resolve_split(name, root="datasets"):
    """-> (json file, image root) of a `DATASETS.TRAIN` name, as datasets/vts.py:228-234 registers it."""
    if name not in PREDEFINED_SPLITS:
        raise KeyError("dataset %r is not in the split table (%s)" % (name, ", ".join(sorted(PREDEFINED_SPLITS))))
    image_root, json_file = PREDEFINED_SPLITS[name]
    return os.path.join(root, json_file), os.path.join(root, image_root)


# ------------------------------------------------------------------------------------------------- dataset
def encode_text(transcription, text_category=None):
    """The `texts` row of an annotation (what vts.py:131-148 produces): TEXT_LEN int32 class ids of the lower-cased
    transcription, characters outside the table as TEXT_UNKNOWN, the rest TEXT_PAD.  A '###' transcription, the
    'nonalphanumeric' category and a missing or empty transcription all read as one unknown character."""
    row = np.full(TEXT_LEN, TEXT_PAD, dtype=np.int32)
    lowered = transcription.lower() if transcription else ""
    if not lowered or lowered == "###" or text_category == "nonalphanumeric":
        row[0] = TEXT_UNKNOWN
        return row
    ids = [CTLABELS.get(ch, TEXT_UNKNOWN) for ch in lowered[:TEXT_LEN]]
    row[:len(ids)] = ids
    return row


def _bernstein3(n):
    """[n,4]: the cubic Bernstein basis at n evenly spaced parameters of [0, 1]."""
    u = np.linspace(0.0, 1.0, n)
    v = 1.0 - u
    return np.stack([v * v * v, 3.0 * u * v * v, 3.0 * u * u * v, u * u * u], axis=1)


_BERNSTEIN_25 = _bernstein3(TEXT_LEN)


def bezier_fields(bezier_pts):
    """The point fields vts.py:168-179 derives from `bezier_pts` = 16 numbers, the control points of the top curve and then of
    the bottom curve, which runs backwards: beziers [4,2], the control points of the centre line; boundary [50,2], point i
    of the top curve followed by the bottom curve's point under it, i = 0..24; polyline [25,2], the centre line.  float64."""
    ctrl = np.asarray(bezier_pts, dtype=np.float64).reshape(2, 4, 2)
    top_ctrl, under_ctrl = ctrl[0], ctrl[1][::-1]                 # both left to right
    top, under = _BERNSTEIN_25 @ top_ctrl, _BERNSTEIN_25 @ under_ctrl
    return {"beziers": (top_ctrl + under_ctrl) / 2,
            "boundary": np.stack([top, under], axis=1).reshape(-1, 2),
            "polyline": (top + under) / 2}


def load_video_json(json_file, image_root, extra_annotation_keys=("instance_id",), map_inst_id=True):
    """`load_video_json` (datasets/vts.py:24-187) as `register_vts_instances` calls it (:196-198), over plain json: one
    record per image, sorted by image id, {file_name, height, width, image_id, video_id, annotations}.  An annotation keeps
    `bbox` (XYWH, "bbox_mode": "XYWH_ABS"), `iscrowd`, `category_id` (contiguous: index among the sorted ids of
    `categories`), `instance_id` (sorted positive ids -> 1..N; 0 and -1 -> 0), `texts`, and from `bezier_pts` the fields
    of `bezier_fields`.  `poly`-only annotations load WITHOUT the point fields (module doc-string); "annotation_id" names
    them in later errors.  Segmentations and keypoints, which the mapper drops (use_instance_mask / use_keypoint are off),
    are not read."""
    with open(json_file, "r") as f:
        doc = json.load(f)
    annotations = doc.get("annotations", [])
    by_image = collections.defaultdict(list)                     # pycocotools' imgToAnns: file order within an image
    for ann in annotations:
        by_image[ann["image_id"]].append(ann)
    category_index = {cid: k for k, cid in enumerate(sorted(c["id"] for c in doc.get("categories", [])))}
    instance_index = None
    if map_inst_id:
        if "instance_id" not in extra_annotation_keys:
            raise ValueError("load_video_json: map_inst_id needs 'instance_id' among extra_annotation_keys")
        positive = sorted({ann["instance_id"] for ann in annotations if ann.get("instance_id", 0) > 0})
        instance_index = dict(zip(positive, range(1, len(positive) + 1)))
        instance_index.update({0: 0, -1: 0})
    copied = ("iscrowd", "bbox", "category_id") + tuple(extra_annotation_keys or ())
    records = []
    for img in sorted(doc.get("images", []), key=lambda im: im["id"]):
        objs = []
        for ann in by_image.get(img["id"], []):
            if ann.get("ignore", 0) != 0:
                raise ValueError("annotation %r: an `ignore` flag is not supported" % (ann.get("id"),))
            obj = {k: ann[k] for k in copied if k in ann}
            obj.update(bbox_mode="XYWH_ABS", annotation_id=ann.get("id"),
                       texts=encode_text(ann.get("transcription"), ann.get("text_category")))
            if category_index:
                if obj["category_id"] not in category_index:
                    raise KeyError("annotation %r: category_id %r is not among the json's `categories`"
                                   % (ann.get("id"), obj["category_id"]))
                obj["category_id"] = category_index[obj["category_id"]]
            if instance_index is not None:
                obj["instance_id"] = instance_index[obj.get("instance_id", 0)]     # a still's annotations may carry none
            if ann.get("bezier_pts") is not None:
                obj.update(bezier_fields(ann["bezier_pts"]))
            elif "poly" in ann and np.size(ann["poly"]) not in (8, 28):
                raise ValueError("annotation %r: `poly` has %d numbers; a quad (8) or a 14-gon (28) is expected"
                                 % (ann.get("id"), np.size(ann["poly"])))
            objs.append(obj)
        records.append({"file_name": os.path.join(image_root, img["file_name"]), "height": img["height"], "width": img["width"],
                        "image_id": img["id"], "video_id": img.get("video_id", -1), "annotations": objs})
    return records


FIRST_GENERATED_ID = 1000001           # one-image "videos" and generated instance ids are numbered from here (the reference's base)


def get_video_dataset_dicts(dataset_dicts_per_source, gen_inst_id=False):
    """vts_dataset_dataloader.py:96-136 over the loaded record lists themselves (there is no catalog here): one
    {'video_id', 'images', 'dataset_source'} per video in order of first appearance, sources one after the other; a record
    without a video id (-1) becomes a one-image video, numbered from FIRST_GENERATED_ID within its source; `gen_inst_id`
    gives every annotation without a positive instance id one of its own, numbered from FIRST_GENERATED_ID over all sources."""
    if not dataset_dicts_per_source:
        raise ValueError("get_video_dataset_dicts: no dataset")
    fresh_instance = itertools.count(FIRST_GENERATED_ID)
    out = []
    for source, records in enumerate(dataset_dicts_per_source):
        if not records:
            raise ValueError("get_video_dataset_dicts: dataset %d is empty" % source)
        fresh_video = itertools.count(FIRST_GENERATED_ID)
        videos = {}
        for rec in records:
            vid = rec.get("video_id", -1)
            if vid == -1:
                vid = next(fresh_video)
            if gen_inst_id:
                for ann in rec["annotations"]:
                    if ann.get("instance_id", 0) <= 0:
                        ann["instance_id"] = next(fresh_instance)
            videos.setdefault(vid, {"video_id": vid, "images": [], "dataset_source": source})["images"].append(rec)
        out.extend(videos.values())
    return out


# -------------------------------------------------------------------------------------------- augmentation
def target_size_of(input_cfg):
    """custom_augmentation_impl.py:40-43 with the arguments of custom_build_augmentation.py:22-27."""
    h, w = input_cfg.TRAIN_H, input_cfg.TRAIN_W
    if h < 0 and w < 0:
        return (input_cfg.TRAIN_SIZE, input_cfg.TRAIN_SIZE)
    return (h, w)


def resize_crop_params(height, width, target_hw, u_scale, u_y, u_x):
    """The numbers of `EfficientDetResizeCrop.get_transform` (custom_augmentation_impl.py:47-66) for its three draws in the
    order it makes them: u_scale = uniform(*SCALE_RANGE), u_y = uniform(0, 1), u_x = uniform(0, 1).
    -> (scaled_h, scaled_w, offset_y, offset_x, img_scale).

    The float expressions and the truncations are the reference's, because the integers must be: the scaled target is
    `u_scale * target` per axis, the image scale the smaller of the two quotients by the source size, the scaled size
    `int(source * scale)`, and an offset `int(max(0.0, float(scaled - target)) * u)` (0 where the scaled image fits)."""
    th, tw = target_hw
    img_scale = min(u_scale * th / height, u_scale * tw / width)
    scaled = (int(height * img_scale), int(width * img_scale))
    offset_y, offset_x = (int(max(0.0, float(have - want)) * u) for have, want, u in zip(scaled, (th, tw), (u_y, u_x)))
    return scaled[0], scaled[1], offset_y, offset_x, img_scale


def crop_window(params, target_hw):
    """(y0, x0, OH, OW) of custom_transform.py:54-57 inside the scaled image."""
    scaled_h, scaled_w, offset_y, offset_x, _ = params
    lower = min(scaled_h, offset_y + target_hw[0])
    right = min(scaled_w, offset_x + target_hw[1])
    return offset_y, offset_x, lower - offset_y, right - offset_x


def apply_coords(coords, params):
    """custom_transform.py:79-84 on a float64 copy: (x, y) * img_scale - (offset_x, offset_y), the product rounded before
    the subtraction."""
    pts = np.array(coords, dtype=np.float64).reshape(-1, 2)
    return pts * params[4] - np.array([params[3], params[2]], dtype=np.float64)


def apply_box(box, params):
    """Detectron2 `Transform.apply_box` for one XYXY box (UNPINNED): its four corners through `apply_coords`, then the
    minimum and the maximum per axis."""
    box = np.asarray(box, dtype="float64").reshape(4)
    idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    coords = apply_coords(box[idxs].reshape(-1, 2), params)
    return np.concatenate((coords.min(axis=0), coords.max(axis=0)))


def apply_image(img, params, target_hw):
    """custom_transform.py:46-59 for a uint8 HxWx3 image: Pillow bilinear resize to (scaled_w, scaled_h), then the slice."""
    from PIL import Image
    assert img.dtype == np.uint8
    y0, x0, oh, ow = crop_window(params, target_hw)
    ret = np.asarray(Image.fromarray(img).resize((params[1], params[0]), Image.BILINEAR))
    return ret[y0:y0 + oh, x0:x0 + ow]


MOTION_SCALE_RANGE = (0.8, 1.2)         # vts_dataset_mapper.py:138-140: the scale range of the motion augmentation


class MotionPlan(list):
    """The transform numbers of a GEN_IMAGE_MOTION clip: one `resize_crop_params` tuple PER FRAME (what `GoMDatasetMapper.plan`
    returns in place of the one tuple of a video clip)."""


def motion_clip_params(height, width, size, train_len, rng):
    """The per-frame transforms of a GEN_IMAGE_MOTION clip (vts_dataset_mapper.py:181-202) for a `height` x `width` still:
    `train_len` tuples (scaled_h, scaled_w, offset_y, offset_x, img_scale), as `resize_crop_params` returns them, in a
    `MotionPlan`.  The window of a frame is `crop_window(params, (size, size))`.

    Two transforms of `EfficientDetResizeCrop(size, MOTION_SCALE_RANGE)` on the SQUARE target (size, size) are drawn from
    `rng`, six uniforms in the order `sample_clip` makes them (scale, y, x for `st`, then for `ed`): `st` for the source,
    `ed` for the image as `st` left it, (OH, OW) of `st`'s window (UNPINNED: Detectron2's `AugInput` is transformed in
    place by `apply_augmentations`, so the second `get_transform` sees the first one's crop; Detectron2 is not here to
    run).  Frame x of n: offset = st + (ed - st) * x // (n - 1) per axis in Python ints (floor division: the difference may
    be negative), img_scale = st + (ed - st) * x / (n - 1) in float64, scaled size = int(source * img_scale)."""
    n = int(train_len)
    if n < 2:
        raise ValueError("motion_clip_params: train_len %r: the interpolation divides by train_len - 1" % (train_len,))
    target = (size, size)

    def draw(h, w):
        u_scale, u_y, u_x = rng.uniform(*MOTION_SCALE_RANGE), rng.uniform(0, 1), rng.uniform(0, 1)
        return resize_crop_params(h, w, target, u_scale, u_y, u_x)

    st = draw(height, width)
    ed = draw(*crop_window(st, target)[2:])
    plan = MotionPlan()
    for x in range(n):
        offset_y = st[2] + (ed[2] - st[2]) * x // (n - 1)
        offset_x = st[3] + (ed[3] - st[3]) * x // (n - 1)
        img_scale = st[4] + (ed[4] - st[4]) * x / (n - 1)
        plan.append((int(height * img_scale), int(width * img_scale), offset_y, offset_x, img_scale))
    return plan


# ------------------------------------------------------------------------------------------------ sampling
def sample_clip(video_dict, rng, train_len, target_hw, scale_range, sample_range=2.0, dynamic_scale=True,
                gen_image_motion=True):
    """The frame choice of `GoMDatasetMapper.__call__` in training (vts_dataset_mapper.py:157-210) -> (indices into
    video_dict['images'], transform numbers of `resize_crop_params`).  Draws, in the reference's order, from `rng`:
    the start frame; under DYNAMIC_SCALE the transform (from frame `st`'s size), then, when
    max_frames = int(n * (target / auged) ** 2) exceeds TRAIN_LEN, a length in [TRAIN_LEN, max_frames] capped at
    2 * TRAIN_LEN and the video; under SAMPLE_RANGE > 1 a sorted choice without replacement from [st, ed); without
    DYNAMIC_SCALE the transform last, from the first chosen frame.  ONE transform serves the clip (:221-225: `transforms`
    is no longer None after the first frame)."""
    images = video_dict["images"]
    n_images = len(images)
    if gen_image_motion and n_images == 1:
        raise NotImplementedError("video %r has one image: INPUT.VIDEO.GEN_IMAGE_MOTION (a transform per frame, mixed-size "
                                  "batches) is not built; set INPUT.VIDEO.GEN_IMAGE_MOTION false" % (video_dict.get("video_id"),))

    def draw_transform(record):
        u_scale, u_y, u_x = rng.uniform(*scale_range), rng.uniform(0, 1), rng.uniform(0, 1)
        return resize_crop_params(record["height"], record["width"], target_hw, u_scale, u_y, u_x)

    length = min(n_images, train_len)
    first = int(rng.integers(n_images - length + 1))
    params = draw_transform(images[first]) if dynamic_scale else None
    if dynamic_scale:
        # a clip scaled down leaves room for more frames: as many as keep the pixel count, between TRAIN_LEN and 2 * TRAIN_LEN
        room = int(length * (max(target_hw) / max(params[0], params[1])) ** 2)
        if room > train_len:
            drawn = train_len + int(rng.integers(room - train_len + 1))
            length = min(drawn, 2 * train_len, n_images)
    if sample_range > 1.0:
        stop = min(first + int(sample_range * length), n_images)
        length = min(length, stop - first)
        inds = sorted(int(k) for k in rng.choice(np.arange(first, stop), size=length, replace=False))
    else:
        inds = list(range(first, min(first + length, n_images)))
    if params is None:
        params = draw_transform(images[inds[0]])
    return inds, params


# -------------------------------------------------------------------------------------------------- mapper
def read_image(path, fmt):
    """HxWx3 uint8 in `fmt` order ("RGB" or "BGR"), decoded with Pillow (UNPINNED against `detection_utils.read_image`)."""
    from PIL import Image
    with Image.open(path) as im:
        image = np.array(im.convert("RGB"))                      # a writable copy: torch.from_numpy wants one
    if fmt == "BGR":
        image = image[:, :, ::-1]
    elif fmt != "RGB":
        raise NotImplementedError("INPUT.FORMAT %r: only RGB and BGR are built" % (fmt,))
    return np.ascontiguousarray(image)


class GoMDatasetMapper:
    """`GoMDatasetMapper` (vts_dataset_mapper.py:94-259) in training: video dict -> list of per-frame dicts, each with
    height, width, image_id, video_id, file_name, `instances` (a dict as `training.forward_losses` takes: gt_boxes f32 XYXY
    after `apply_box`, gt_classes, gt_instance_ids, texts, and beziers / polyline / boundary when every kept annotation has
    them) and the frame itself:

      device_ingest=True   `frame_u8` (u8 [H,W,3] as decoded, INPUT.FORMAT order), `resize_hw`, `crop` = (y0, x0, OH, OW),
                           `flip_channels` False -- the model's input stage does resize + crop + normalise in one launch;
      device_ingest=False  the reference's `image`: u8 [3,h,w] from Pillow resize and slice on the host.

    `image_motion=True` (opt-in; module doc-string) with GEN_IMAGE_MOTION and a one-image video: the clip is TRAIN_LEN copies
    of the record, frame x under its own numbers (`motion_clip_params`; DYNAMIC_SCALE does not apply), the file decoded ONCE.
    Every frame dict carries `motion: True`; with device ingest they all hold the SAME `frame_u8` tensor and their own
    `resize_hw` / `crop` / `flip_channels`, with host ingest their own `image`.  Annotations are transformed per frame; the
    instance ids are those `get_video_dataset_dicts(gen_inst_id=True)` gave, equal in all frames.  For such a clip `plan`
    returns (TRAIN_LEN times the record, a `MotionPlan`: per-frame numbers instead of one tuple) and `map_clip` maps it.

    `mapper(video_dict, rng)`: every draw comes from the `numpy.random.Generator` handed in.  `plan` (the draws) and
    `map_frame` (decoding and the per-frame work, free of shared state) are separate so that a loader can decode the frames
    of a planned clip in parallel."""

    def __init__(self, cfg, is_train=True, device_ingest=True, image_motion=False):
        if not is_train:
            raise NotImplementedError("GoMDatasetMapper: only the training mapper is built (inference reads frames in eval.py)")
        D = data_cfg(cfg)
        I = D.INPUT
        if I.CUSTOM_AUG != "EfficientDetResizeCrop":
            raise NotImplementedError("INPUT.CUSTOM_AUG %r: only EfficientDetResizeCrop is built for training" % (I.CUSTOM_AUG,))
        if I.FORMAT not in ("RGB", "BGR"):
            raise NotImplementedError("INPUT.FORMAT %r: only RGB and BGR are built" % (I.FORMAT,))
        self.is_train, self.device_ingest = is_train, bool(device_ingest)
        self.image_format = I.FORMAT
        self.target_size = tuple(int(v) for v in target_size_of(I))
        scale = I.SCALE_RANGE                                    # a yaml "(0.1, 2.0)", as the reference's files write it, is a string
        if isinstance(scale, str):
            import ast
            scale = ast.literal_eval(scale)
        self.scale = tuple(float(v) for v in scale)
        if len(self.scale) != 2:
            raise ValueError("INPUT.SCALE_RANGE %r: expected (low, high)" % (I.SCALE_RANGE,))
        self.train_len = int(I.VIDEO.TRAIN_LEN)
        self.not_clamp_box = bool(I.NOT_CLAMP_BOX)
        self.sample_range = float(I.VIDEO.SAMPLE_RANGE)
        self.dynamic_scale = bool(I.VIDEO.DYNAMIC_SCALE)
        self.gen_image_motion = bool(I.VIDEO.GEN_IMAGE_MOTION)
        self.with_resr = bool(cfg.MODEL.ROI_HEADS.WITH_RESR)
        self.image_motion = bool(image_motion)
        self.motion_size = self.target_size[0]                   # :139-140: `augmentations[0].target_size[0]`, a square target
        if self.image_motion and self.gen_image_motion and self.train_len < 2:
            raise ValueError("INPUT.VIDEO.TRAIN_LEN %d: GEN_IMAGE_MOTION interpolates over TRAIN_LEN - 1 steps and needs at "
                             "least 2 frames" % self.train_len)

    def plan(self, video_dict, rng):
        """-> (frame records of the clip, transform numbers).  No file is opened: sizes are the json's.  For a one-image
        video under `image_motion`: (TRAIN_LEN times the record, `MotionPlan` of per-frame numbers)."""
        if self.image_motion and self.gen_image_motion and len(video_dict["images"]) == 1:
            rec = video_dict["images"][0]
            plan = motion_clip_params(rec["height"], rec["width"], self.motion_size, self.train_len, rng)
            for x, p in enumerate(plan):
                y0, x0, oh, ow = crop_window(p, (self.motion_size, self.motion_size))
                if min(oh, ow) <= 0 or y0 < 0 or x0 < 0 or y0 + oh > p[0] or x0 + ow > p[1]:
                    raise ValueError("video %r: frame %d of its motion clip has the window (y0=%d, x0=%d, %dx%d) in a %dx%d "
                                     "resized image" % (video_dict.get("video_id"), x, y0, x0, oh, ow, p[0], p[1]))
            return [rec] * self.train_len, plan
        inds, params = sample_clip(video_dict, rng, self.train_len, self.target_size, self.scale, self.sample_range,
                                   self.dynamic_scale, self.gen_image_motion)
        records = [video_dict["images"][x] for x in inds]
        sizes = set((r["height"], r["width"]) for r in records)
        if len(sizes) != 1:
            raise ValueError("video %r: the frames of one clip must share a source size, got %s"
                             % (video_dict.get("video_id"), sorted(sizes)))
        return records, params

    def _annotation(self, obj, params, image_shape, record):
        """`custom_transform_instance_annotations` (custom_dataset_mapper.py:41-72) for one annotation."""
        x, y, w, h = obj["bbox"]
        bbox = apply_box([x, y, x + w, y + h], params)
        if not self.not_clamp_box:
            bbox = np.minimum(bbox.clip(min=0), list(image_shape + image_shape)[::-1])
        out = {"bbox": bbox, "category_id": obj.get("category_id", 0), "instance_id": obj.get("instance_id", 0),
               "texts": obj["texts"]}
        for key in ("beziers", "polyline", "boundary"):
            if key in obj:
                out[key] = apply_coords(obj[key], params).reshape(-1)
        if self.with_resr and "polyline" not in out:
            raise ValueError("annotation %r of image %r (%s) has no `bezier_pts`: MODEL.ROI_HEADS.WITH_RESR needs control points, "
                             "and the `poly` -> Bezier conversion is not built; `bezier_pts` must be precomputed in the json"
                             % (obj.get("annotation_id"), record["image_id"], record["file_name"]))
        return out

    def _decode(self, record):
        image = read_image(record["file_name"], self.image_format)
        if (image.shape[0], image.shape[1]) != (record["height"], record["width"]):     # detection_utils.check_image_size
            raise ValueError("Mismatched image shape for image %s, got %s, expect %s. Please check the width/height in your "
                             "annotation." % (record["file_name"], (image.shape[0], image.shape[1]),
                                              (record["height"], record["width"])))
        return image

    def map_frame(self, record, params):
        import torch
        image = self._decode(record)
        return self._frame(record, image, torch.from_numpy(image) if self.device_ingest else None, params, self.target_size)

    def map_clip(self, records, params):
        """The frames of a planned clip.  A `MotionPlan`: one decode, frame x under params[x] on the square motion target."""
        if not isinstance(params, MotionPlan):
            return [self.map_frame(r, params) for r in records]
        import torch
        image = self._decode(records[0])
        shared = torch.from_numpy(image) if self.device_ingest else None
        target = (self.motion_size, self.motion_size)
        return [dict(self._frame(r, image, shared, p, target), motion=True) for r, p in zip(records, params)]

    def _frame(self, record, image, frame_u8, params, target_size):
        import torch
        y0, x0, oh, ow = crop_window(params, target_size)
        image_shape = (oh, ow)
        out = {k: record[k] for k in ("file_name", "height", "width", "image_id", "video_id")}
        if self.device_ingest:
            out.update(frame_u8=frame_u8, resize_hw=(params[0], params[1]), crop=(y0, x0, oh, ow), flip_channels=False)
        else:
            out["image"] = torch.as_tensor(np.ascontiguousarray(apply_image(image, params, target_size).transpose(2, 0, 1)))
        annos = [self._annotation(obj, params, image_shape, record) for obj in record.get("annotations", [])
                 if obj.get("iscrowd", 0) == 0]
        boxes = torch.as_tensor(np.array([a["bbox"] for a in annos], dtype="float64").reshape(-1, 4), dtype=torch.float32)
        inst = {"gt_boxes": boxes,
                "gt_classes": torch.tensor([a["category_id"] for a in annos], dtype=torch.int64),
                "gt_instance_ids": torch.tensor([a["instance_id"] for a in annos], dtype=torch.int64),
                "texts": torch.as_tensor(np.array([a["texts"] for a in annos], dtype=np.int32).reshape(-1, TEXT_LEN))}
        if all("polyline" in a for a in annos):
            for key, width in (("beziers", 8), ("polyline", 50), ("boundary", 100)):
                inst[key] = torch.as_tensor(np.array([a[key] for a in annos], dtype="float64").reshape(-1, width),
                                            dtype=torch.float32)
        # filter_empty_instances: boxes wider and taller than 1e-5 stay
        keep = ((boxes[:, 2] - boxes[:, 0]) > 1e-5) & ((boxes[:, 3] - boxes[:, 1]) > 1e-5)
        out["instances"] = {k: v[keep] for k, v in inst.items()}
        return out

    def __call__(self, video_dict, rng=None):
        records, params = self.plan(video_dict, np.random.default_rng() if rng is None else rng)
        return self.map_clip(records, params)


# -------------------------------------------------------------------------------------------------- loader
def new_data_seed():
    """A fresh 63-bit seed for the data stream, from the operating system."""
    return int.from_bytes(os.urandom(8), "little") >> 1


def check_videos(videos, gen_image_motion):
    """Raise at start-up what `sample_clip` / `GoMDatasetMapper.plan` would raise in the middle of a run, some iteration
    that happens to draw the video: a one-image video under GEN_IMAGE_MOTION, a video whose frames differ in source size."""
    for v in videos:
        if gen_image_motion and len(v["images"]) == 1:
            raise NotImplementedError("video %r has one image: INPUT.VIDEO.GEN_IMAGE_MOTION (a transform per frame, mixed-size "
                                      "batches) is not built; set INPUT.VIDEO.GEN_IMAGE_MOTION false" % (v.get("video_id"),))
        sizes = sorted(set((r["height"], r["width"]) for r in v["images"]))
        if len(sizes) != 1:
            raise ValueError("video %r: the frames of one clip must share a source size, and this video has %s"
                             % (v.get("video_id"), sizes))


class VTSTrainLoader:
    """Iterator of clips; see `build_vts_train_loader`."""

    def __init__(self, videos, mapper, seed, rank=0, world_size=1, start_iter=0, num_workers=4):
        if not (0 <= rank < world_size):
            raise ValueError("rank %r of world size %r" % (rank, world_size))
        self.videos, self.mapper = videos, mapper
        self.seed, self.rank, self.world_size = int(seed), int(rank), int(world_size)
        self.iteration = int(start_iter)
        self.num_workers = max(1, min(int(num_workers), MAX_DECODE_THREADS))
        self._pool = None
        self._pending = collections.deque()
        self._perm = (None, None)

    def position(self, i):
        """Position of iteration i in the endless stream of shuffled epochs (TrainingSampler: rank r serves positions r,
        r + world_size, ...)."""
        return i * self.world_size + self.rank

    def video_index(self, i):
        epoch, k = divmod(self.position(i), len(self.videos))
        if self._perm[0] != epoch:
            self._perm = (epoch, np.random.default_rng([0, self.seed, epoch]).permutation(len(self.videos)))
        return int(self._perm[1][k])

    def plan(self, i):
        """-> (video index, frame records, transform numbers) of iteration i: a pure function of (seed, i, rank, world_size)."""
        v = self.video_index(i)
        rng = np.random.default_rng([1, self.seed, i, self.rank])
        records, params = self.mapper.plan(self.videos[v], rng)
        return v, records, params

    def _submit(self):
        _, records, params = self.plan(self.iteration + len(self._pending))
        if isinstance(params, MotionPlan):                       # one decode serves the clip: one task, a list of frames
            self._pending.append((True, [self._pool.submit(self.mapper.map_clip, records, params)]))
        else:
            self._pending.append((False, [self._pool.submit(self.mapper.map_frame, r, params) for r in records]))

    def __iter__(self):
        return self

    def __next__(self):
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.num_workers)
        while len(self._pending) < LOOKAHEAD_CLIPS:
            self._submit()
        whole, futures = self._pending.popleft()
        clip = futures[0].result() if whole else [f.result() for f in futures]
        self.iteration += 1
        return clip

    def close(self):
        if self._pool is not None:
            for _, futures in self._pending:
                for f in futures:
                    f.cancel()
            self._pending.clear()
            self._pool.shutdown(wait=True)
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def build_vts_train_loader(cfg, mapper, seed, rank=0, world_size=1, start_iter=0, dataset_dicts=None):
    """`build_vts_train_loader` (vts_dataset_dataloader.py:27-71) -> an iterator of clips (lists of frame dicts).

    The clip of iteration i is a pure function of (seed, i, rank, world_size): epoch e's permutation of the videos is drawn
    from (seed, e); position i * world_size + rank of the endless stream picks the video; the sampling and augmentation
    draws come from a generator keyed by (seed, i, rank).  So a run resumed at `start_iter`, and a run with another number
    of decode threads, see the clips the first run saw, and ranks never share a position.

    A video the sampler would refuse (`check_videos`) is refused here, when the loader is built, not at the iteration that draws
    it; a mapper built with `image_motion` takes one-image videos (module doc-string), so videos and stills mix.
    Frames are decoded ahead, at most LOOKAHEAD_CLIPS clips, by DATALOADER.NUM_WORKERS threads (default 4, at most 16).
    `dataset_dicts`: the records of `load_video_json`; default: the one name in DATASETS.TRAIN through the split table."""
    D = data_cfg(cfg)
    if D.DATALOADER.SAMPLER_TRAIN != "TrainingSampler":
        raise NotImplementedError("DATALOADER.SAMPLER_TRAIN %r: only TrainingSampler is built" % (D.DATALOADER.SAMPLER_TRAIN,))
    if dataset_dicts is None:
        names = list((cfg.get("DATASETS") or {}).get("TRAIN") or [])
        if len(names) != 1:
            raise NotImplementedError("DATASETS.TRAIN %r: exactly one training dataset is built (several need "
                                      "MultiDatasetSampler)" % (names,))
        dataset_dicts = load_video_json(*resolve_split(names[0]))
    from .solver import solver_cfg
    batch_size = solver_cfg(cfg).IMS_PER_BATCH // world_size
    assert batch_size == 1, "SOLVER.IMS_PER_BATCH // world size must be 1 (one clip per rank), got %d" % batch_size
    videos = get_video_dataset_dicts([dataset_dicts], gen_inst_id=D.INPUT.VIDEO.GEN_IMAGE_MOTION)
    check_videos(videos, mapper.gen_image_motion and not getattr(mapper, "image_motion", False))
    return VTSTrainLoader(videos, mapper, seed, rank, world_size, start_iter, D.DATALOADER.NUM_WORKERS)
