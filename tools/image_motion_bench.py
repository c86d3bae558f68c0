"""Times training from a still image (`--image-motion`, INPUT.VIDEO.GEN_IMAGE_MOTION) at the headline size: ONE 720x1280 source,
TRAIN_SIZE 1280, TRAIN_LEN 6, fixed seeds, one process, the paths alternating, medians and ranges.

  input stage   host path: T Pillow resizes + slices (the mapper's `device_ingest=False` work), then T uploads, normalise, pad
                (`preprocess_image` on the frames' `image`s); device path: one image upload + one table upload + one launch
                (`preprocess_image` on the shared `frame_u8`).  Both start from the decoded image and end, synchronised, with the
                same padded NHWC4 batch; the tool checks that the two are equal.
  launch alone  `ops.ingest_motion` on the resident image with device events (the host-side table build and the table upload
                are in front of the first event's kernel: the figure holds them), the kernel alone into a preallocated batch with
                resident tables, and a device-to-device copy of as many bytes.
  Trainer.step  on a motion clip with the detector per group of equally sized frames (`--motion-batch grouped`, the default) and
                once on the whole padded clip with per-frame valid extents (`--motion-batch whole`), beside the same step on a
                6-frame same-size video clip from the same source at scale 1.0 (the floor); the three alternate.
  groups        detector groups (distinct frame sizes) per clip over 100 planned clips.
  memory        `torch.cuda.memory_allocated` after steps 50, 100, 150 and 200 of a motion run (a new clip every step), and after
                the clip of step 50 run once more at the end.

    python tools/image_motion_bench.py [--repeats 7] > profiles/image_motion_bench.log

Launches per step, in a run of its own (tracing slows the host: no time of that run is reported):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o launches -- python tools/image_motion_bench.py --launches
    python tools/image_motion_bench.py --count-trace DIR/*/launches_kernel_trace.csv >> profiles/image_motion_bench.log

`--launches` runs two warm-up rounds and then one step of each kind between marker launches (`gom_copy_words` of MARKER_WORDS
words: a grid no other launch of the run has); `--count-trace` counts the dispatches between the markers.
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gomatching_amd import data, ops, solver  # noqa: E402
from gomatching_amd.config import merge_from_list, setup_cfg  # noqa: E402
from gomatching_amd.synth import TRAINING_CLS_BIAS, make_clip  # noqa: E402
from gomatching_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda"
H, W, FRAMES = 720, 1280, 6


def fmt(xs):
    return "%8.2f ms (%.2f .. %.2f)" % (1e3 * statistics.median(xs), 1e3 * min(xs), 1e3 * max(xs))


def record_of(root):
    os.makedirs(os.path.join(root, "frame"), exist_ok=True)
    name = os.path.join(root, "frame", "still.jpg")
    Image.fromarray(make_clip(1, H, W, clip_id=1)[0]).save(name, quality=90)
    annotations = []
    for j in range(8):
        x0, y0 = 60 + 140 * j, 80 + 60 * j
        xs = np.linspace(x0, x0 + 120, 4)
        bez = [float(v) for p in [(x, y0) for x in xs] + [(x, y0 + 40) for x in xs[::-1]] for v in p]
        annotations.append({"bbox": [x0, y0, 120, 40], "bbox_mode": "XYWH_ABS", "iscrowd": 0, "category_id": 0,
                            "instance_id": data.FIRST_GENERATED_ID + j, "annotation_id": j + 1,
                            "texts": data.encode_text("word%d" % j), **data.bezier_fields(bez)})
    return {"file_name": name, "height": H, "width": W, "image_id": 1, "video_id": -1, "annotations": annotations}


def clip_of(mapper, record, seed):
    video = {"video_id": data.FIRST_GENERATED_ID, "images": [record]}
    records, plan = mapper.plan(video, np.random.default_rng(seed))
    return mapper.map_clip(records, plan), plan


def input_stage(model, cfg, record, repeats):
    sync = torch.cuda.synchronize
    dev_mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True, image_motion=True)
    image = data.read_image(record["file_name"], dev_mapper.image_format)
    dev_clip, plan = clip_of(dev_mapper, record, 3)
    target = (dev_mapper.motion_size,) * 2
    windows = [data.crop_window(p, target) for p in plan]
    print("input stage of one motion clip: %d frames of one %dx%d image, TRAIN_SIZE %d, %d repeats, host and device path alternating"
          % (FRAMES, W, H, target[0], repeats))
    for p, w in zip(plan, windows):
        print("   frame: resized %dx%d, window %dx%d at (%d, %d)" % (p[1], p[0], w[3], w[2], w[1], w[0]))

    def host():
        t0 = time.perf_counter()
        clip = [{"image": torch.as_tensor(np.ascontiguousarray(data.apply_image(image, p, target).transpose(2, 0, 1))), "motion": True}
                for p in plan]
        t1 = time.perf_counter()
        x, _ = model.preprocess_image(clip)
        sync()
        return t1 - t0, time.perf_counter() - t1, x

    def device():
        t0 = time.perf_counter()
        x, _ = model.preprocess_image(dev_clip)
        sync()
        return time.perf_counter() - t0, x
    for _ in range(2):
        a, b = host()[2], device()[1]
    assert torch.equal(a, b), "the two paths disagree"
    hp, hu, d = [], [], []
    for _ in range(repeats):
        t_cpu, t_up, _ = host()
        hp.append(t_cpu), hu.append(t_up)
        d.append(device()[0])
    tot = [x + y for x, y in zip(hp, hu)]
    alone = [device()[0] for _ in range(repeats + 2)][2:]
    print("   host path    %s  = %d Pillow resizes + slices %s  + %d uploads + normalise + pad %s" % (fmt(tot), FRAMES, fmt(hp), FRAMES, fmt(hu)))
    print("   device path  %s  = one image upload + one table upload + one launch" % fmt(d))
    print("   device path, not alternating  %s" % fmt(alone))
    verdict = "faster beyond the spread" if max(d) < min(tot) else ("slower beyond the spread" if min(d) > max(tot) else "within the spread")
    print("   device / host = %.3f: the device path is %s  [the two outputs are bit-equal]" % (statistics.median(d) / statistics.median(tot), verdict))

    # the launch alone
    resident = torch.from_numpy(image).to(DEV)
    frames = [((p[0], p[1]), w) for p, w in zip(plan, windows)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ts = []
        for _ in range(repeats + 2):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        return ts[2:]
    op = timed(lambda: ops.ingest_motion(resident, frames, model.pixel_mean, model.pixel_std, False))
    tables, desc, (PH, PW) = ops.motion_tables(H, W, frames)
    tab = tables.to(DEV)
    out = torch.empty((FRAMES, PH, PW, 4), dtype=torch.float32, device=DEV)
    m = (ctypes.c_float * 3)(*[float(v) for v in model.pixel_mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in model.pixel_std])
    L = ops._L()
    kernel = timed(lambda: ops.check(L.gom_ingest_motion_u8_hwc3_to_nhwc4(
        ops._p(resident), H, W, ops._p(tab), tab.numel(), ops._p(desc), FRAMES, m, s, ops._p(out), PH, PW, 0, ops._stream())))
    other = torch.empty_like(out)
    copy = timed(lambda: other.copy_(out))
    nbytes = out.numel() * 4
    inside = sum(w[2] * w[3] for w in windows) * 16
    print("   launch alone on the resident image (device events): `ops.ingest_motion` with its table build and upload %s; the kernel, "
          "tables resident, %s: %.0f MB written (%.0f MB inside the windows, the rest zeros; tables %.2f MB) = %.2f TB/s; a "
          "device-to-device copy of as many bytes %s = %.2f TB/s written"
          % (fmt(op), fmt(kernel), nbytes / 1e6, inside / 1e6, tables.numel() * 4 / 1e6, nbytes / statistics.median(kernel) / 1e12,
             fmt(copy), nbytes / statistics.median(copy) / 1e12))
    return dev_clip


KINDS = ("video", "grouped", "whole")                       # the order inside a round
MARKER_WORDS = 777777                                       # `gom_copy_words` of this many words: cdiv(., 256) * 256 = 777984 threads


def step_of(tr, kind, video_clip, dev_clip):
    tr.motion_whole_batch = kind == "whole"                  # what Trainer(..., motion_whole_batch=) sets; a video step ignores it
    tr.step(video_clip if kind == "video" else dev_clip)


def video_clip_of(cfg, record):
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True)
    params = data.resize_crop_params(H, W, mapper.target_size, 1.0, 0.5, 0.5)
    return [mapper.map_frame(record, params) for _ in range(FRAMES)]


def steps(model, cfg, record, dev_clip, repeats):
    tr = solver.Trainer(cfg, model, None)
    video_clip = video_clip_of(cfg, record)
    print("Trainer.step (full icdar15 config, %d queries, synthetic weights; video / grouped / whole alternating, %d repeats after 2 "
          "warm-up rounds, host-synchronised):" % (cfg.MODEL.TRANSFORMER.NUM_QUERIES, repeats))
    ts = {k: [] for k in KINDS}
    for i in range(repeats + 2):
        for name in KINDS:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            step_of(tr, name, video_clip, dev_clip)
            torch.cuda.synchronize()
            if i >= 2:
                ts[name].append(time.perf_counter() - t0)
    tr.motion_whole_batch = False
    sizes = [fr["crop"][2:] for fr in dev_clip]
    print("   video clip, %d frames of %dx%d (one group)             %s" % (FRAMES, video_clip[0]["crop"][3], video_clip[0]["crop"][2], fmt(ts["video"])))
    print("   motion clip, grouped: %d frames in %d groups %s  %s" % (FRAMES, len(set(sizes)), sorted(set(sizes)), fmt(ts["grouped"])))
    print("   motion clip, whole: one padded batch of %d frames, per-frame valid extents  %s" % (FRAMES, fmt(ts["whole"])))
    med = {k: statistics.median(v) for k, v in ts.items()}
    print("   grouped / video = %.2f, whole / video = %.2f, whole / grouped = %.3f" % (med["grouped"] / med["video"], med["whole"] / med["video"],
                                                                                     med["whole"] / med["grouped"]))
    if max(ts["whole"]) < min(ts["grouped"]):
        print("   whole is faster than grouped beyond the spread of the %d repeats" % repeats)
    elif min(ts["whole"]) > max(ts["grouped"]):
        print("   whole is SLOWER than grouped beyond the spread of the %d repeats" % repeats)
    else:
        print("   whole and grouped are within each other's spread")
    return tr


def launches(model, cfg, record):
    """One step of each kind between marker launches, for a kernel trace (see the module docstring)."""
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True, image_motion=True)
    dev_clip, _ = clip_of(mapper, record, 3)
    video_clip = video_clip_of(cfg, record)
    tr = solver.Trainer(cfg, model, None)
    a = torch.zeros((MARKER_WORDS,), dtype=torch.int32, device=DEV)
    b = torch.empty_like(a)
    for _ in range(2):
        for name in KINDS:
            step_of(tr, name, video_clip, dev_clip)
    torch.cuda.synchronize()
    for name in KINDS:
        ops.copy_words(a, b)
        step_of(tr, name, video_clip, dev_clip)
        torch.cuda.synchronize()
    ops.copy_words(a, b)
    torch.cuda.synchronize()


def count_trace(path):
    import csv
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    grid = -(-MARKER_WORDS // 256) * 256
    marks = [i for i, r in enumerate(rows) if "copy_words_kernel" in r["Kernel_Name"] and
             int(r.get("Grid_Size") or r.get("Grid_Size_X")) == grid]
    assert len(marks) == len(KINDS) + 1, "expected %d marker launches in the trace, found %d" % (len(KINDS) + 1, len(marks))
    print("launches per Trainer.step (kernel dispatches between marker launches of a rocprofv3 --kernel-trace run, every kind of "
          "dispatch counted: the library's kernels and torch's):")
    for name, lo, hi in zip(KINDS, marks, marks[1:]):
        seg = rows[lo + 1:hi]
        ours = sum(1 for r in seg if "anonymous namespace" in r["Kernel_Name"])
        print("   %-8s %5d dispatches, %d of them the library's kernels" % (name, len(seg), ours))


def groups(cfg, record):
    mapper = data.GoMDatasetMapper(cfg, True, image_motion=True)
    target = (mapper.motion_size,) * 2
    video = {"video_id": data.FIRST_GENERATED_ID, "images": [record]}
    counts = []
    for seed in range(100):
        _, plan = mapper.plan(video, np.random.default_rng([7, seed]))
        counts.append(len({data.crop_window(p, target)[2:] for p in plan}))
    print("detector groups per clip over 100 planned clips: mean %.2f of %d frames, min %d, max %d, %d clips with one group"
          % (statistics.mean(counts), FRAMES, min(counts), max(counts), counts.count(1)))


def memory(model, cfg, record, tr):
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True, image_motion=True)
    print("memory of a motion run, a new clip every step (torch.cuda.memory_allocated, synchronised):")
    readings = {}

    def read(step, what=""):
        torch.cuda.synchronize()
        readings[step] = torch.cuda.memory_allocated()
        print("   after step %3d%s: %.2f MB allocated, %.1f MB reserved; geometry cache %d entries, crop tables %d, resample tables %d"
              % (step, what, readings[step] / 1e6, torch.cuda.memory_reserved() / 1e6, len(model.detection_transformer._geom),
                 len(ops._crop_tables), len(ops._resample_tables)))
    t0 = time.perf_counter()
    for step in range(1, 201):
        clip, _ = clip_of(mapper, record, [11, step])
        tr.step(clip)
        if step % 50 == 0:
            read(step)
    print("   200 steps in %.1f s; step 200 - step 50 = %+.2f MB" % (time.perf_counter() - t0, (readings[200] - readings[50]) / 1e6))
    # a leak grows with the number of steps; state that depends on the clip a step ran does not: the clip of step 50 once more,
    # after 200 others, shows which of the two a difference between the readings is
    clip, _ = clip_of(mapper, record, [11, 50])
    tr.step(clip)
    read(201, " (the clip of step 50 again)")
    print("   step 201 - step 50 = %+.2f MB" % ((readings[201] - readings[50]) / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", action="store_true", help="one step of each kind between marker launches, for a kernel trace")
    ap.add_argument("--count-trace", default=None, metavar="CSV", help="count the dispatches per step in the kernel trace of a --launches run")
    args = ap.parse_args()
    if args.count_trace is not None:
        return count_trace(args.count_trace)
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    merge_from_list(cfg, ["SOLVER.WARMUP_ITERS", "0"])
    assert data.data_cfg(cfg).INPUT.VIDEO.TRAIN_LEN == FRAMES
    print("torch %s, %s" % (torch.__version__, torch.cuda.get_device_name(0)))
    with tempfile.TemporaryDirectory() as root:
        record = record_of(root)
        from gomatching_amd.modeling import GoMatching
        model = GoMatching(cfg, synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS), device=DEV)
        if args.launches:
            launches(model, cfg, record)
            model.close()
            return
        dev_clip = input_stage(model, cfg, record, args.repeats)
        tr = steps(model, cfg, record, dev_clip, args.repeats)
        groups(cfg, record)
        memory(model, cfg, record, tr)
        model.close()


if __name__ == "__main__":
    main()
