"""Times the data side of head training at the headline clip size: 6 frames of 1280x720 (synthetic JPEGs written to a
temporary directory), TRAIN_SIZE 1280, at the scale draws 0.5, 1.0 and 2.0 (360x640 whole; 720x1280 whole; 1440x2560 of which
a 1280x1280 window is kept).  One process; per scale the two ingest paths alternate, REPEATS repeats, medians and ranges:

  host path    per clip: Pillow resize + slice + CHW float32 on the host (the mapper's `device_ingest=False` work plus the
               reference's conversion to float), then fp32 upload and the normaliser kernel (`preprocess_image`);
  device path  per clip: u8 upload and ONE launch (`preprocess_image` on `frame_u8` + `resize_hw` + `crop`).

The device path is also timed on its own (not alternating), and its launch alone on resident frames with device events.
Both start from decoded frames (decoding is common to both) and end, synchronised, with the same normalised NHWC4 tensor; the
tool checks that the two tensors are equal.  Then the loader's clips per second at 1, 4 and 16 decode threads (JPEG decoding
plus annotation work with device ingest; plus the Pillow resize with host ingest), and one `Trainer.step` (full icdar15
config, synthetic weights) on the same clip at each scale, for scale, and at the scales 0.1 (72x128, the small end of the
shipped SCALE_RANGE) and 0.37 (an odd size).

    python tools/train_data_bench.py [--repeats 7] > profiles/train_data_bench.log
"""
import argparse
import json
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
H, W, FRAMES, VIDEO_FRAMES = 720, 1280, 6, 24
SCALES = (0.5, 1.0, 2.0)
STEP_SCALES = (0.1, 0.37) + SCALES            # Trainer.step also at the small end of the shipped range (72x128) and at an odd size


def write_dataset(root):
    images, annotations = [], []
    os.makedirs(os.path.join(root, "frame", "v"), exist_ok=True)
    for t, fr in enumerate(make_clip(VIDEO_FRAMES, H, W, clip_id=1)):
        name = os.path.join("v", "%d.jpg" % (t + 1))
        Image.fromarray(fr).save(os.path.join(root, "frame", name), quality=90)
        images.append({"id": t + 1, "file_name": name, "height": H, "width": W, "video_id": 1})
        for j in range(8):                                        # eight moving boxes per frame
            x0, y0 = 60 + 140 * j + 4 * t, 80 + 60 * j + 2 * t
            xs = np.linspace(x0, x0 + 120, 4)
            bez = [float(v) for p in [(x, y0) for x in xs] + [(x, y0 + 40) for x in xs[::-1]] for v in p]
            annotations.append({"id": len(annotations) + 1, "image_id": t + 1, "category_id": 1, "iscrowd": 0, "bbox": [x0, y0, 120, 40],
                                "instance_id": j + 1, "transcription": "word%d" % j, "bezier_pts": bez})
    path = os.path.join(root, "train.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "text"}]}, f)
    return path, os.path.join(root, "frame")


def fmt(xs):
    return "%8.2f ms (%.2f .. %.2f)" % (1e3 * statistics.median(xs), 1e3 * min(xs), 1e3 * max(xs))


def ingest_paths(model, cfg, records, repeats):
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True)
    frames = [data.read_image(r["file_name"], mapper.image_format) for r in records]
    sync = torch.cuda.synchronize
    print("ingest of one clip: %d frames of %dx%d, TRAIN_SIZE 1280, %d repeats, host and device path alternating" % (FRAMES, W, H, repeats))
    for scale in SCALES:
        params = data.resize_crop_params(H, W, mapper.target_size, scale, 0.5, 0.5)
        window = data.crop_window(params, mapper.target_size)
        dev_clip = [{"frame_u8": torch.from_numpy(f), "resize_hw": params[:2], "crop": window, "flip_channels": False} for f in frames]

        def host():
            t0 = time.perf_counter()
            clip = [{"image": torch.as_tensor(np.ascontiguousarray(data.apply_image(f, params, mapper.target_size).transpose(2, 0, 1))
                                              .astype("float32"))} for f in frames]
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
        assert torch.equal(a, b), "the two paths disagree at scale %g" % scale
        hp, hu, d = [], [], []
        for _ in range(repeats):
            t_cpu, t_up, _ = host()
            hp.append(t_cpu), hu.append(t_up)
            d.append(device()[0])
        tot = [x + y for x, y in zip(hp, hu)]
        # the device path on its own, as a training run has it, and its launch alone on resident frames.  (Alternating with the
        # host path makes the model's staging key change on every call, and `_upload` then synchronises and allocates anew: the
        # likely reason the alternating figure is the larger one -- a hypothesis, not measured apart.)
        alone = [device()[0] for _ in range(repeats + 2)][2:]
        resident = torch.stack([torch.from_numpy(f) for f in frames]).to(DEV)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        launch = []
        for _ in range(repeats + 2):
            ev[0].record()
            ops.ingest_crop(resident, params[:2], window, model.pixel_mean, model.pixel_std, False)
            ev[1].record()
            ev[1].synchronize()
            launch.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        launch = launch[2:]
        out_bytes = FRAMES * window[2] * window[3] * 16
        print(" scale %.1f: resized %dx%d, window %dx%d at (%d, %d)  [the two outputs are bit-equal]" % (
            scale, params[1], params[0], window[3], window[2], window[1], window[0]))
        print("   host path    %s  = Pillow resize + slice + float %s  + fp32 upload + normalise %s" % (fmt(tot), fmt(hp), fmt(hu)))
        print("   device path  %s  = u8 upload + one launch" % fmt(d))
        print("   device path, not alternating  %s;  its launch alone on resident frames (device events) %s, %.0f MB written = %.2f TB/s" % (
            fmt(alone), fmt(launch), out_bytes / 1e6, out_bytes / statistics.median(launch) / 1e12))
        verdict = "faster beyond the spread" if max(d) < min(tot) else ("slower beyond the spread" if min(d) > max(tot) else "within the spread")
        print("   device / host = %.3f: the device path is %s" % (statistics.median(d) / statistics.median(tot), verdict))


def loader_rates(cfg, recs, clips=24):
    print("loader, clips per second over %d clips after 4 warm-up clips (JPEG decode + annotations; host ingest adds the Pillow resize):" % clips)
    for device_ingest in (True, False):
        for workers in (1, 4, 16):
            c = cfg.clone()
            c.DATALOADER = {"SAMPLER_TRAIN": "TrainingSampler", "NUM_WORKERS": workers}
            mapper = data.GoMDatasetMapper(c, True, device_ingest=device_ingest)
            rates = []
            for rep in range(3):
                with data.build_vts_train_loader(c, mapper, 5, dataset_dicts=recs) as ld:
                    for _ in range(4):
                        next(ld)
                    t0 = time.perf_counter()
                    n = sum(len(next(ld)) for _ in range(clips))
                    rates.append((clips / (time.perf_counter() - t0), n / clips))
            r = [x[0] for x in rates]
            print("  %-13s %2d threads  %7.1f clips/s (%.1f .. %.1f), %.1f frames per clip" % (
                "device ingest" if device_ingest else "host ingest", workers, statistics.median(r), min(r), max(r), rates[0][1]))


def trainer_steps(model, cfg, records):
    tr = solver.Trainer(cfg, model, None)
    mapper = data.GoMDatasetMapper(cfg, True, device_ingest=True)
    print("Trainer.step on the same clip (full icdar15 config, %d queries, synthetic weights; median of 5 after 2 warm-up steps, "
          "host-synchronised):" % cfg.MODEL.TRANSFORMER.NUM_QUERIES)
    out = {}
    for scale in STEP_SCALES:
        params = data.resize_crop_params(H, W, mapper.target_size, scale, 0.5, 0.5)
        clip = [mapper.map_frame(r, params) for r in records]
        try:
            ts = []
            for i in range(7):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                tr.step(clip)
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(time.perf_counter() - t0)
            out[scale] = statistics.median(ts)
            print("  scale %.2f (network input %dx%d): %s" % (scale, clip[0]["crop"][3], clip[0]["crop"][2], fmt(ts)))
        except (ValueError, NotImplementedError, RuntimeError, FloatingPointError) as e:
            print("  scale %.2f (network input %dx%d): REFUSED: %s: %s" % (scale, clip[0]["crop"][3], clip[0]["crop"][2], type(e).__name__, e))
            break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    cfg = setup_cfg(builtin="icdar15")
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    merge_from_list(cfg, ["SOLVER.WARMUP_ITERS", "0"])
    print("torch %s, %s" % (torch.__version__, torch.cuda.get_device_name(0)))
    with tempfile.TemporaryDirectory() as root:
        json_file, image_root = write_dataset(root)
        recs = data.load_video_json(json_file, image_root)
        from gomatching_amd.modeling import GoMatching
        model = GoMatching(cfg, synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS), device=DEV)
        ingest_paths(model, cfg, recs[:FRAMES], args.repeats)
        loader_rates(cfg, recs)
        trainer_steps(model, cfg, recs[:FRAMES])
        model.close()


if __name__ == "__main__":
    main()
