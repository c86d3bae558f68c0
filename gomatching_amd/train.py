"""`python -m gomatching_amd.train`: train the association head of the native model on a video dataset -- the counterpart of
the reference's train_net.py:50-211.

    python -m gomatching_amd.train (--config-file F | --builtin NAME) [--json FILE --image-root DIR] [--resume]
           [--host-ingest] [--image-motion [--motion-batch {grouped,whole}]] [--seed N] --opts MODEL.WEIGHTS W OUTPUT_DIR out ...
      -> out/model_*.pth, out/model_final.pth, out/last_checkpoint, out/metrics.json

What it keeps of the reference: `setup` (config file, then --opts; INFERENCE_TH_TEST = INFERENCE_TH_TRAIN, which `Trainer`
applies), `DATASETS.TRAIN` resolved through the split table of datasets/vts.py:216-233 (under ./datasets), the frozen
detector and the rescoring-head rule, the loop of `do_train` up to `max_iter` (SOLVER.TRAIN_ITER when >= 0), the finite
check, one metrics.json line (loss dict, total_loss, lr, data_time, time, iteration; plus grad_norm) and one
`CommonMetricPrinter`-style line every 20 iterations and at the end -- `time` is the step WITHOUT the wait for data, as
train_net.py:109-133 times it (its step timer is reset after the data arrived; Detectron2's own trainer counts the whole
iteration, so compare `time + data_time` with a metrics.json of that trainer) --, periodic checkpoints (all three with `solver.Trainer`).

Deliberate differences:
  * `--json` and `--image-root` name a dataset directly instead of a registered split;
  * the data stream is seeded (`data.build_vts_train_loader`): the seed is --seed, else `cfg.SEED` when >= 0, else drawn
    once by rank 0, shared with the other ranks and printed; it is stored in every checkpoint and `--resume` restores it, so a resumed run sees the clips the
    uninterrupted run would have seen (the reference's workers reseed from the clock);
  * frames are resized, cropped and normalised on the GPU, one launch per clip (`--host-ingest`: with Pillow on the host, the
    same bits);
  * still images (records without a video id) are refused unless `--image-motion` is given: the flag builds the mapper with
    `image_motion=True`, which turns each still into a GEN_IMAGE_MOTION clip (`data.motion_clip_params`; one image upload and
    one ingest launch per clip, the detector per group of equally sized frames).  Opt-in because the refusal is what existing
    callers rely on; `--host-ingest` combines with it.  `--motion-batch whole` runs such a clip through the detector as ONE
    padded batch with per-frame valid extents inside the kernels instead (`training.detect_for_training(whole_batch=True)`);
    `grouped` stays the default;
  * no TensorBoard writer, no `--num-gpus` / launcher: under an initialised `torch.distributed` the rank and world size go
    to the loader and only rank 0 writes metrics, but starting the ranks is the caller's business;
  * metrics are the last iteration's values, not medians over a window; the reference's silence during the first 5
    iterations after the start is not kept.
"""
import argparse
import json
import os
import sys
import time

from . import config as _config
from . import data as _data


def get_parser():
    p = argparse.ArgumentParser(
        prog="python -m gomatching_amd.train",
        description="Train the association head on an MI355X from a video dataset (json + frames); writes checkpoints and "
                    "metrics.json under OUTPUT_DIR.")
    p.add_argument("--config-file", default=None, metavar="FILE", help="path to config file")
    p.add_argument("--builtin", default=None, choices=sorted(_config.BUILTIN), metavar="NAME",
                   help="a packaged config instead of --config-file: " + ", ".join(sorted(_config.BUILTIN)))
    p.add_argument("--json", default=None, metavar="FILE", help="annotation json (default: DATASETS.TRAIN through the split table)")
    p.add_argument("--image-root", default=None, metavar="DIR", help="directory the json's file names are relative to")
    p.add_argument("--resume", action="store_true", help="continue from OUTPUT_DIR/last_checkpoint")
    p.add_argument("--host-ingest", action="store_true",
                   help="resize and crop frames with Pillow on the host (default: on the GPU, bit-exact with the host path)")
    p.add_argument("--image-motion", action="store_true",
                   help="train from still images too: a one-image video becomes a GEN_IMAGE_MOTION clip of TRAIN_LEN frames "
                        "(default: such a video is refused)")
    p.add_argument("--motion-batch", default="grouped", choices=("grouped", "whole"),
                   help="with --image-motion: the detector per group of equally sized frames (grouped, the default) or once on the "
                        "whole padded clip with per-frame valid extents (whole)")
    p.add_argument("--seed", type=int, default=None, metavar="N", help="seed of the data stream (default: cfg.SEED, else drawn)")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER,
                   help="modify config options using the command-line 'KEY VALUE' pairs")
    return p


def _distributed():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _shared_drawn_seed(rank, world_size):
    """A data seed drawn once: by rank 0, and handed to the other ranks -- the ranks deal out ONE stream of shuffled epochs,
    which they can only do from one seed."""
    box = [_data.new_data_seed() if rank == 0 else None]
    if world_size > 1:
        import torch.distributed as dist
        dist.broadcast_object_list(box, src=0)
    return int(box[0])


def _error(msg):
    sys.stderr.write("error: %s\n" % msg)
    return 2


def metric_line(m, max_iter):
    """One line in the manner of Detectron2's `CommonMetricPrinter`."""
    losses = "  ".join("%s: %.4g" % (k, v) for k, v in m.items() if "loss" in k and k != "total_loss")
    return " iter: %d/%d  total_loss: %.4g  %s  time: %.4f  data_time: %.4f  lr: %.5g  grad_norm: %.4g" % (
        m["iteration"], max_iter, m["total_loss"], losses, m["time"], m["data_time"], m["lr"], float("nan") if m["grad_norm"] is None else m["grad_norm"])


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.motion_batch == "whole" and not args.image_motion:
        return _error("--motion-batch whole needs --image-motion (video clips are one batch already)")
    if (args.config_file is None) == (args.builtin is None):
        return _error("give exactly one of --config-file and --builtin")
    if args.config_file is not None and not os.path.isfile(args.config_file):
        return _error("config file %r not found" % args.config_file)
    if len(args.opts) % 2:
        return _error("--opts takes KEY VALUE pairs")
    if (args.json is None) != (args.image_root is None):
        return _error("--json and --image-root go together")
    cfg = _config.setup_cfg(config_file=args.config_file, opts=args.opts, builtin=args.builtin)
    if args.json is not None:
        json_file, image_root = args.json, args.image_root
    else:
        names = list((cfg.get("DATASETS") or {}).get("TRAIN") or [])
        if len(names) != 1:
            return _error("DATASETS.TRAIN %r: exactly one training dataset is built (or give --json and --image-root)" % (names,))
        try:
            json_file, image_root = _data.resolve_split(names[0])
        except KeyError as e:
            return _error(e.args[0])
    if not os.path.isfile(json_file):
        return _error("annotation json %r not found" % json_file)
    if not cfg.MODEL.WEIGHTS or not os.path.isfile(cfg.MODEL.WEIGHTS):
        return _error("MODEL.WEIGHTS %r is not a file (set it with --opts MODEL.WEIGHTS PATH)" % (cfg.MODEL.WEIGHTS,))
    try:
        mapper = _data.GoMDatasetMapper(cfg, True, device_ingest=not args.host_ingest, image_motion=args.image_motion)
        if _data.data_cfg(cfg).DATALOADER.SAMPLER_TRAIN != "TrainingSampler":
            raise NotImplementedError("DATALOADER.SAMPLER_TRAIN %r: only TrainingSampler is built"
                                      % (_data.data_cfg(cfg).DATALOADER.SAMPLER_TRAIN,))
    except (NotImplementedError, ValueError) as e:
        return _error(e.args[0])
    output_dir = cfg.get("OUTPUT_DIR", "./output")
    if args.resume and not os.path.isfile(os.path.join(output_dir, "last_checkpoint")):
        return _error("--resume: no last_checkpoint under OUTPUT_DIR %r" % (output_dir,))

    dataset_dicts = _data.load_video_json(json_file, image_root)
    try:                                                         # what the sampler would refuse mid-run is refused here
        _data.check_videos(_data.get_video_dataset_dicts([dataset_dicts]), mapper.gen_image_motion and not mapper.image_motion)
    except (NotImplementedError, ValueError) as e:
        return _error(e.args[0])

    # ---- from here on the GPU is in use
    from .eval import load_weights
    from .modeling import GoMatching
    from .solver import Trainer
    rank, world_size = _distributed()
    model = GoMatching(cfg, load_weights(cfg.MODEL.WEIGHTS))
    trainer = Trainer(cfg, model, output_dir, motion_whole_batch=args.motion_batch == "whole")
    start_iter = trainer.resume() if args.resume else 0
    seed = args.seed
    if args.resume and trainer.data_seed is not None:
        if seed is not None and seed != trainer.data_seed:
            print("--seed %d ignored: the checkpoint's data seed %d continues" % (seed, trainer.data_seed))
        seed = trainer.data_seed
    cfg_seed = cfg.get("SEED", -1)
    if seed is None and cfg_seed is not None and int(cfg_seed) >= 0:
        seed = int(cfg_seed)
    if seed is None:
        seed = _shared_drawn_seed(rank, world_size)
    trainer.data_seed = int(seed)
    print("data seed %d, %d images, starting training from iteration %d" % (trainer.data_seed, len(dataset_dicts), start_iter))
    max_iter = trainer.max_iter
    os.makedirs(output_dir, exist_ok=True)
    metrics_path = os.path.join(output_dir, "metrics.json")
    loader = _data.build_vts_train_loader(cfg, mapper, trainer.data_seed, rank, world_size, start_iter, dataset_dicts=dataset_dicts)
    start_time = time.perf_counter()
    try:
        for iteration in range(start_iter, max_iter):
            t0 = time.perf_counter()
            clip = next(loader)
            t1 = time.perf_counter()
            m = trainer.step(clip)
            m.update(data_time=t1 - t0, time=time.perf_counter() - t1)
            if rank == 0 and (m["iteration"] % 20 == 0 or m["iteration"] == max_iter):
                with open(metrics_path, "a") as f:
                    f.write(json.dumps(m, sort_keys=True) + "\n")
                print(metric_line(m, max_iter))
    finally:
        loader.close()
        model.close()
    print("Total training time: %.1f s" % (time.perf_counter() - start_time))
    return 0


if __name__ == "__main__":
    sys.exit(main())
