"""Time drawing tracked text on one synthetic video: 1280 x 720, 44 instances per frame over 100 frames, every instance a
50-point boundary polygon around a curved text line with a `(id)TEXT` label, frames of 16-pixel colour blocks under mild noise.

The description of the chunk (polygons, boxes, colours, label bitmaps: `show._scene_of_rows`) is built once and shared.  In one
process, alternating and after a warm-up:
  host    `show.compose_host`: rasterisation and blending in numpy
  device  `show.compose_device`: upload of the frames and of the description, the fill, outline and compose launches, copy back
and, on their own, the three launches between device events with the inputs resident (10 passes per window, time per pass),
the compose launch alone against a device-to-device copy of the same frames (bytes read + written over time, both), and
Pillow's JPEG encoding (quality 95) of the 100 drawn frames on one thread and on the command's pool of 4.
Prints the median and the range of each over the rounds and whether the two paths returned the same bytes.  The reference's
visualizer (Detectron2 + matplotlib) cannot run here, so no ratio against it is claimed: the baseline is this tree's numpy
path."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gomatching_amd import show                                         # noqa: E402

H, W = 720, 1280
WORDS = ["street", "open", "coffee", "exit", "42", "market", "hotel", "sale", "bus", "north"]


def curved_polygon(rng):
    """50 points: 25 along the upper side of a bent text line, left to right, 25 back along the lower side."""
    length, thick = rng.randint(60, 260), rng.randint(10, 36)
    x0, cy = rng.randint(0, W - length), rng.randint(40, H - 40)
    amp = rng.randint(-30, 31)
    t = np.linspace(0.0, 1.0, 25)
    x = x0 + t * length
    y = cy + amp * np.sin(np.pi * t)
    top = np.stack([x, y - thick / 2], 1)
    bottom = np.stack([x[::-1], y[::-1] + thick / 2], 1)
    return np.concatenate([top, bottom]).astype(np.int64)


def video(per_frame, frames, seed):
    """-> (frames u8 [F,H,W,3], rows per frame): `per_frame` tracks that drift a little from frame to frame."""
    rng = np.random.RandomState(seed)
    base = [curved_polygon(rng) for _ in range(per_frame)]
    rows = []
    for f in range(frames):
        fr = []
        for k, c in enumerate(base):
            poly = c + rng.randint(-3, 4, size=2)
            fr.append([0] * 8 + [k + 1, WORDS[(k + f // 25) % len(WORDS)], [poly.tolist()]])
        rows.append(fr)
    coarse = np.kron(rng.randint(0, 256, (frames, H // 16, W // 16, 3)), np.ones((1, 16, 16, 1), dtype=np.int64))
    return np.clip(coarse + rng.randint(-8, 9, coarse.shape), 0, 255).astype(np.uint8), rows


def stats(ts):
    ts = sorted(ts)
    return "median %9.3f ms  (min %9.3f, max %9.3f, n = %d)" % (ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3, len(ts))


def event_times(fn, rounds, reps):
    """Seconds per call of `fn` between device events, `reps` calls per window, after one window of warm-up."""
    times = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    return times[1:]


def encode(frame):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, format="JPEG", quality=95)
    return buf.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", default="44x100")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "overlay_bench needs the GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    per_frame, frames = [int(s) for s in args.size.split("x")]
    fr, rows = video(per_frame, frames, seed=per_frame)
    scene = show._scene_of_rows(rows, 37, show.Atlas(), H, W, True)
    host = lambda: show.compose_host(fr, scene)
    device = lambda: show.compose_device(fr, scene)
    h, d = host(), device()                                       # the warm-up of both, and the comparison
    same = h.tobytes() == d.tobytes()
    times = {"host": [], "device": []}
    for _ in range(args.rounds):
        for name, fn in (("host", host), ("device", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

    dev = torch.device("cuda:0")
    src = torch.from_numpy(fr).to(dev)
    dst = torch.empty_like(src)
    arrays = show.device_arrays(scene, dev)
    launches = event_times(lambda: show.launch(src, scene, arrays, out=dst), args.rounds, 10)
    up, face, line, _ = arrays
    (_, _, _, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph, label_rgb, gwh, gwoff, gwords) = up
    from gomatching_amd import ops
    compose = event_times(lambda: ops.overlay_compose(src, face, line, boxes, woff, inst_off, inst_rgb, label_off, label_pos,
                                                      label_glyph, label_rgb, gwh, gwoff, gwords, show.A_FACE, show.A_BOX, out=dst),
                          args.rounds, 10)
    copy = event_times(lambda: dst.copy_(src), args.rounds, 10)
    moved = 2 * src.numel()                                       # every pixel read once and written once

    enc = {1: [], show.WRITE_THREADS: []}
    for _ in range(args.rounds):
        for n in enc:
            with ThreadPoolExecutor(max_workers=n) as pool:
                t0 = time.perf_counter()
                size = sum(pool.map(encode, d))
                enc[n].append(time.perf_counter() - t0)

    med = lambda ts: sorted(ts)[len(ts) // 2]
    print("%d x %d, %d instances per frame x %d frames: %d polygons of 50 points, %d labels from %d bitmaps, %d mask words per set "
          "(%.1f MiB), %d of %d pixels drawn on; host and device outputs bytewise equal: %s" % (
              W, H, per_frame, frames, scene.mset.N, len(scene.label_glyph), len(scene.glyph_wh), int(scene.mset.woff[-1]),
              int(scene.mset.woff[-1]) * 4 / 2 ** 20, int((d != fr).any(-1).sum()), frames * H * W, same))
    print("  %-28s %s" % ("host (numpy)", stats(times["host"])))
    print("  %-28s %s" % ("device (upload .. copy back)", stats(times["device"])))
    print("  %-28s %s" % ("kernels (3 launches)", stats(launches)))
    print("  %-28s %s  %.1f MB read + written: %.2f TB/s" % ("compose launch alone", stats(compose), moved / 1e6,
                                                            moved / med(compose) / 1e12))
    print("  %-28s %s  %.1f MB read + written: %.2f TB/s" % ("device-to-device copy", stats(copy), moved / 1e6,
                                                            moved / med(copy) / 1e12))
    for n in enc:
        print("  %-28s %s  (%d frames, %.1f MB of JPEG)" % ("JPEG q95, %d thread%s" % (n, "" if n == 1 else "s"), stats(enc[n]),
                                                          frames, size / 1e6))


if __name__ == "__main__":
    main()
