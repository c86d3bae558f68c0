"""Time JPEG encoding of the drawn frames of `overlay_bench`'s video: 1280 x 720, 44 instances per frame over 100 frames, at
quality 95.  One process, the paths alternating, after a warm-up of each; median and range over the rounds:
  pillow x1 / x4   Pillow's `save(quality=95)` of the 100 drawn frames (host arrays) on one thread / on the command's pool of 4
  host-encode      `jpeg.encode_host` + `jpeg.files`: the rule in numpy (what --host-encode runs; `--host-rounds` of it: it is slow)
  device path      from the drawn frames RESIDENT on the GPU to the files' bytes on the host: `ops.jpeg_encode` (four launches and
                   the copy of the F + 1 offsets), the copy of the payload, `jpeg.files`
  launches         the four launches alone between device events over a workspace allocated once (transform + entropy +
                   offsets in one call, pack in the other), and a device-to-device copy of the same frames for scale
and the whole `show` command (`show.main`, in process) on a tree of that video's frames as .jpg files, with and without
--device-encode.  Prints the bytes that cross back to the host under each path, and whether device and host bytes are equal."""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gomatching_amd import jpeg, ops, show                                # noqa: E402
from overlay_bench import H, W, event_times, stats, video                # noqa: E402

QUALITY = 95


def pillow_encode(frame):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, format="JPEG", quality=QUALITY)
    return buf.tell()


def write_tree(root, fr, rows):
    """The video as a dataset directory of .jpg frames and the result json `show` reads."""
    from PIL import Image
    data = os.path.join(root, "ICDAR15_frames", "Video_1_1_1")
    os.makedirs(data)
    os.makedirs(os.path.join(root, "out", "jsons"))
    for i, f in enumerate(fr):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(os.path.join(data, "%d.jpg" % (i + 1)), quality=QUALITY)
    tracks = {str(i + 1): [{"points": r[:8], "ID": r[8], "transcription": r[9], "segmentation": r[10]} for r in rows[i]]
              for i in range(len(rows))}
    with open(os.path.join(root, "out", "jsons", "Video_1_1_1.json"), "w") as fp:
        json.dump(tracks, fp)
    return os.path.join(root, "ICDAR15_frames"), os.path.join(root, "out")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=None, help="rounds of the numpy path (default: --rounds)")
    ap.add_argument("--size", default="44x100")
    args = ap.parse_args()
    host_rounds = args.rounds if args.host_rounds is None else args.host_rounds
    assert torch.cuda.is_available(), "jpeg_encode_bench needs the GPU"
    print("device: %s" % torch.cuda.get_device_name(0))
    per_frame, frames = [int(s) for s in args.size.split("x")]
    fr, rows = video(per_frame, frames, seed=per_frame)
    scene = show._scene_of_rows(rows, 37, show.Atlas(), H, W, True)
    dev = torch.device("cuda:0")
    drawn_dev = show.compose_resident(fr, scene)
    drawn = drawn_dev.cpu().numpy()

    def device_path():
        payload, offsets = ops.jpeg_encode(drawn_dev, QUALITY, True)
        return jpeg.files(payload.cpu().numpy(), offsets.numpy(), H, W, QUALITY)

    def host_path(sel=slice(None)):
        return jpeg.files(*jpeg.encode_host(drawn[sel], QUALITY, True), H, W, QUALITY)

    def pillow_path(n):
        with ThreadPoolExecutor(max_workers=n) as pool:
            return sum(pool.map(pillow_encode, drawn))

    files_dev = device_path()                                               # warm-ups, and the comparison
    same = files_dev[:2] == host_path(slice(0, 2))
    pillow_bytes = pillow_path(show.WRITE_THREADS)
    times = {"pillow x1": [], "pillow x%d" % show.WRITE_THREADS: [], "host-encode": [], "device path": []}
    for r in range(args.rounds):
        for name, fn in (("pillow x1", lambda: pillow_path(1)), ("pillow x%d" % show.WRITE_THREADS, lambda: pillow_path(show.WRITE_THREADS)),
                         ("host-encode", host_path), ("device path", device_path)):
            if name == "host-encode" and r >= host_rounds:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            if name == "host-encode" and r == 0:
                same = same and out == files_dev

    # the launches alone, over a workspace and a payload allocated once
    L = ops._L()
    nbytes = L.gom_jpeg_workspace_bytes(frames, H, W)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    off = torch.empty((frames + 1,), dtype=torch.int64, device=dev)

    def scan():
        ops.check(L.gom_jpeg_encode_scan_u8(ops._p(drawn_dev), frames, H, W, 1, QUALITY, ops._p(ws), nbytes, ops._p(off), ops._stream()))
    scan()
    total = int(off.cpu()[frames])
    payload = torch.empty(((total + 3) // 4 * 4,), dtype=torch.uint8, device=dev)

    def pack():
        ops.check(L.gom_jpeg_encode_pack_u8(ops._p(ws), nbytes, frames, H, W, total, ops._p(payload), payload.shape[0], ops._stream()))
    pack()
    assert payload[:total].cpu().numpy().tobytes() == b"".join(f[len(jpeg.header(H, W, QUALITY)):-2] for f in files_dev)
    t_scan = event_times(scan, args.rounds, 5)
    t_pack = event_times(pack, args.rounds, 5)
    t_all = event_times(lambda: (scan(), pack()), args.rounds, 5)
    dst = torch.empty_like(drawn_dev)
    t_copy = event_times(lambda: dst.copy_(drawn_dev), args.rounds, 10)

    # the whole command
    cmd = {"show": [], "show --device-encode": []}
    with tempfile.TemporaryDirectory() as root:
        data, out = write_tree(root, fr, rows)
        base = ["--input", data, "--results", out, "--voc-size", "37"]
        for r in range(args.rounds + 1):                                    # round 0 warms both up
            for name, extra in (("show", []), ("show --device-encode", ["--device-encode"])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert show.main(base + ["--output", os.path.join(root, name.replace(" ", "_"))] + extra) == 0
                torch.cuda.synchronize()
                if r:
                    cmd[name].append(time.perf_counter() - t0)

    med = lambda ts: sorted(ts)[len(ts) // 2]
    src_bytes = drawn_dev.numel()
    print("%d x %d, %d instances per frame x %d frames at quality %d; device and host files bytewise equal: %s" % (
        W, H, per_frame, frames, QUALITY, same))
    print("  bytes to the host: %.1f MB of frames without --device-encode, %.1f MB of entropy-coded data + %d offsets with it "
          "(files: %.1f MB ours, %.1f MB Pillow's); workspace %.0f MB" % (
              src_bytes / 1e6, total / 1e6, frames + 1, sum(len(f) for f in files_dev) / 1e6, pillow_bytes / 1e6, nbytes / 1e6))
    for name in times:
        if times[name]:
            print("  %-28s %s" % (name, stats(times[name])))
    print("  %-28s %s" % ("launches: transform..offsets", stats(t_scan)))
    print("  %-28s %s" % ("launches: pack", stats(t_pack)))
    print("  %-28s %s  %.1f MB of frames read: %.3f TB/s" % ("launches: all four", stats(t_all), src_bytes / 1e6,
                                                           src_bytes / med(t_all) / 1e12))
    print("  %-28s %s  %.1f MB read (and as much written): %.3f TB/s" % ("device-to-device copy", stats(t_copy), src_bytes / 1e6,
                                                                        src_bytes / med(t_copy) / 1e12))
    for name in cmd:
        print("  %-28s %s" % (name, stats(cmd[name])))


if __name__ == "__main__":
    main()
