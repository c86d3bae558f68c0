"""`python -m gomatching_amd.eval`: run the spotter over a dataset directory and write the result files the reference's
offline evaluation protocols consume -- the counterpart of the reference's measured entry point (eval.py:212-383)
with `--show` as the one optional drawing step.

    python -m gomatching_amd.eval --config-file FILE --input DIR --output OUT [--show] --opts MODEL.WEIGHTS W
      -> OUT/preds/res_<video>.xml, OUT/preds/res_<video>.txt, OUT/jsons/<video>.json
      -> with --show also OUT/results/<video>/<frame file>: every frame with its tracked text drawn on it

What it keeps of the reference: `setup_cfg` (with the ASSO_THRESH_TEST override of :220), the data type taken from the
input path (DSText / ICDAR15 / BOVText / OTHER), video directories one level deeper for DSText and BOVText (:290-295),
frames sorted by the integer stem of the file name (:309), 100-frame chunks, skipping of videos whose XML exists and of
the damaged `Cls1_Livestreaming_video40` (:275-277, :316), the ICDAR15 XML naming (:372-378), the per-track
transcription files (:381) and the wording of the timing lines.

Deliberate differences:
  * the "already written" check compares the XML stem `results.result_names` returns; the reference compares the raw
    video name, which never matches an ICDAR15 stem ('Video_35_2_3' is written as res_video_35.xml), so it never
    resumes on ICDAR15;
  * no `--cpu` (there is no CPU path), no `--webcam` (no capture library is installed).  What a camera needs is there, though:
    `--online [--push N]` runs every video as a stream through `gomatching_amd.online.OnlineSpotter` -- frames are decoded one
    push (N frames, default 4 detector steps, rounded up to whole steps) ahead instead of the whole video at once, rows leave
    the model as soon as their tracks have settled (at most 20 frames after the frame was tracked with the shipped configs) and
    go straight to `results.VideoResultWriter`, and host and device memory do not grow with the length of the video.  The
    three files per video are byte-identical to a run without the flag, which issues the launches it always issued.
    `--online` builds rows on the GPU only and collects no pixels on the host: with `--host-rows`, or with `--show` alone, the
    command exits with status 2 (`python -m gomatching_amd.show` draws from OUT/jsons afterwards, as it does for resumed
    runs).  `--online --show --device-decode` draws: the frames are born in device memory, the session keeps the pending ones
    in a pixel ring beside its rows (`OnlineSpotter(draw=...)`), draws the frames that settle with one gather-compose launch
    per push and every drawn chunk is written as `show.draw_video` writes it -- the pictures of a run without `--online`, byte
    for byte; under `--device-encode` only compressed bytes come back.  Not with `--host-draw` (status 2);
  * `--show` draws with csrc/overlay.hip by an integer rule instead of matplotlib (`gomatching_amd.show`: colours by track
    id, Pillow's glyphs, no antialiasing); without it the command does what it did before the flag existed, launch for launch.
    A resumed run skips finished videos, pictures included: `python -m gomatching_amd.show` draws them from OUT/jsons.
    With `--show`, `--device-encode` / `--host-encode` [`--jpeg-quality N`] write the JPEG frames with the project's own
    baseline encoder (csrc/jpeg.hip on the GPU / the same rule in numpy) instead of Pillow, as the show command does;
  * `--lexicon FILE|DIR [--lexicon-pairs FILE] [--lexicon-max-dist N] [--lexicon-unmatched keep|drop]` runs
    `gomatching_amd.lexicon.correct_results` over OUT after the videos are written (those of earlier, resumed runs included)
    and writes OUT/lexicon/{jsons,preds}; without it the command issues the launches and writes the bytes it always did;
  * `--device-lexicon` (with `--lexicon`, `--device-write` and `--device-vote`; without all three status 2, before anything is
    created; without a GPU status 1) corrects the rows where they lie instead (csrc/lexicon_rows.hip; the rule is in
    include/gomatching_hip.h, `gom_lexicon_rows_*`): every call -- a 100-frame chunk offline, a push with `--online` -- writes the
    original text under OUT/ as ever and the corrected text under OUT/lexicon/{jsons,preds}, the corrected txt voted over the
    corrected words when the video closes, byte-identical to the end-of-run host step, which then skips those videos and still
    corrects the ones this run did not write (a resumed run); the run prints both counts and the kept, accepted and dropped
    rows of the device path (`distinct` and `changed` are not computed there).  A display form above 175 bytes in the JSON or
    XML file or 100 bytes in the txt file is refused with status 2 before a model is built or anything is created
    (`device_lexicons`): those stay with the host step; a transcription above 64 code points ends the run with status 2 too.  Without
    the flag the command issues the launches and writes the bytes it always did;
  * `--decode-walk {auto,segments,chunks}` (with `--device-decode`; default auto) picks the decoder's entropy walk: a wavefront per
    restart segment, or a lane per chunk of a segment for files without restart markers; the pixels are the same, and the run prints
    how many segments went which way.  Without `--device-decode` status 2;
  * `--device-write` formats the text of jsons/<video>.json and preds/res_<video>.xml on the GPU (csrc/result_text.hip; the rule
    is in include/gomatching_hip.h, `gom_result_text_*`), from the rows where `ops.result_rows` / `result_rows_gather` left them:
    only the words `results.finish_points` needs come back, the eight rectangle points go up, and the text comes back as bytes,
    at most 100 frames per call offline and per gather with `--online`.  The files are byte-identical (always UTF-8; the host
    writer opens the XML in the locale's encoding).  With `--show` the row lists are still built, for the drawing only; `--lexicon`
    reads the files afterwards; goes with `--device-decode`.  With `--host-rows` status 2; without a GPU status 1 (a choice, not a
    fall-back).  Without the flag the command issues the launches and writes the bytes it always did;
  * `--device-vote` (with `--device-write`; without it status 2, without a GPU status 1) votes preds/res_<video>.txt on the GPU as
    well (csrc/track_vote.hip; the rule is in include/gomatching_hip.h, `gom_track_vote_*`): every call's rows leave a 112-byte
    record each in a device log that lives as long as the video, and when the video's other two files are closed the log is
    ordered by track, voted and formatted, offline and with `--online`.  The end-of-run host step skips those files and still
    parses the XMLs this run did not write (a resumed run); the run prints both counts.  The bytes are the same.  Without the
    flag the command issues the launches and writes the bytes it always did, `--device-write` alone included;
  * `--device-decode` reads file bytes on the pool and decodes baseline JPEG frames on the GPU (csrc/jpeg_decode.hip, byte-equal
    to Pillow's decode, so the result files do not change), per 100-frame chunk offline and per push with `--online`: host
    memory holds bytes, device memory one chunk of pixels.  Files with another extension, files `jpeg.parse` refuses and files
    whose status word is set go through Pillow per file; the run prints the count of every route.  Not with `--host-ingest`
    (status 2); without a GPU status 1.  With `--show` the drawing step decodes the video a second time, chunk by chunk, on the
    GPU as well (`show.DecodedChunks`) and draws every chunk where it lies: tens of milliseconds per chunk, against holding the
    video's pixels in either memory.  Those decodes are counted apart and printed on a line of their own ("drawing decode:");
    the "device decode:" line counts the spotting decode only.  The pictures do not change: the decoder is byte-equal to Pillow;
  * frames are decoded with Pillow (`convert("RGB")`, reversed to the BGR order `read_image(format="BGR")` yields).
    OpenCV is not available here, so the parity of the decoded pixels with `cv2.imread` (JPEG decoders differ in their
    IDCT and chroma upsampling) is UNPINNED, as is the parity of `results.min_area_rect` with `cv2.minAreaRect`.
"""
import argparse
import os
import shutil
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import config as _config
from . import results as _results

DAMAGED_VIDEOS = ("Cls1_Livestreaming_video40",)          # eval.py:316 "filter bovtext damaged video"
DECODE_THREADS = 4                                        # a small fixed pool that decodes frames ahead (never sized by the host)


def get_parser(drawing=False):
    """The spotting options; drawing=True, what the command itself parses with, adds the drawing step's (--show, --font,
    --host-draw).  A caller that builds on the default parser gets a run that draws nothing and an error for --show."""
    p = argparse.ArgumentParser(
        prog="python -m gomatching_amd.eval",
        description="Video text spotting over a dataset directory on an MI355X; writes preds/res_*.xml, preds/res_*.txt and "
                    "jsons/*.json under --output" + (
                        ", and with --show results/<video>/<frame file> with the tracked text drawn on every frame.  There is no "
                        "--cpu or --webcam: the package has no CPU path." if drawing else
                        ".  There is no --cpu or --webcam (the package has no CPU path); --show belongs to the command's own "
                        "parser, get_parser(drawing=True)."))
    p.add_argument("--config-file", default=None, metavar="FILE", help="path to config file")
    p.add_argument("--builtin", default=None, choices=sorted(_config.BUILTIN), metavar="NAME",
                   help="a packaged config instead of --config-file: " + ", ".join(sorted(_config.BUILTIN)))
    p.add_argument("--input", required=True, metavar="DIR",
                   help="dataset directory: one directory of frames per video (one level deeper for DSText / BOVText)")
    p.add_argument("--output", required=True, metavar="DIR", help="directory for preds/ and jsons/")
    p.add_argument("--frames-per-step", type=int, default=8, metavar="N", help="frames per detector step (default 8)")
    p.add_argument("--host-ingest", action="store_true",
                   help="resize and normalise frames on the host (default: on the GPU, bit-exact with the host path)")
    p.add_argument("--host-rows", action="store_true",
                   help="build result rows per frame on the host (default: one kernel launch and one copy per clip)")
    p.add_argument("--device-decode", action="store_true",
                   help="decode baseline JPEG frames on the GPU (the same bytes as Pillow's): the pool reads file bytes, host "
                        "memory holds no pixels; any other file goes through Pillow, per file (not with --host-ingest)")
    p.add_argument("--decode-walk", choices=("auto", "segments", "chunks"), default=None,
                   help="with --device-decode: the entropy walk -- a wavefront per restart segment, a lane per chunk of a segment "
                        "(files without restart markers), or auto (default): chunks where a call's segments are long; the same "
                        "pixels either way")
    p.add_argument("--device-write", action="store_true",
                   help="format the text of jsons/*.json and preds/res_*.xml on the GPU, from the rows where they lie "
                        "(csrc/result_text.hip); the same bytes (not with --host-rows)")
    p.add_argument("--device-vote", action="store_true",
                   help="with --device-write: vote every video's track transcriptions (preds/res_*.txt) on the GPU as well, from "
                        "the same rows (csrc/track_vote.hip); the same bytes")
    p.add_argument("--online", action="store_true",
                   help="run every video as a stream: frames are decoded one push ahead, rows are written as their tracks "
                        "settle, memory does not grow with the video; the files are the same (not with --host-rows; with --show "
                        "only together with --device-decode)")
    p.add_argument("--push", type=int, default=None, metavar="N",
                   help="with --online: frames per push, rounded up to whole detector steps (default 4 steps)")
    if drawing:
        p.add_argument("--show", action="store_true",
                       help="write every frame with its tracked text drawn on it to results/<video>/ (polygons in the colour "
                            "of their track, (id)TEXT labels)")
        p.add_argument("--font", default=None, metavar="FILE",
                       help="with --show: a TrueType font for the labels (default: Pillow's)")
        p.add_argument("--host-draw", action="store_true",
                       help="with --show: draw in numpy on the host (default: on the GPU, the same bytes)")
        from . import show as _show
        _show.add_encode_arguments(p)                      # with --show: --device-encode, --host-encode, --jpeg-quality
    p.add_argument("--lexicon", default=None, metavar="FILE|DIR",
                   help="after the videos are written, also write OUT/lexicon/ with every transcription snapped to the nearest "
                        "word of this vocabulary (gomatching_amd.lexicon; a directory holds per-video <video>.txt files)")
    p.add_argument("--lexicon-pairs", default=None, metavar="FILE", help="with --lexicon FILE: its pair list")
    p.add_argument("--lexicon-max-dist", type=int, default=1, metavar="N",
                   help="with --lexicon: accept a word at an edit distance of at most N (default 1)")
    p.add_argument("--lexicon-unmatched", choices=("keep", "drop"), default="keep",
                   help="with --lexicon: keep a transcription without an accepted word (default) or remove its row")
    p.add_argument("--device-lexicon", action="store_true",
                   help="with --lexicon, --device-write and --device-vote: correct the rows on the GPU, in the call that formats "
                        "them (csrc/lexicon_rows.hip), offline and with --online; OUT/lexicon/ gets the same bytes, nothing is "
                        "parsed or dumped at the end.  The figures are the kept, accepted and dropped rows: `distinct` and "
                        "`changed` are not computed on the device path")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER,
                   help="modify config options using the command-line 'KEY VALUE' pairs")
    return p


def data_type_of(input_dir):
    for name in ("DSText", "ICDAR15", "BOVText"):
        if name in input_dir:
            return name
    return "OTHER"


def list_videos(input_dir, done=()):
    """-> (data type, [(video name, video directory)]) in listing order; videos whose XML stem is in `done` and the damaged
    BOVText video are left out."""
    data_type = data_type_of(input_dir)
    dirs = []
    for video in sorted(os.listdir(input_dir)):
        path = os.path.join(input_dir, video)
        if data_type in ("DSText", "BOVText"):
            dirs.extend(os.path.join(path, v) for v in sorted(os.listdir(path)))
        else:
            dirs.append(path)
    out = []
    for d in dirs:
        name = os.path.basename(d).split(".")[0]
        if name in DAMAGED_VIDEOS or _results.result_names(name, data_type)[0] in done:
            continue
        out.append((name, d))
    return data_type, out


def written_videos(xml_dir):
    """XML stems already present under preds/ (eval.py:275-277)."""
    if not os.path.isdir(xml_dir):
        return set()
    return set(f[len("res_"):-len(".xml")] for f in os.listdir(xml_dir) if f.startswith("res_") and f.endswith(".xml"))


def frame_paths(video_dir):
    """Frame files of one video, sorted by the integer stem of the file name (2.jpg before 10.jpg)."""
    return sorted((os.path.join(video_dir, f) for f in os.listdir(video_dir)),
                  key=lambda p: int(os.path.basename(p).split(".")[0]))


def read_frame(path):
    """HxWx3 uint8 in BGR order, as `read_image(path, format="BGR")`."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


DECODE_ROUTES = ("device", "refused", "flagged", "other")
DECODE_WALK_ROUTES = ("chunks", "serial")                      # segments the chunk walk finished / walked by one lane


def decode_frames(paths, blobs, counts, device, walk="segments"):
    """`--device-decode`: the files' bytes -> one CUDA u8 [H,W,3] tensor per frame, in BGR order as `read_frame` yields.
    `.jpg` / `.jpeg` files that `jpeg.parse` accepts are decoded on the GPU, one `ops.jpeg_decode` call per geometry (a
    video's frames share one); a file with another extension ("other"), one the parser refuses ("refused") and one whose
    status word comes back set ("flagged") go through `read_frame`, per file, and are uploaded beside the others.  `counts`
    is incremented per route.  `walk`: jpeg.decode_device's ("auto" resolves per call); the segments that went through the
    chunk walk and through the serial one are counted under DECODE_WALK_ROUTES ("serial": every segment of a call that took
    the segment walk, and the segments the chunk walk marked -- it is no count of damaged segments)."""
    import torch
    from . import jpeg as _jpeg
    from . import ops
    out = [None] * len(paths)
    groups = {}
    for i, (path, blob) in enumerate(zip(paths, blobs)):
        if os.path.splitext(path)[1].lower() not in (".jpg", ".jpeg"):
            counts["other"] += 1
            continue
        info = _jpeg.parse(blob)
        if isinstance(info, _jpeg.Refusal):
            counts["refused"] += 1
            continue
        groups.setdefault(info.key, []).append((i, info))
    for items in groups.values():
        plan = _jpeg.plan([blobs[i] for i, _ in items], [info for _, info in items])
        nseg = int(plan.desc.shape[0])
        if _jpeg.resolve_walk(walk, plan) == "chunks":
            pixels, status, seg_info = ops.jpeg_decode(plan, True, device, walk="chunks", return_info=True)
            by_chunks = int((seg_info[:, 0] == 0).sum().item())
        else:
            pixels, status = ops.jpeg_decode(plan, True, device)
            by_chunks = 0
        counts["chunks"] = counts.get("chunks", 0) + by_chunks
        counts["serial"] = counts.get("serial", 0) + nseg - by_chunks
        status = status.cpu().numpy()
        for j, (i, _) in enumerate(items):
            if status[j] == 0:
                out[i] = pixels[j]
                counts["device"] += 1
            else:
                counts["flagged"] += 1
    for i, path in enumerate(paths):
        if out[i] is None:                                 # Pillow raises or decodes exactly as without the flag
            out[i] = torch.from_numpy(read_frame(path)).to(device)
    return out


def spot_video_device_decode(spotter, pool, paths, time_cost, counts, device, batch=100, walk="segments"):
    """`results.spot_video` for `--device-decode`: the pool reads the bytes of one chunk ahead, the chunk's frames are decoded
    into device memory and go to the predictor as they are.  Host memory holds file bytes only, device memory one chunk of
    pixels.  -> (per-frame results, seconds inside the timed window, seconds reading and decoding)."""
    chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]
    instances, id_count, seconds, read = [], 0, 0.0, 0.0
    ahead = [pool.submit(read_bytes, p) for p in chunks[0]]
    for batch_id, chunk in enumerate(chunks):
        t0 = time.time()
        blobs = [f.result() for f in ahead]
        ahead = [pool.submit(read_bytes, p) for p in chunks[batch_id + 1]] if batch_id + 1 < len(chunks) else []
        frames = decode_frames(chunk, blobs, counts, device, walk)
        del blobs
        read += time.time() - t0
        instances, id_count, dt = spotter(frames, instances, batch_id, id_count, batch_id == len(chunks) - 1, time_cost,
                                          return_time=True)
        del frames
        seconds += dt
        time_cost["total_time"] += dt
    return instances, seconds, read


def device_lexicons(lexicon, pairs, input_dir, done=()):
    """`--device-lexicon`: the Lexicon (`--lexicon FILE`) or {video: Lexicon} (`--lexicon DIR`) of the videos this run will spot,
    every one with its display tables built -- on the host, before a model is built or anything is uploaded or created.  A
    missing per-video lexicon, a word without a pair and a display form above the device path's limits (175 bytes in the JSON
    or XML file, 100 in the txt file) raise `lexicon.LexiconError` here: status 2."""
    from . import lexicon as _lexicon
    data_type, videos = list_videos(input_dir, done=done)
    lexicons = _lexicon.load_lexicons(lexicon, pairs, [_results.result_names(v, data_type)[1] for v, d in videos if os.listdir(d)])
    for lex in ([lexicons] if isinstance(lexicons, _lexicon.Lexicon) else lexicons.values()):
        _lexicon.checked_display_tables(lex)
    return lexicons


def load_weights(path):
    """-> canonical state dict, or None when `path` is empty or no file."""
    if not path or not os.path.isfile(path):
        return None
    import torch
    from .weights import normalize_state_dict
    return normalize_state_dict(torch.load(path, map_location="cpu"))


def spot_video_online(cfg, model, decoder, pool, paths, video_name, data_type, args, time_cost, counts=None, fix=None, draw=None):
    """One video through `online.OnlineSpotter`: the pool decodes one push ahead, rows go to the incremental writer as they
    settle.  -> seconds reading / inside the timed window / building rows and writing, and the session's wait figures.
    draw = (atlas, encode, quality) (`--online --show`, with `--device-decode`): the session draws the frames that settle from
    its ring of pending frames, and every drawn chunk is written to OUT/results/<video>/<frame file> through the functions
    `show.draw_video` uses -- `show._write_encoded` under --device-encode (only compressed bytes come back) / --host-encode,
    `show.write_frame` otherwise: the pictures of a run without --online; "draw" = seconds encoding and writing them."""
    from .online import OnlineSpotter
    step = model.frames_per_step
    push = args.push if args.push is not None else 4 * step
    push = (push + step - 1) // step * step
    session = OnlineSpotter(cfg, model, decoder, device_ingest=not args.host_ingest, time_cost=time_cost,
                            device_text=args.device_write, device_vote=args.device_vote, device_lexicon=fix,
                            draw=draw[0] if draw is not None else None)
    drawing = [0.0]

    def write_drawn():
        if draw is None:
            return
        from . import show as _show
        t0 = time.time()
        for first, drawn in session.take_drawn():
            targets = [os.path.join(save_dir, os.path.basename(p)) for p in paths[first:first + int(drawn.shape[0])]]
            try:
                if draw[1] is not None:
                    _show._write_encoded(drawn if draw[1] == "device" else drawn.cpu().numpy(), targets, pool, draw[1], draw[2])
                else:
                    list(pool.map(_show.write_frame, drawn.cpu().numpy(), targets))
            except _show.ShowError as e:
                raise _show.ShowError("video %s: %s" % (video_name, e))
        drawing[0] += time.time() - t0
    if draw is not None:
        save_dir = os.path.join(args.output, "results", video_name)
        os.makedirs(save_dir, exist_ok=True)
    add = (lambda item: writer.add_text(*item[:4])) if args.device_write else (lambda item: writer.add(*item))
    writer = _results.VideoResultWriter(video_name, data_type, args.output)
    fixed = _results.VideoResultWriter(video_name, data_type, os.path.join(args.output, "lexicon")) if fix is not None else None
    if fixed is not None:                                   # --device-lexicon: an item carries the corrected text as well
        add = lambda item: (writer.add_text(*item[:4]), fixed.add_text(item[0], item[1], item[4], item[5]))
    read, write = 0.0, 0.0
    chunks = [paths[i:i + push] for i in range(0, len(paths), push)]
    reader = read_bytes if counts is not None else read_frame      # --device-decode: bytes ahead, pixels made on the GPU
    try:
        ahead = [pool.submit(reader, p) for p in chunks[0]]
        for c in range(len(chunks)):
            t0 = time.time()
            frames = [f.result() for f in ahead]
            ahead = [pool.submit(reader, p) for p in chunks[c + 1]] if c + 1 < len(chunks) else []
            if counts is not None:
                frames = decode_frames(chunks[c], frames, counts, model.device, args.decode_walk)
            read += time.time() - t0
            settled = session.push(frames)
            del frames
            t0 = time.time()
            for item in settled:
                add(item)
            write += time.time() - t0
            write_drawn()
        settled = session.close()
        write_drawn()
        t0 = time.time()
        for item in settled:
            add(item)
        assert writer.frames == len(paths), (writer.frames, len(paths))
        writer.close(session.track_txt)                     # (None without --device-vote: no txt is written here)
        if fixed is not None:
            fixed.close(session.lexicon_txt)
        write += time.time() - t0
    except BaseException:
        writer.abort()
        if fixed is not None:
            fixed.abort()
        raise
    time_cost["total_time"] += session.seconds
    return {"read": read, "window": session.seconds, "rows": session.rows_seconds + write, "max_wait": session.max_wait,
            "bound": session.latency_bound, "launches": session.gather_launches, "draw": drawing[0]}


def main(argv=None):
    """The command.  A `lexicon.LexiconError` from anywhere in the run -- the device path raises it inside the video loop for a
    transcription above the length limit, as the host step does at the end -- ends it with a message and status 2; the
    writers of the video at hand have dropped their unfinished files by then."""
    from . import lexicon as _lexicon
    from . import show as _show
    try:
        return run(argv)
    except _lexicon.LexiconError as e:
        sys.stderr.write("error: lexicon: %s\n" % e)
        return 2
    except _show.ShowError as e:                            # frames the drawing step cannot draw (a clip of mixed sizes)
        sys.stderr.write("error: %s\n" % e)
        return 2


def run(argv=None):
    args = get_parser(drawing=True).parse_args(argv)
    if args.online and ((args.show and not args.device_decode) or args.host_rows):
        sys.stderr.write("error: --online builds rows on the GPU and collects no pixels on the host: it does not take --host-rows, "
                         "and it takes --show only together with --device-decode, which leaves the frames in device memory "
                         "(python -m gomatching_amd.show draws from OUT/jsons afterwards)\n")
        return 2
    if args.online and args.show and args.host_draw:
        sys.stderr.write("error: --online --show draws the frames where they lie on the GPU: it does not go with --host-draw\n")
        return 2
    encode, quality = None, 95
    if getattr(args, "device_encode", False) or getattr(args, "host_encode", False) or getattr(args, "jpeg_quality", None) is not None:
        if not args.show:
            sys.stderr.write("error: --device-encode, --host-encode and --jpeg-quality go with --show\n")
            return 2
        from . import show as _show
        encode, quality, status, message = _show.encode_choice(args)
        if status:
            sys.stderr.write("error: %s\n" % message)
            return status
    if args.push is not None and (not args.online or args.push < 1):
        sys.stderr.write("error: --push N (N >= 1) goes with --online\n")
        return 2
    if args.decode_walk is not None and not args.device_decode:
        sys.stderr.write("error: --decode-walk goes with --device-decode\n")
        return 2
    if args.device_decode and args.decode_walk is None:
        args.decode_walk = "auto"
    if args.device_decode and args.host_ingest:
        sys.stderr.write("error: --device-decode leaves the frames in device memory: it does not go with --host-ingest\n")
        return 2
    if args.device_decode:
        import torch
        if not torch.cuda.is_available():
            sys.stderr.write("error: --device-decode needs a GPU: the decoder runs in csrc/jpeg_decode.hip\n")
            return 1
    if args.device_write and args.host_rows:
        sys.stderr.write("error: --device-write formats the rows where they lie on the GPU: it does not go with --host-rows\n")
        return 2
    if args.device_vote and not args.device_write:
        sys.stderr.write("error: --device-vote votes over the rows --device-write leaves on the GPU: it goes with --device-write\n")
        return 2
    if args.device_lexicon and not (args.lexicon is not None and args.device_write and args.device_vote):
        sys.stderr.write("error: --device-lexicon corrects the rows --device-write and --device-vote leave on the GPU by the "
                         "vocabulary of --lexicon: it goes with all three\n")
        return 2
    if args.device_write:
        import torch
        if not torch.cuda.is_available():
            sys.stderr.write("error: --device-write needs a GPU: the text is formatted in csrc/result_text.hip\n" if not args.device_vote
                             else "error: --device-write --device-vote need a GPU: the text is formatted in csrc/result_text.hip, "
                                  "the tracks are voted in csrc/track_vote.hip\n")
            return 1
    if (args.config_file is None) == (args.builtin is None):
        sys.stderr.write("error: give exactly one of --config-file and --builtin\n")
        return 2
    if args.config_file is not None and not os.path.isfile(args.config_file):
        sys.stderr.write("error: config file %r not found\n" % args.config_file)
        return 2
    if len(args.opts) % 2:
        sys.stderr.write("error: --opts takes KEY VALUE pairs\n")
        return 2
    if not os.path.isdir(args.input):
        sys.stderr.write("error: input directory %r not found\n" % args.input)
        return 2
    if args.lexicon is None and (args.lexicon_pairs is not None or args.lexicon_max_dist != 1 or args.lexicon_unmatched != "keep"):
        sys.stderr.write("error: --lexicon-pairs, --lexicon-max-dist and --lexicon-unmatched go with --lexicon\n")
        return 2
    if args.lexicon is not None and (not os.path.exists(args.lexicon) or args.lexicon_max_dist < 0 or (
            args.lexicon_pairs is not None and not os.path.isfile(args.lexicon_pairs))):
        sys.stderr.write("error: --lexicon %r / --lexicon-pairs %r not found, or a negative --lexicon-max-dist\n"
                         % (args.lexicon, args.lexicon_pairs))
        return 2
    if args.device_lexicon:                                 # the limits of the device path, before anything is built or created
        from . import lexicon as _lexicon
        try:
            lexicons = device_lexicons(args.lexicon, args.lexicon_pairs, args.input,
                                       done=written_videos(os.path.join(args.output, "preds")))
        except _lexicon.LexiconError as e:
            sys.stderr.write("error: lexicon: %s\n" % e)
            return 2
    cfg = _config.setup_cfg(config_file=args.config_file, opts=args.opts, builtin=args.builtin)
    state_dict = load_weights(cfg.MODEL.WEIGHTS)
    if state_dict is None:
        sys.stderr.write("error: MODEL.WEIGHTS %r is not a file (set it with --opts MODEL.WEIGHTS PATH)\n"
                         % (cfg.MODEL.WEIGHTS,))
        return 2

    xml_dir, json_dir = os.path.join(args.output, "preds"), os.path.join(args.output, "jsons")
    os.makedirs(xml_dir, exist_ok=True)
    os.makedirs(json_dir, exist_ok=True)
    config_file = args.config_file or _config.BUILTIN[args.builtin]
    shutil.copy(config_file, args.output)
    data_type, videos = list_videos(args.input, done=written_videos(xml_dir))

    from .predictor import GoMBatchPredictor, TextDecoder, new_time_cost
    time_cost = new_time_cost()
    if videos:                                              # a resumed run with nothing left builds no model
        from .modeling import GoMatching
        model = GoMatching(cfg, state_dict, frames_per_step=args.frames_per_step)
        spotter = GoMBatchPredictor(cfg, model, device_ingest=not args.host_ingest)
        decoder = TextDecoder(cfg.MODEL.TRANSFORMER.VOC_SIZE, cfg.MODEL.TRANSFORMER.CUSTOM_DICT)
    total_frame, read_seconds, rows_seconds, draw_seconds = 0, 0.0, 0.0, 0.0
    routes = {k: 0 for k in DECODE_ROUTES} if args.device_decode else None
    draw_routes = {k: 0 for k in DECODE_ROUTES}             # --show --device-decode: the decodes made for drawing, counted apart
    voted = []                                              # --device-vote: the XMLs whose txt the GPU wrote in this run
    corrected, fix_rows = [], [0, 0, 0]                     # --device-lexicon: the videos corrected on the GPU; kept, accepted, dropped

    def row_correction(video_name):                         # (per-video lexicons: one DeviceLexicon per video)
        if not args.device_lexicon:
            return None
        lex = lexicons if isinstance(lexicons, _lexicon.Lexicon) else lexicons[_results.result_names(video_name, data_type)[1]]
        return _lexicon.RowCorrection(_lexicon.DeviceLexicon.of(lex, decoder, model.device), args.lexicon_max_dist,
                                      args.lexicon_unmatched, video=video_name)

    def corrected_video(video_name, fix):
        if fix is not None:
            corrected.append(_results.result_names(video_name, data_type)[1])
            for k, v in enumerate((fix.rows, fix.accepted, fix.dropped)):
                fix_rows[k] += v
    if args.show:
        from . import show as _show
        atlas = _show.Atlas(args.font)
    with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
        for video_name, video_dir in videos:
            print("processing {}...".format(video_name))
            t0 = time.time()
            paths = frame_paths(video_dir)
            if args.online:
                if not paths:
                    continue
                fix = row_correction(video_name)
                stats = spot_video_online(cfg, model, decoder, pool, paths, video_name, data_type, args, time_cost, routes, fix,
                                          draw=(atlas, encode, quality) if args.show else None)
                draw_seconds += stats["draw"]
                corrected_video(video_name, fix)
                if args.device_vote:
                    voted.append("res_%s.xml" % _results.result_names(video_name, data_type)[0])
                read_seconds += stats["read"]
                rows_seconds += stats["rows"]
                total_frame += len(paths)
                print("Video: ", video_name, "per_img_time: ", stats["window"] / len(paths), ", FPS: ",
                      len(paths) / stats["window"])
                print("online: largest wait ", stats["max_wait"], " frames (bound ", stats["bound"], "), gather launches ",
                      stats["launches"])
                continue
            if routes is not None:
                if not paths:
                    continue
                preds, per_video_time, read = spot_video_device_decode(spotter, pool, paths, time_cost, routes, model.device,
                                                                       walk=args.decode_walk)
                read_seconds += read
                frames = paths                              # (counted below; the pixels are gone)
            else:
                frames = list(pool.map(read_frame, paths))
                read_seconds += time.time() - t0
                if not frames:
                    continue
                preds, per_video_time = _results.spot_video(spotter, frames, time_cost)
            total_frame += len(frames)
            t0 = time.time()
            fix = row_correction(video_name)
            annotation = _results.write_video(preds, video_name, data_type, args.output, decoder,
                                              device_rows=not args.host_rows, device_text=args.device_write, rows=args.show,
                                              device_vote=args.device_vote, lexicon=fix)
            corrected_video(video_name, fix)
            if args.device_vote:
                voted.append("res_%s.xml" % _results.result_names(video_name, data_type)[0])
            rows_seconds += time.time() - t0
            if args.show:
                t0 = time.time()
                source = frames
                if routes is not None:                      # decoded on the GPU a second time, chunk by chunk, and drawn there
                    source = _show.DecodedChunks(paths, pool, draw_routes, model.device, args.decode_walk)
                _show.draw_video(source, annotation, paths, video_name, args.output, cfg.MODEL.TRANSFORMER.VOC_SIZE, pool, atlas,
                                 host=args.host_draw, encode=encode, quality=quality)
                draw_seconds += time.time() - t0
            print("Video: ", video_name, "per_img_time: ", per_video_time / len(frames), ", FPS: ",
                  len(frames) / per_video_time)
    t0 = time.time()
    if args.device_vote:                                    # XMLs this run did not write (a resumed run) stay with the host
        by_host = [n for n in os.listdir(xml_dir) if ".txt" not in n and "ipynb" not in n and n not in voted]
        _results.write_track_transcriptions(xml_dir, skip=voted)
        print("track transcriptions: ", len(voted), " txt files voted on the GPU, ", len(by_host), " by the host from their XML")
    else:
        _results.write_track_transcriptions(xml_dir)
    rows_seconds += time.time() - t0
    if total_frame:
        print("total_time: ", time_cost["total_time"], ", per_video_time: ", time_cost["total_time"] / len(videos),
              ", per_img_time: ", time_cost["total_time"] / total_frame, ", FPS: ", total_frame / time_cost["total_time"])
    print(time_cost)
    print("host seconds outside the timed window: reading frames ", read_seconds, ", building rows and writing files ",
          rows_seconds, ", videos processed: ", len(videos))
    if routes is not None:
        print("device decode: ", routes["device"], " files decoded on the GPU; through Pillow: ", routes["other"],
              " with another extension, ", routes["refused"], " refused by the parser, ", routes["flagged"], " with a status word set")
        print("device decode walk (--decode-walk ", args.decode_walk, "): ", routes.get("chunks", 0), " segments by the chunk walk, ",
              routes.get("serial", 0), " by the serial walk (those of calls that took the segment walk, and those the chunk walk marked)")
    if args.show and routes is not None:                    # the frames drawn: decoded a second time offline, the pushes' own online
        _show.print_draw_routes(routes if args.online else draw_routes, args.decode_walk, shared=args.online)
    if args.show:
        print("host seconds drawing and encoding frames: ", draw_seconds)
    if args.lexicon is not None:                            # every video under OUT, those of earlier (resumed) runs included
        from . import lexicon as _lexicon
        t0 = time.time()
        try:
            figures = _lexicon.correct_results(args.output, None, args.lexicon, args.lexicon_pairs, args.lexicon_max_dist,
                                               args.lexicon_unmatched, skip=corrected)
        except _lexicon.LexiconError as e:
            sys.stderr.write("error: lexicon: %s\n" % e)
            return 2
        if args.device_lexicon:
            print("device lexicon: ", len(corrected), " videos corrected on the GPU (", fix_rows[0], " kept rows, ", fix_rows[1],
                  " accepted, ", fix_rows[2], " dropped), ", figures["videos"], " by the host from their json")
        print("lexicon: ", figures["rows"], " rows, ", figures["distinct"], " distinct strings matched, ", figures["changed"],
              " changed, ", figures["dropped"], " dropped -> ", figures["output"], ", seconds: ", time.time() - t0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
