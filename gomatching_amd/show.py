"""`python -m gomatching_amd.show`: draw tracked text on the frames of a dataset from the result files `gomatching_amd.eval`
wrote -- the counterpart of the reference's `eval.py --show` (eval.py:364-369, text_track_visualizer.py), without a model.

    python -m gomatching_amd.show --input DIR --results OUT [--output DIR] [--font FILE] [--host-draw]
                                  [--device-encode | --host-encode] [--jpeg-quality N]
                                  [--device-decode [--decode-walk {auto,segments,chunks}]]
                                  [--device-read] [--voc-size N | --config-file F | --builtin NAME]
      -> DIR/results/<video name>/<basename of the source frame>   (DIR defaults to OUT)

Drawing is a pure function of the frames and the result rows `[x1..y4, id, text, [polygon]]` (what `results.frame_lines` /
`clip_lines` build and `jsons/<video>.json` stores), so `eval --show` and this command draw the same bytes.  Per instance of a
frame, in row order: the polygon's face blended at `A_FACE` / 255 in the colour of its track and its outline in that colour,
opaque; then, above every polygon, per instance a `(id)TEXT` label: a white box blended at `A_BOX` / 255 with the text in a
readable variant of the track colour.  The pixels are the integer rule of include/gomatching_hip.h
(`gom_overlay_compose_u8`): csrc/overlay.hip on the GPU, `compose_host` in numpy (`--host-draw`), byte for byte the same.

What it keeps of the reference: translucent face at alpha 0.5 and an outline per polygon, label text `(id)TEXT` upper-cased for
the 37-character vocabulary (text_track_visualizer.py:139-144), the label colour rule of `draw_text` (:231-232), the white
label box at alpha 0.8, labels above all polygons (zorder 10), the font size `max(sqrt(H W) // 70, 10)` (:98-100), the label
anchored with its top-left corner at the midpoint of the text's centre line (:146-148), `results/<video>/<frame file name>`
(eval.py:269, 321, 368).

Deliberate differences:
  * `track_color` is a pure function of the track id (a fixed palette of 500 colours indexed by id % 500); the reference draws
    random colours and hands them out by first appearance, so a redrawn or resumed video would change colours;
  * `label_anchor` takes the centre line from the 50-point result polygon (c_i = (P[i] + P[n-1-i]) / 2); the reference walks the
    float `ctrl_points`, which the result files do not carry;
  * `font_px` is used as a pixel size; matplotlib's point-to-pixel scale is not reproduced, and the label box is padded by one
    pixel (the reference's `pad: 0.7` is in points).
UNPINNED against the reference by construction: antialiasing (there is none here), matplotlib's stroke width and fonts (label
bitmaps come from Pillow: `ImageFont.truetype(--font)` or `ImageFont.load_default`, `getmask(text, mode="1")`; characters the
font lacks are Pillow's business) and the encoder of `cv2.imwrite` (frames are written with Pillow, JPEG at quality 95).
Not built: `--webcam`, video-file input, `ColorMode.IMAGE_BW`.

Writing.  By default Pillow encodes every drawn frame on a pool of four threads.  Two opt-in flags write the JPEG frames (source
extension .jpg / .jpeg) with the project's own baseline encoder instead -- the integer rule of include/gomatching_hip.h
(`gom_jpeg_encode_*`): the same sampling and quantisation tables as Pillow's files, a restart interval per MCU row, not
libjpeg's bytes:
  --device-encode   csrc/jpeg.hip: the drawn frames stay on the GPU, `ops.jpeg_encode` codes the chunk, the F + 1 offsets and
                    one copy of exactly the compressed bytes come back and the pool only writes them.  Not with --host-draw
                    (status 2); without a GPU status 1.  A choice, not a fall-back.
  --host-encode     `jpeg.encode_host`, the same rule in numpy: the same files.  With --host-draw the command needs no GPU.
  --jpeg-quality N  1 .. 100, default 95; only with one of the two.
Frames of any other extension go through Pillow as before, and with neither flag nothing changes.

Reading.  By default a pool of four threads decodes the whole video through Pillow into host arrays, which are uploaded chunk
by chunk.  One opt-in flag keeps the pixels off the host:
  --device-decode   the pool reads file BYTES, one chunk (100 frames) ahead; `eval.decode_frames` makes the chunk's pixels in
                    device memory (csrc/jpeg_decode.hip, byte-equal to Pillow; files of another extension, files the parser
                    refuses and flagged files go through Pillow, per file, as in `eval`), the chunk is drawn IN PLACE and goes
                    to the writers as ever.  Nothing is uploaded, and no more than one chunk of pixels is ever held; with
                    --device-encode a frame enters the GPU as entropy bytes and leaves it as entropy bytes.  The run prints the
                    route counts.  Not with --host-draw (status 2); without a GPU status 1.
  --decode-walk W   with --device-decode: the decoder's entropy walk, as in `eval` (default auto); alone status 2.
  --device-read     every jsons/<video>.json goes to the GPU as bytes and is parsed there (csrc/result_parse.hip; the rule is
                    `gom_result_parse_*` in include/gomatching_hip.h: exactly the text json.dumps(indent=4,
                    ensure_ascii=False) writes for a result file); each chunk's contours, boxes, word offsets and colours are
                    made from the parsed rows where they lie (`ops.scene_polygons`), about 430 bytes per instance come back
                    for the labels, which stay host work (`label_anchors`, Pillow's bitmaps).  Any other text -- another
                    indent, escapes json.dumps would not write, several contours -- is refused by the parser and read by
                    json.load, per file; the run prints how many files went each way and why.  The same pictures, byte for
                    byte.  Not with --host-draw (status 2); without a GPU status 1.  A choice, not a fall-back.
The same drawing functions serve frames that already lie in device memory elsewhere: `draw_chunk_resident` / `compose_resident`
take a CUDA u8 [F,H,W,3] tensor and draw it where it lies, `draw_gather_resident` draws frames that wait in a ring through
one `gom_overlay_compose_gather_u8` launch (`online.OnlineSpotter(draw=...)`, `eval --online --show --device-decode`), and
`draw_video` takes a function that yields the video chunk by chunk (`DecodedChunks`; `eval --show --device-decode`).  The
frames of a video must share one size: a chunk of mixed sizes ends the run with "the frames of a clip must share one size".
"""
import argparse
import colorsys
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import score_json as _sj
from .score import ScoreError

PALETTE_SIZE = 500
A_FACE = 128                                               # alpha 0.5 of draw_polygon, in 255ths
A_BOX = 204                                                # alpha 0.8 of the label's bbox
CHUNK = 100                                                # frames per fill / outline / compose call
WRITE_THREADS = 4                                          # a small fixed pool that encodes frames (never sized by the host)


class ShowError(Exception):
    """Input the command cannot draw; the message names the video."""


# ------------------------------------------------------------------------------------------ colours, text, geometry
def _palette():
    """Colour i: hue = frac(i * 0.618033988749895) (golden-ratio steps keep neighbouring ids apart), saturation
    (0.55, 0.75, 0.95)[i % 3], value (1.0, 0.85)[(i // 3) % 2], `colorsys.hsv_to_rgb`, each channel int(c * 255 + 0.5)."""
    out = np.zeros((PALETTE_SIZE, 3), dtype=np.uint8)
    for i in range(PALETTE_SIZE):
        rgb = colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, (0.55, 0.75, 0.95)[i % 3], (1.0, 0.85)[(i // 3) % 2])
        out[i] = [int(c * 255 + 0.5) for c in rgb]
    return out


PALETTE = _palette()


def track_color(track_id):
    """(r, g, b) in 0..255 of a track: PALETTE[track_id % 500]."""
    return tuple(int(v) for v in PALETTE[int(track_id) % PALETTE_SIZE])


def text_color(rgb):
    """`draw_text`'s readable variant of a colour (text_track_visualizer.py:231-232): every channel at least 0.2, the largest
    at least 0.8; channels back to 0..255 as int(c * 255 + 0.5)."""
    c = [max(int(v) / 255.0, 0.2) for v in rgb]
    top = max(range(3), key=lambda i: (c[i], -i))          # np.argmax: the first of equal maxima
    c[top] = max(0.8, c[top])
    return tuple(int(v * 255 + 0.5) for v in c)


def label_text(track_id, text, voc_size):
    """"(id)TEXT", upper-cased for the 37-character vocabulary (text_track_visualizer.py:139-144)."""
    text = str(text)
    if int(voc_size) == 37:
        text = text.upper()
    return "({}){}".format(int(track_id), text)


def font_px(H, W):
    """`_default_font_size` (text_track_visualizer.py:98-100), used as a pixel size."""
    return max(int(math.sqrt(int(H) * int(W))) // 70, 10)


def label_anchor(polygon):
    """(x, y) int of a label's top-left corner: the point at half the arc length of the centre line c_i = (P[i] + P[n-1-i]) / 2,
    i < n / 2 (what `LineString(c).interpolate(0.5, normalized=True)` returns), truncated toward zero."""
    P = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    n = len(P)
    if n == 0:
        return 0, 0
    half = (n + 1) // 2
    c = (P[:half] + P[::-1][:half]) / 2.0
    seg = np.hypot(*(c[1:] - c[:-1]).T) if half > 1 else np.zeros(0)
    total = float(seg.sum())
    pt = c[0]
    if total > 0.0:
        target, walked = total / 2.0, 0.0
        for i, d in enumerate(seg.tolist()):
            if d > 0.0 and walked + d >= target:
                pt = c[i] + (target - walked) / d * (c[i + 1] - c[i])
                break
            walked += d
        else:
            pt = c[-1]
    return int(pt[0]), int(pt[1])


def label_anchors(poly_xy, poly_off):
    """`label_anchor` of many polygons at once: poly_xy int [P,2], poly_off int [N+1] (polygon k = poly_xy[poly_off[k] :
    poly_off[k+1]]) -> int64 [N,2], bit for bit what `label_anchor` gives for each.  Polygons of one vertex count are taken
    together, a row each: every step is the scalar function's own expression over rows -- np.hypot per element, the sum of a
    row's lengths by the same reduction over the same count (numpy reduces a contiguous row as it reduces a vector of that
    length), the walk as a running sum along the row (sequential additions, as the loop makes them)."""
    xy = np.asarray(poly_xy, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(poly_off, dtype=np.int64).reshape(-1)
    N = len(off) - 1
    out = np.zeros((N, 2), dtype=np.int64)
    counts = off[1:] - off[:-1]
    for n in np.unique(counts).tolist():
        if n == 0:
            continue
        ks = np.nonzero(counts == n)[0]
        P = xy[off[ks][:, None] + np.arange(n)[None, :]]     # [G,n,2]
        half = (n + 1) // 2
        c = (P[:, :half] + P[:, ::-1][:, :half]) / 2.0
        pt = c[:, 0].copy()
        if half > 1:
            d = c[:, 1:] - c[:, :-1]
            seg = np.ascontiguousarray(np.hypot(d[:, :, 0], d[:, :, 1]))     # [G,half-1]
            total = seg.sum(axis=1)
            target = total / 2.0
            after = np.cumsum(seg, axis=1)                    # walked + d at every step
            before = np.concatenate([np.zeros((len(ks), 1)), after[:, :-1]], axis=1)
            hit = (seg > 0.0) & (after >= target[:, None])
            first = hit.argmax(axis=1)
            rows = np.arange(len(ks))
            w, dd = before[rows, first], seg[rows, first]
            with np.errstate(divide="ignore", invalid="ignore"):
                on = c[rows, first] + ((target - w) / dd)[:, None] * (c[rows, first + 1] - c[rows, first])
            walked = np.where(hit.any(axis=1)[:, None], on, c[:, -1])
            pt = np.where((total > 0.0)[:, None], walked, pt)
        out[ks] = pt.astype(np.int64)                         # (truncation toward zero, as int() does)
    return out


# ------------------------------------------------------------------------------------------ label bitmaps
def pack_bitmap(bits):
    """bool [h, w] -> uint32 [h, (w + 31) // 32], bit b of word j of a row = column 32 j + b."""
    bits = np.asarray(bits, dtype=bool)
    h, w = bits.shape
    rw = (w + 31) // 32
    padded = np.zeros((h, 32 * rw), dtype=bool)
    padded[:, :w] = bits
    if h == 0 or rw == 0:
        return np.zeros((h, rw), dtype=np.uint32)
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(h, rw)


def unpack_bitmap(words, w):
    """The inverse of `pack_bitmap`: uint32 [h, rw] -> bool [h, w]."""
    words = np.ascontiguousarray(words, dtype="<u4")
    if words.size == 0:
        return np.zeros((words.shape[0], w), dtype=bool)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)[:, :w]


class Atlas:
    """Label bitmaps, rendered once per (string, pixel size) -- a track's label repeats over its frames -- and packed for
    `gom_overlay_compose_u8`: glyph_wh int32 [G,2], glyph_woff int64 [G+1], glyph_words uint32."""

    def __init__(self, font=None):
        self.font_file = font
        self._fonts, self._index = {}, {}
        self.wh, self.rows = [], []

    def _font(self, px):
        if px not in self._fonts:
            from PIL import ImageFont
            self._fonts[px] = ImageFont.truetype(self.font_file, px) if self.font_file else ImageFont.load_default(px)
        return self._fonts[px]

    def render(self, text, px):
        """bool [h + 2, w + 2]: Pillow's 1-bit mask of the string, padded by one pixel on every side."""
        mask = self._font(px).getmask(text, mode="1")
        w, h = mask.size
        out = np.zeros((h + 2, w + 2), dtype=bool)
        if w and h:
            out[1:-1, 1:-1] = np.frombuffer(bytes(mask), dtype=np.uint8).reshape(h, w) != 0
        return out

    def add(self, bits):
        """A bitmap of the caller's -> its index."""
        bits = np.asarray(bits, dtype=bool)
        self.wh.append((bits.shape[1], bits.shape[0]))
        self.rows.append(pack_bitmap(bits))
        return len(self.wh) - 1

    def index(self, text, px):
        key = (text, px)
        if key not in self._index:
            self._index[key] = self.add(self.render(text, px))
        return self._index[key]

    def arrays(self, indices=None):
        """(glyph_wh, glyph_woff, glyph_words) of the whole atlas, or of the bitmaps `indices` names, in that order."""
        indices = range(len(self.rows)) if indices is None else [int(i) for i in indices]
        rows = [self.rows[i] for i in indices]
        wh = np.asarray([self.wh[i] for i in indices], dtype=np.int32).reshape(-1, 2)
        woff = np.zeros(len(rows) + 1, dtype=np.int64)
        woff[1:] = np.cumsum([r.size for r in rows])
        words = np.concatenate([r.reshape(-1) for r in rows]) if rows else np.zeros(0, dtype=np.uint32)
        return wh, woff, words.astype(np.uint32)


# ------------------------------------------------------------------------------------------ a chunk, described
class Scene:
    """What one compose call draws over F frames of H x W, as host arrays: `mset` (`score_json.MaskSet`: contours, boxes, word
    offsets of the N instances), inst_off int32 [F+1], inst_rgb u8 [N,3], label_off int32 [F+1], label_pos int32 [L,2],
    label_glyph int32 [L], label_rgb u8 [L,3] and the atlas arrays."""

    def __init__(self, polys, colors, labels, atlas, H, W):
        """polys: per frame a list of int [n,2] vertex arrays; colors: per frame a list of u8 triples (the frames' channel
        order); labels: per frame a list of (x0, y0, atlas index, u8 triple); atlas: `Atlas.arrays()`."""
        self.H, self.W, self.F = int(H), int(W), len(polys)
        self.mset = _sj.MaskSet([("poly", [p]) for fr in polys for p in fr], H, W)
        self.inst_off = np.concatenate([[0], np.cumsum([len(fr) for fr in polys])]).astype(np.int32)
        self.inst_rgb = np.asarray([c for fr in colors for c in fr], dtype=np.uint8).reshape(-1, 3)
        self.label_off = np.concatenate([[0], np.cumsum([len(fr) for fr in labels])]).astype(np.int32)
        flat = [l for fr in labels for l in fr]
        self.label_pos = np.asarray([(l[0], l[1]) for l in flat], dtype=np.int32).reshape(-1, 2)
        self.label_glyph = np.asarray([l[2] for l in flat], dtype=np.int32).reshape(-1)
        self.label_rgb = np.asarray([l[3] for l in flat], dtype=np.uint8).reshape(-1, 3)
        self.glyph_wh, self.glyph_woff, self.glyph_words = atlas
        assert len(self.inst_rgb) == self.mset.N and len(colors) == self.F and len(labels) == self.F


def _blend(p, c, a):
    return (p * (255 - a) + c * a + 127) // 255


def compose_host(frames, scene, a_face=A_FACE, a_box=A_BOX):
    """The rule of `gom_overlay_compose_u8` in numpy integers: u8 [F,H,W,3] -> a new u8 [F,H,W,3]."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    F, H, W, _ = out.shape
    ms = scene.mset
    assert (F, H, W) == (scene.F, scene.H, scene.W)
    for f in range(F):
        for k in range(int(scene.inst_off[f]), int(scene.inst_off[f + 1])):
            y0, y1, wx0, wx1 = (int(v) for v in ms.boxes[k])
            if y1 <= y0 or wx1 <= wx0:
                continue
            x0, x1 = 32 * wx0, min(32 * wx1, W)
            face = unpack_bitmap(_sj.fill_polygon_rows(ms.contours(k), ms.boxes[k], W), x1 - x0)[..., None]
            line = unpack_bitmap(_sj.fill_polygon_rows(ms.contours(k), ms.boxes[k], W, fill=False), x1 - x0)[..., None]
            v = out[f, y0:y1, x0:x1].astype(np.int32)
            c = scene.inst_rgb[k].astype(np.int32)
            out[f, y0:y1, x0:x1] = np.where(line, c, np.where(face, _blend(v, c, a_face), v))
        for k in range(int(scene.label_off[f]), int(scene.label_off[f + 1])):
            g = int(scene.label_glyph[k])
            x0, y0 = (int(v) for v in scene.label_pos[k])
            w, h = (int(v) for v in scene.glyph_wh[g])
            xa, xb, ya, yb = max(x0, 0), min(x0 + w, W), max(y0, 0), min(y0 + h, H)
            if xa >= xb or ya >= yb:
                continue
            rw = (w + 31) // 32
            o = int(scene.glyph_woff[g])
            bits = unpack_bitmap(scene.glyph_words[o:o + h * rw].reshape(h, rw), w)[ya - y0:yb - y0, xa - x0:xb - x0, None]
            v = out[f, ya:yb, xa:xb].astype(np.int32)
            out[f, ya:yb, xa:xb] = np.where(bits, scene.label_rgb[k].astype(np.int32), _blend(v, 255, a_box))
    return out


def _upload(arrays, dev):
    """Host arrays -> device tensors of the same dtypes through ONE copy: the arrays laid end to end, each 16-byte aligned."""
    import torch
    offs, size = [], 0
    for a in arrays:
        offs.append(size)
        size += (a.nbytes + 15) // 16 * 16
    blob = np.zeros(max(size, 16), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        blob[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(blob).to(dev)
    dtypes = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8,
              np.dtype(np.uint32): torch.int32}
    return [t[o:o + a.nbytes].view(dtypes[a.dtype]).reshape(a.shape) for a, o in zip(arrays, offs)]


def device_arrays(scene, dev):
    """The scene on the device (one upload) plus its two empty word buffers, in the argument order of `launch`."""
    import torch
    ms = scene.mset
    up = _upload([ms.points.astype(np.int32), ms.coff.astype(np.int32), ms.mcoff.astype(np.int32), ms.boxes.astype(np.int32),
                  ms.woff.astype(np.int64), scene.inst_off, scene.inst_rgb, scene.label_off, scene.label_pos, scene.label_glyph,
                  scene.label_rgb, scene.glyph_wh.astype(np.int32), scene.glyph_woff.astype(np.int64),
                  scene.glyph_words.astype(np.uint32)], dev)
    nwords = int(ms.woff[-1])
    face = torch.empty((nwords,), dtype=torch.int32, device=dev)
    line = torch.empty((nwords,), dtype=torch.int32, device=dev)
    area = torch.empty((ms.N,), dtype=torch.int32, device=dev)
    return up, face, line, area


def launch(frames_dev, scene, arrays, a_face=A_FACE, a_box=A_BOX, out=None, slots=None):
    """The three launches of a chunk over resident inputs: fill, outline, compose (in place unless `out` is given).  With
    `slots` (int32 [F], CUDA) `frames_dev` is a ring that is only read and frame f is drawn from frames_dev[slots[f]] into a
    dense tensor (`out`, default a new one): the gather form of the compose launch, still one launch."""
    from . import ops
    (points, coff, mcoff, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph, label_rgb, gwh, gwoff,
     gwords), face, line, area = arrays
    ops.mask_fill_polygons(points, coff, mcoff, boxes, woff, scene.H, scene.W, face, area)
    ops.mask_outline_polygons(points, coff, mcoff, boxes, woff, scene.H, scene.W, line)
    if slots is not None:
        return ops.overlay_compose(frames_dev, face, line, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph,
                                   label_rgb, gwh, gwoff, gwords, a_face, a_box, out=out, slots=slots)
    return ops.overlay_compose(frames_dev, face, line, boxes, woff, inst_off, inst_rgb, label_off, label_pos, label_glyph,
                               label_rgb, gwh, gwoff, gwords, a_face, a_box, out=frames_dev if out is None else out)


def is_resident(frames):
    """Whether `frames` is a CUDA tensor: frames that already lie in device memory (decoded there, or a session's ring)."""
    if isinstance(frames, (list, tuple, np.ndarray)):
        return False
    import torch
    return isinstance(frames, torch.Tensor) and frames.is_cuda


def _resident_frames(frames):
    import torch
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("resident frames must be a contiguous CUDA u8 [F,H,W,3] tensor")
    return frames


def compose_resident(frames, scene, a_face=A_FACE, a_box=A_BOX):
    """`compose_host` through csrc/overlay.hip, the drawn frames LEFT on the device: one upload of the frames and one of the
    description, the fill, outline and compose launches.  -> a CUDA u8 tensor [F,H,W,3].  Frames that are a CUDA u8
    [F,H,W,3] tensor already are used where they lie -- no upload -- and drawn IN PLACE: the result is that tensor."""
    import torch
    if is_resident(frames):
        fr = _resident_frames(frames)
        assert tuple(fr.shape[:3]) == (scene.F, scene.H, scene.W)
        with torch.cuda.device(fr.device):
            return launch(fr, scene, device_arrays(scene, fr.device), a_face, a_box)
    if not torch.cuda.is_available():
        raise ShowError("no GPU: drawing runs in csrc/overlay.hip (use --host-draw for the numpy path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    fr = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).to(dev)
    return launch(fr, scene, device_arrays(scene, dev), a_face, a_box)


def compose_gather_resident(ring, slots, scene, a_face=A_FACE, a_box=A_BOX):
    """`compose_resident` for frames that lie in a ring: `ring` a CUDA u8 [cap,H,W,3] tensor that is only read, `slots` the
    ring slot of each of the scene's frames (a sequence of ints; a slot may repeat).  One upload of the description and of
    the slot table, the fill and outline launches and ONE gather-compose launch.  -> a new dense CUDA u8 tensor [F,H,W,3]."""
    import torch
    ring = _resident_frames(ring)
    slots = np.asarray(slots, dtype=np.int32).reshape(-1)
    if len(slots) != scene.F or tuple(ring.shape[1:3]) != (scene.H, scene.W):
        raise ValueError("%d slots for a scene of %d frames, or a ring of another frame size" % (len(slots), scene.F))
    if len(slots) and (slots.min() < 0 or slots.max() >= ring.shape[0]):
        raise ValueError("slots must lie in [0, %d), the ring's frames" % ring.shape[0])
    with torch.cuda.device(ring.device):
        return launch(ring, scene, device_arrays(scene, ring.device), a_face, a_box,
                      slots=torch.from_numpy(slots).to(ring.device))


def compose_device(frames, scene, a_face=A_FACE, a_box=A_BOX):
    """`compose_resident` and one copy back."""
    return compose_resident(frames, scene, a_face, a_box).cpu().numpy()


# ------------------------------------------------------------------------------------------ rows -> pictures
def _scene_of_rows(rows_per_frame, voc_size, atlas, H, W, bgr):
    px = font_px(H, W)
    polys, colors, labels = [], [], []
    for rows in rows_per_frame:
        p, c, l = [], [], []
        for row in rows:
            if len(row) < 11 or not row[10]:
                raise ShowError("a result row without a segmentation cannot be drawn")
            poly = np.asarray(row[10][0], dtype=np.int64).reshape(-1, 2)
            rgb = track_color(row[8])
            ink = text_color(rgb)
            x, y = label_anchor(poly)
            p.append(poly)
            c.append(rgb[::-1] if bgr else rgb)
            l.append((x, y, atlas.index(label_text(row[8], row[9], voc_size), px), ink[::-1] if bgr else ink))
        polys.append(p)
        colors.append(c)
        labels.append(l)
    used = sorted(set(l[2] for fr in labels for l in fr))     # the chunk's own bitmaps, re-indexed
    local = {g: i for i, g in enumerate(used)}
    labels = [[(x, y, local[g], ink) for x, y, g, ink in fr] for fr in labels]
    try:
        return Scene(polys, colors, labels, atlas.arrays(used), H, W)
    except ScoreError as e:
        raise ShowError(str(e))


def _chunk_scene(frames_u8, rows_per_frame, voc_size, atlas, bgr):
    part = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames_u8]), dtype=np.uint8)
    if part.ndim != 4 or part.shape[3] != 3:
        raise ValueError("frames must be u8 [F,H,W,3]")
    return part, _scene_of_rows(rows_per_frame, voc_size, atlas, part.shape[1], part.shape[2], bgr)


class _Dims:
    """What `launch` reads of a scene whose arrays were made on the device."""

    def __init__(self, F, H, W):
        self.F, self.H, self.W = int(F), int(H), int(W)


INK = np.asarray([text_color(track_color(i)) for i in range(PALETTE_SIZE)], dtype=np.uint8)     # a label's colour, by id % 500
_palette_dev = {}


def _device_palette(dev):
    """PALETTE on `dev`, uploaded once."""
    import torch
    if dev not in _palette_dev:
        _palette_dev[dev] = torch.from_numpy(PALETTE.copy()).to(dev)
    return _palette_dev[dev]


class ParsedScenes:
    """The scenes of one video whose rows `results.parse_json_device` read (`show --device-read`): the polygons stay on the
    device, where `ops.scene_polygons` makes each chunk's contour offsets, boxes, word offsets and colours from them; the labels
    are host work, done here once per video from the compact arrays that came back -- the anchors (`label_anchors`), the
    colours (`INK[id % 500]`) -- and per frame size the atlas indices, rendered once per distinct (id, transcription)."""

    def __init__(self, parsed, voc_size, atlas, bgr=True):
        self.parsed, self.voc_size, self.atlas, self.bgr = parsed, voc_size, atlas, bool(bgr)
        self.anchors = label_anchors(parsed.poly_xy, parsed.poly_off).astype(np.int32)
        ink = INK[np.mod(parsed.ids, PALETTE_SIZE)]          # (numpy's mod is Python's %: non-negative)
        self.label_rgb = np.ascontiguousarray(ink[:, ::-1] if self.bgr else ink)
        self.kept = (np.diff(parsed.poly_off) > 0).astype(np.int64)
        self._glyphs = {}

    def glyphs(self, px, i0, i1):
        """The atlas index of the labels of rows i0 .. i1 - 1 at pixel size px: int32 [i1 - i0].  A label is rendered when its
        row is first asked for, in row order -- the order in which `_scene_of_rows` meets the labels of the same chunks."""
        if px not in self._glyphs:
            self._glyphs[px] = ({}, np.full(self.parsed.N, -1, dtype=np.int32))
        seen, out = self._glyphs[px]
        todo = np.nonzero(out[i0:i1] < 0)[0] + i0
        if len(todo):
            ids, texts = self.parsed.ids[todo].tolist(), self.parsed.texts
            for k, track in zip(todo.tolist(), ids):
                key = (track, texts[k])
                g = seen.get(key)
                if g is None:
                    g = seen[key] = self.atlas.index(label_text(track, key[1], self.voc_size), px)
                out[k] = g
        return out[i0:i1]

    def chunk(self, f0, f1, H, W, dev):
        """Frames f0 .. f1 - 1 at H x W -> (what `launch` takes as its scene, its `arrays`): two launches, one upload of the
        label arrays and ONE synchronising read (the chunk's word count and status: the bit rows are sized by the first)."""
        import torch
        from . import ops
        p = self.parsed
        if H < 1 or W < 1 or H * W > 2 ** 31 - 1:
            raise ShowError("image size %d x %d is not supported" % (H, W))
        i0, i1 = int(p.frame_rows[f0]), int(p.frame_rows[f1])
        d = p.dev
        points, coff, mcoff, boxes, woff, inst_off, inst_rgb, status = ops.scene_polygons(
            d["frame_rows"], d["ids"], d["poly_off"], d["poly_xy"], f0, f1, i1 - i0, int(self.kept[i0:i1].sum()),
            int(p.poly_off[i0]), int(p.poly_off[i1]), H, W, _device_palette(dev), self.bgr)
        used, local = np.unique(self.glyphs(font_px(H, W), i0, i1), return_inverse=True)
        gwh, gwoff, gwords = self.atlas.arrays(used)
        label_off = (p.frame_rows[f0:f1 + 1] - i0).astype(np.int32)
        up = _upload([label_off, self.anchors[i0:i1], local.astype(np.int32).reshape(-1), self.label_rgb[i0:i1],
                      gwh.astype(np.int32), gwoff.astype(np.int64), gwords.astype(np.uint32)], dev)
        nwords, bad = torch.cat((woff[-1:], status.to(torch.int64))).tolist()
        if bad & ops.SCENE_BAD_COORD:
            raise ShowError("a polygon coordinate beyond +-2^20")
        if bad:
            raise ShowError("the parsed rows are not the ones the scene was counted from (status %d)" % bad)
        face = torch.empty((nwords,), dtype=torch.int32, device=dev)
        line = torch.empty((nwords,), dtype=torch.int32, device=dev)
        area = torch.empty((i1 - i0,), dtype=torch.int32, device=dev)
        return _Dims(f1 - f0, H, W), ([points, coff, mcoff, boxes, woff, inst_off, inst_rgb] + up, face, line, area)


def draw_chunk_parsed(frames_u8, scenes, f0, bgr=True):
    """`draw_chunk_resident` with the scene made from parsed rows: the chunk is frames f0 .. f0 + len(frames_u8) - 1 of the
    video `scenes` (a `ParsedScenes`) describes.  -> a CUDA u8 tensor [F,H,W,3]; resident frames are drawn in place."""
    import torch
    if not len(frames_u8):
        raise ValueError("no frames")
    if is_resident(frames_u8):
        fr = _resident_frames(frames_u8)
    else:
        if not torch.cuda.is_available():
            raise ShowError("no GPU: drawing runs in csrc/overlay.hip (use --host-draw for the numpy path)")
        part = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames_u8]), dtype=np.uint8)
        if part.ndim != 4 or part.shape[3] != 3:
            raise ValueError("frames must be u8 [F,H,W,3]")
        fr = torch.from_numpy(part).to(torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(fr.device):
        dims, arrays = scenes.chunk(f0, f0 + fr.shape[0], int(fr.shape[1]), int(fr.shape[2]), fr.device)
        return launch(fr, dims, arrays)


def draw_chunk_resident(frames_u8, rows_per_frame, voc_size, atlas, bgr=True):
    """One chunk of `draw_clip` on the GPU, the drawn frames left there for the encoder: -> a CUDA u8 tensor [F,H,W,3].
    `frames_u8` may be a CUDA u8 [F,H,W,3] tensor (frames decoded on the GPU): it is drawn where it lies, in place, and
    returned; host frames are uploaded as ever."""
    if len(rows_per_frame) != len(frames_u8) or not len(frames_u8):
        raise ValueError("%d frames but rows for %d" % (len(frames_u8), len(rows_per_frame)))
    if is_resident(frames_u8):
        fr = _resident_frames(frames_u8)
        return compose_resident(fr, _scene_of_rows(rows_per_frame, voc_size, atlas, fr.shape[1], fr.shape[2], bgr))
    return compose_resident(*_chunk_scene(frames_u8, rows_per_frame, voc_size, atlas, bgr))


def draw_gather_resident(ring, slots, rows_per_frame, voc_size, atlas, bgr=True):
    """`draw_chunk_resident` for frames that wait in a ring (`online.OnlineSpotter`'s pending frames): frame i of the result
    is ring[slots[i]] with rows_per_frame[i] drawn on it.  The ring is only read.  -> a new dense CUDA u8 tensor [F,H,W,3]."""
    if len(rows_per_frame) != len(slots) or not len(slots):
        raise ValueError("%d slots but rows for %d" % (len(slots), len(rows_per_frame)))
    scene = _scene_of_rows(rows_per_frame, voc_size, atlas, ring.shape[1], ring.shape[2], bgr)
    return compose_gather_resident(ring, slots, scene)


def draw_clip(frames_u8, rows_per_frame, voc_size, font=None, host=False, chunk=CHUNK, bgr=True, atlas=None):
    """Frames u8 [F,H,W,3] (an array or a list of H x W x 3 arrays) and, per frame, its result rows -> the drawn frames u8
    [F,H,W,3].  Per chunk of at most `chunk` frames: one fill, one outline and one compose call with one upload and one copy
    back; host=True does the same integer arithmetic in numpy and returns the same bytes.  The colours of a track are RGB;
    bgr=True (what `eval.read_frame` yields) hands them to the rule in the frames' B, G, R order.  `atlas` carries the label
    bitmaps from one call to the next."""
    F = len(frames_u8)
    if len(rows_per_frame) != F:
        raise ValueError("%d frames but rows for %d" % (F, len(rows_per_frame)))
    if F == 0:
        return np.zeros((0, 0, 0, 3), dtype=np.uint8)
    atlas = atlas or Atlas(font)
    out = []
    for f0 in range(0, F, int(chunk)):
        part, scene = _chunk_scene(frames_u8[f0:f0 + chunk], rows_per_frame[f0:f0 + chunk], voc_size, atlas, bgr)
        out.append(compose_host(part, scene) if host else compose_device(part, scene))
    if any(o.shape[1:] != out[0].shape[1:] for o in out):
        raise ValueError("the frames of a clip must share one size")
    return np.concatenate(out)


def write_frame(bgr, path):
    """One drawn frame in the format its extension names (JPEG at quality 95)."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
    if os.path.splitext(path)[1].lower() in (".jpg", ".jpeg"):
        im.save(path, quality=95)
    else:
        im.save(path)


def is_jpeg(path):
    return os.path.splitext(path)[1].lower() in (".jpg", ".jpeg")


def write_bytes(data, path):
    with open(path, "wb") as fp:
        fp.write(data)


def _write_encoded(drawn, targets, pool, encode, quality):
    """The writing step of a chunk under --device-encode (`drawn` = the resident CUDA tensor) or --host-encode (a host
    array): the JPEG targets through the project's encoder -- the pool only writes bytes --, every other target through Pillow."""
    from . import jpeg as _jpeg
    jpg = [i for i, t in enumerate(targets) if is_jpeg(t)]
    rest = [i for i, t in enumerate(targets) if not is_jpeg(t)]
    H, W = int(drawn.shape[1]), int(drawn.shape[2])
    if encode == "device":
        import torch
        from . import lib as _lib
        from . import ops
        if jpg:
            sel = drawn if not rest else drawn[torch.as_tensor(jpg, device=drawn.device)]
            try:
                payload, offsets = ops.jpeg_encode(sel, quality, True)
            except _lib.GomError as e:
                raise ShowError(str(e))
            data = _jpeg.files(payload.cpu().numpy(), offsets.numpy(), H, W, quality)
        others = drawn[torch.as_tensor(rest, device=drawn.device)].cpu().numpy() if rest else []
    else:
        if jpg:
            try:
                data = _jpeg.files(*_jpeg.encode_host(drawn[jpg], quality, True), H, W, quality)
            except ValueError as e:
                raise ShowError(str(e))
        others = drawn[rest] if rest else []
    if jpg:
        list(pool.map(write_bytes, data, [targets[i] for i in jpg]))
    if rest:
        list(pool.map(write_frame, others, [targets[i] for i in rest]))


def draw_video(frames, annotation, paths, video_name, out_dir, voc_size, pool, atlas, host=False, encode=None, quality=95,
               parsed=None):
    """Draw a whole video (BGR frames, `annotation` = {1-based frame id as str: rows}) chunk by chunk and write
    out_dir/results/<video name>/<basename of the frame's source path> through `pool`.  encode = None: Pillow writes every
    file; "device" / "host": the JPEG frames go through csrc/jpeg.hip (the drawn chunk never leaves the GPU) / through
    `jpeg.encode_host`, at `quality`.
    `frames` may be, instead of the list of host frames, a function `frames(f0, f1)` that returns frames f0 .. f1 - 1 of the
    video (one per path) as ONE CUDA u8 [f1 - f0,H,W,3] tensor, called once per chunk of at most CHUNK frames in order (a
    `DecodedChunks`): the chunk is drawn where it lies and no more than one chunk of pixels is ever held.  It raises
    `ShowError` for frames of a chunk that differ in size.
    parsed = a `results.ParsedRows` (status 0) in place of `annotation` (then None): every chunk's scene is made from the rows
    where the parser left them (`ParsedScenes`: `ops.scene_polygons` plus the host's label arrays) and drawn on the GPU, for
    host frames (uploaded as ever) and for a provider alike; the same bytes.  Not with host=True."""
    provider = frames if callable(frames) else None
    count = len(paths) if provider is not None else len(frames)
    have = parsed.F if parsed is not None else len(annotation)
    if have != count:
        raise ShowError("video %s: %d frames but results for %d" % (video_name, count, have))
    if parsed is not None and host:
        raise ValueError("parsed rows are drawn on the GPU")
    if parsed is not None and not parsed.has_seg.all():
        raise ShowError("video %s: result rows without a segmentation cannot be drawn" % video_name)
    save_dir = os.path.join(out_dir, "results", video_name)
    os.makedirs(save_dir, exist_ok=True)
    if parsed is not None:
        scenes = ParsedScenes(parsed, voc_size, atlas)
    else:
        try:
            rows = [annotation[str(i + 1)] for i in range(count)]
        except KeyError as e:
            raise ShowError("video %s: no results for frame %s" % (video_name, e))
    for f0 in range(0, count, CHUNK):
        targets = [os.path.join(save_dir, os.path.basename(p)) for p in paths[f0:f0 + CHUNK]]
        try:
            if parsed is not None:
                part = provider(f0, min(f0 + CHUNK, count)) if provider is not None else frames[f0:f0 + CHUNK]
                drawn = draw_chunk_parsed(part, scenes, f0)
                if encode != "device":
                    drawn = drawn.cpu().numpy()
                del part
            elif provider is not None:
                part = provider(f0, min(f0 + CHUNK, count))
                if host:                                    # (the numpy rule on frames decoded on the GPU: one copy back)
                    drawn = draw_clip(part.cpu().numpy(), rows[f0:f0 + CHUNK], voc_size, host=True, atlas=atlas)
                else:
                    drawn = draw_chunk_resident(part, rows[f0:f0 + CHUNK], voc_size, atlas)
                    if encode != "device":
                        drawn = drawn.cpu().numpy()
                del part
            elif encode == "device":
                drawn = draw_chunk_resident(frames[f0:f0 + CHUNK], rows[f0:f0 + CHUNK], voc_size, atlas)
            else:
                drawn = draw_clip(frames[f0:f0 + CHUNK], rows[f0:f0 + CHUNK], voc_size, host=host, atlas=atlas)
            if encode is not None:
                _write_encoded(drawn, targets, pool, encode, quality)
        except ShowError as e:
            raise ShowError("video %s: %s" % (video_name, e))
        if encode is None:
            list(pool.map(write_frame, drawn, targets))


class DecodedChunks:
    """The frames of one video for `draw_video`, decoded on the GPU chunk by chunk (`--device-decode`): `pool` reads the
    files' bytes one chunk ahead, `eval.decode_frames` makes the chunk's pixels in device memory -- baseline JPEG files in
    csrc/jpeg_decode.hip, files of another extension, refused files and flagged files through Pillow, per file, `counts`
    incremented per route -- and the chunk is handed over as ONE CUDA u8 [n,H,W,3] tensor.  Host memory holds file bytes only,
    device memory one chunk.  Called with consecutive ranges, in order."""

    def __init__(self, paths, pool, counts, device, walk="auto", chunk=CHUNK):
        self.paths, self.pool, self.counts, self.device, self.walk, self.chunk = paths, pool, counts, device, walk, int(chunk)
        self._next = 0
        self._ahead = self._read(0)

    def _read(self, f0):
        from . import eval as _eval
        return [self.pool.submit(_eval.read_bytes, p) for p in self.paths[f0:f0 + self.chunk]]

    def __call__(self, f0, f1):
        import torch
        from . import eval as _eval
        if f0 != self._next or not f0 < f1 <= f0 + self.chunk:
            raise ValueError("chunks are taken in order, at most %d frames each: asked for %d .. %d at frame %d"
                             % (self.chunk, f0, f1, self._next))
        blobs = [f.result() for f in self._ahead][:f1 - f0]
        self._next = f1
        self._ahead = self._read(f1)
        frames = _eval.decode_frames(self.paths[f0:f1], blobs, self.counts, self.device, self.walk)
        del blobs
        if any(tuple(f.shape) != tuple(frames[0].shape) for f in frames):
            raise ShowError("the frames of a clip must share one size")
        return torch.stack(frames)


def print_draw_routes(counts, walk, shared=False):
    """The route counts of the decodes made for drawing, on a line of their own; shared=True: the frames drawn are the ones
    the spotter's own decode made (an online run), counted by the route they took there."""
    print("drawing decode: ", counts["device"], " files decoded on the GPU ",
          "once, for spotting and drawing" if shared else "for drawing", "; through Pillow: ", counts["other"],
          " with another extension, ", counts["refused"], " refused by the parser, ", counts["flagged"],
          " with a status word set; walk (--decode-walk ", walk, "): ", counts.get("chunks", 0), " segments by the chunk walk, ",
          counts.get("serial", 0), " by the serial walk")


def print_read_routes(counts):
    """The routes the result files took under --device-read, on a line of their own; for the refused ones, why."""
    why = ", ".join("%s: %d" % kv for kv in sorted(counts["causes"].items()))
    print("result files: ", counts["device"], " read on the GPU, ", counts["host"], " through json.load",
          " (refused by the parser -- %s)" % why if why else "", sep="")


def rows_of_json(tracks):
    """`jsons/<video>.json` -> the annotation `results.write_video` returns: {frame: [[x1..y4, id, text, [polygon]], ..]}."""
    out = {}
    for frame, objs in tracks.items():
        rows = []
        for o in objs:
            row = list(o["points"]) + [o["ID"], o["transcription"]]
            if "segmentation" in o:
                row.append(o["segmentation"])
            rows.append(row)
        out[str(frame)] = rows
    return out


# ------------------------------------------------------------------------------------------ command line
def add_encode_arguments(p):
    """--device-encode, --host-encode and --jpeg-quality, for this command and for `eval --show`."""
    p.add_argument("--device-encode", action="store_true",
                   help="encode the drawn JPEG frames on the GPU (csrc/jpeg.hip): only compressed bytes come back (default: "
                        "Pillow on the host; not with --host-draw)")
    p.add_argument("--host-encode", action="store_true",
                   help="encode the drawn JPEG frames with the same integer rule in numpy: the files of --device-encode")
    p.add_argument("--jpeg-quality", type=int, default=None, metavar="N",
                   help="with --device-encode or --host-encode: JPEG quality 1 .. 100 (default 95)")


def encode_choice(args):
    """The parsed encode flags -> (None | "device" | "host", quality, exit status, message): status 2 for flags that do not go
    together, 1 for --device-encode on a machine without a GPU, 0 otherwise."""
    quality = 95 if args.jpeg_quality is None else args.jpeg_quality
    if args.device_encode and args.host_encode:
        return None, quality, 2, "give at most one of --device-encode and --host-encode"
    if args.device_encode and args.host_draw:
        return None, quality, 2, "--device-encode encodes frames drawn on the GPU: it does not go with --host-draw " \
                                 "(--host-encode writes the same files)"
    if args.jpeg_quality is not None and not (args.device_encode or args.host_encode):
        return None, quality, 2, "--jpeg-quality goes with --device-encode or --host-encode"
    if not 1 <= quality <= 100:
        return None, quality, 2, "--jpeg-quality must lie in 1 .. 100"
    if args.device_encode:
        import torch
        if not torch.cuda.is_available():
            return None, quality, 1, "--device-encode needs a GPU (--host-encode writes the same files without one)"
        return "device", quality, 0, ""
    return ("host" if args.host_encode else None), quality, 0, ""


def get_parser():
    p = argparse.ArgumentParser(
        prog="python -m gomatching_amd.show",
        description="Draw the tracked text of OUT/jsons/*.json on the frames of a dataset directory: a translucent polygon per "
                    "instance in the colour of its track and a (id)TEXT label; writes results/<video>/<frame file>.  Needs no "
                    "model; it is also how a resumed eval gets its pictures.")
    p.add_argument("--input", required=True, metavar="DIR", help="dataset directory, as given to gomatching_amd.eval")
    p.add_argument("--results", required=True, metavar="OUT", help="the --output directory of gomatching_amd.eval (reads OUT/jsons)")
    p.add_argument("--output", default=None, metavar="DIR", help="directory for results/ (default: OUT)")
    p.add_argument("--font", default=None, metavar="FILE", help="a TrueType font for the labels (default: Pillow's built-in font)")
    p.add_argument("--host-draw", action="store_true", help="draw in numpy on the host (default: on the GPU, the same bytes)")
    add_encode_arguments(p)
    p.add_argument("--device-decode", action="store_true",
                   help="decode baseline JPEG frames on the GPU (the same bytes as Pillow's) and draw them where they lie: the "
                        "pool reads file bytes one chunk ahead, nothing is uploaded; any other file goes through Pillow, per "
                        "file (not with --host-draw)")
    p.add_argument("--decode-walk", choices=("auto", "segments", "chunks"), default=None,
                   help="with --device-decode: the decoder's entropy walk, as in gomatching_amd.eval (default auto)")
    p.add_argument("--device-read", action="store_true",
                   help="read every result file on the GPU (csrc/result_parse.hip) and build each chunk's polygons there from "
                        "the parsed rows; a file that is not the canonical json.dumps(indent=4) text goes through json.load, "
                        "per file (not with --host-draw)")
    p.add_argument("--voc-size", type=int, default=None, metavar="N",
                   help="vocabulary size of the model: 37 upper-cases the labels (default 37)")
    p.add_argument("--config-file", default=None, metavar="FILE", help="take the vocabulary size from a config file")
    p.add_argument("--builtin", default=None, metavar="NAME", help="take the vocabulary size from a packaged config")
    return p


def main(argv=None):
    from . import config as _config
    from . import eval as _eval
    from . import results as _results
    args = get_parser().parse_args(argv)
    if sum(v is not None for v in (args.voc_size, args.config_file, args.builtin)) > 1:
        sys.stderr.write("error: give at most one of --voc-size, --config-file and --builtin\n")
        return 2
    if args.builtin is not None and args.builtin not in _config.BUILTIN:
        sys.stderr.write("error: unknown packaged config %r\n" % args.builtin)
        return 2
    if args.config_file is not None and not os.path.isfile(args.config_file):
        sys.stderr.write("error: config file %r not found\n" % args.config_file)
        return 2
    if not os.path.isdir(args.input):
        sys.stderr.write("error: input directory %r not found\n" % args.input)
        return 2
    if args.decode_walk is not None and not args.device_decode:
        sys.stderr.write("error: --decode-walk goes with --device-decode\n")
        return 2
    if args.device_decode and args.host_draw:
        sys.stderr.write("error: --device-decode leaves the frames in device memory, where they are drawn: it does not go with "
                         "--host-draw\n")
        return 2
    if args.device_read and args.host_draw:
        sys.stderr.write("error: --device-read leaves the rows in device memory, where the scene is made from them: it does not "
                         "go with --host-draw\n")
        return 2
    encode, quality, status, message = encode_choice(args)
    if status:
        sys.stderr.write("error: %s\n" % message)
        return status
    read_routes = None
    if args.device_read:
        import torch
        if not torch.cuda.is_available():
            sys.stderr.write("error: --device-read needs a GPU: the parser runs in csrc/result_parse.hip\n")
            return 1
        read_routes = {"device": 0, "host": 0, "causes": {}}
        read_device = torch.device("cuda", torch.cuda.current_device())
    routes = None
    if args.device_decode:
        import torch
        if not torch.cuda.is_available():
            sys.stderr.write("error: --device-decode needs a GPU: the decoder runs in csrc/jpeg_decode.hip\n")
            return 1
        routes = {k: 0 for k in _eval.DECODE_ROUTES}
        walk = args.decode_walk or "auto"
        device = torch.device("cuda", torch.cuda.current_device())
    voc_size = 37 if args.voc_size is None else args.voc_size
    if args.config_file is not None or args.builtin is not None:
        voc_size = _config.setup_cfg(config_file=args.config_file, opts=[], builtin=args.builtin).MODEL.TRANSFORMER.VOC_SIZE
    out_dir = args.output or args.results
    data_type, videos = _eval.list_videos(args.input)
    atlas = Atlas(args.font)
    try:
        with ThreadPoolExecutor(max_workers=_eval.DECODE_THREADS) as readers, \
                ThreadPoolExecutor(max_workers=WRITE_THREADS) as writers:
            for video_name, video_dir in videos:
                json_path = os.path.join(args.results, "jsons", "%s.json" % _results.result_names(video_name, data_type)[1])
                if not os.path.isfile(json_path):
                    raise ShowError("video %s: result file %s not found" % (video_name, json_path))
                parsed = None
                if read_routes is not None:                 # the file's bytes to the GPU; a refused file is read as ever
                    with open(json_path, "rb") as fp:
                        data = fp.read()
                    parsed = _results.parse_json_device(data, read_device)
                    if parsed.status:
                        read_routes["host"] += 1
                        for cause in parsed.causes():
                            read_routes["causes"][cause] = read_routes["causes"].get(cause, 0) + 1
                        parsed, annotation = None, rows_of_json(json.loads(data.decode("utf-8")))
                    else:
                        read_routes["device"] += 1
                        annotation = None
                    del data
                else:
                    with open(json_path, "r", encoding="utf-8") as fp:
                        annotation = rows_of_json(json.load(fp))
                paths = _eval.frame_paths(video_dir)
                have = parsed.F if parsed is not None else len(annotation)
                if len(paths) != have:
                    raise ShowError("video %s: %d frames but results for %d" % (video_name, len(paths), have))
                if (not parsed.has_seg.all()) if parsed is not None else \
                        any(len(row) < 11 for rows in annotation.values() for row in rows):
                    raise ShowError("video %s: result rows without a segmentation cannot be drawn" % video_name)
                print("drawing {}...".format(video_name))
                if routes is not None:                      # bytes one chunk ahead, pixels made and drawn on the GPU
                    frames = DecodedChunks(paths, readers, routes, device, walk)
                else:
                    frames = list(readers.map(_eval.read_frame, paths))
                draw_video(frames, annotation, paths, video_name, out_dir, voc_size, writers, atlas, host=args.host_draw,
                           encode=encode, quality=quality, parsed=parsed)
    except ShowError as e:
        sys.stderr.write("error: %s\n" % e)
        return 2
    if routes is not None:
        print_draw_routes(routes, walk)
    if read_routes is not None:
        print_read_routes(read_routes)
    return 0


if __name__ == "__main__":
    sys.exit(main())
