"""Online spotting: a video goes in push by push and each frame's result rows come out as soon as its tracks have settled --
the rows, byte for byte, that the offline path (`results.spot_video` -> `_remove_short_track` -> `batch_postprocess` ->
`results.clip_lines`) produces once the whole video is in, with bounded latency and bounded memory.

Why that is possible.  Ids of frame t are final once t is tracked (`run_long_term_match` only writes the ids of the current
frame k), and a frame's detections do not depend on what shares its detector step.  The one thing that needs
the future is `_remove_short_track`, and it needs a bounded amount of it.

The settling rule (also in include/gomatching_hip.h).  L = model.test_len, M = model.min_track_len, R = max(L - 1, 1): how
many frames back a match can reach -- in `GoMatching.track_frames` the long-term window starts at
`win_st = real + 1 - test_len` and the short-term match sees frame `real - 1`; the native path hands over
`carried = instances[-max(test_len - 1, 1):]`.  After frame t (0-based) is tracked, with c(id) the detections of a track so
far and s(id) the last frame it was seen in, a track is

    confirmed   c >= M                  its rows are kept, past ones included
    dead        c <  M and t >= s + R   frame t + 1 can no longer reach frame s: no later frame can take the id; rows dropped
    open        otherwise

A frame is settled when none of its ids is open.  Frames leave in frame order: the longest settled prefix of the pending
frames goes out.  With M <= 0 every frame settles as soon as it is tracked; `close()` makes every open track dead.  So a frame
leaves at most D = max(M - 1, 0) * R frames after it was tracked (20 frames for every shipped config: MIN_TRACK_LEN 5,
TEST_LEN 6), and its kept rows are exactly those `_remove_short_track` keeps.  An id that shows up again beyond the reach is
a broken invariant and raises; nothing is emitted silently.  (Ids are issued in increasing order -- `id_count + 1` in
`run_short_term_match` / `run_long_term_match` -- which is what lets the settler forget a track once it is out of reach and
its frames have left, and still recognise its id if it ever came back.)
"""
import collections
import time

import numpy as np


class TrackSettler:
    """The rule above on the host, no torch and no GPU: one int64 id array per frame in, `(frame index, keep mask)` tuples in
    frame order out.  Holds the pending frames' ids and one (count, last frame) pair per track that can still matter, so its
    memory does not grow with the stream."""

    def __init__(self, test_len, min_track_len):
        self.reach = max(int(test_len) - 1, 1)
        self.min_track_len = int(min_track_len)
        self.latency_bound = max(self.min_track_len - 1, 0) * self.reach
        self._count, self._last = {}, {}
        self._frames = collections.deque()                       # (frame index, ids) tracked and not yet emitted
        self._high = None                                        # largest id seen in earlier frames
        self.frames_seen = 0
        self.emitted = 0                                         # frames emitted so far = index of the first pending frame
        self.max_wait, self.wait_sum = 0, 0
        self.rows_dropped = 0
        self.closed = False

    @property
    def pending(self):
        return len(self._frames)

    def push(self, ids):
        """Ids of the next frame -> the frames that settled with it."""
        if self.closed:
            raise RuntimeError("the settler is closed")
        ids = np.array(ids, dtype=np.int64).reshape(-1)
        t = self.frames_seen
        count, last = self._count, self._last
        for i in ids.tolist():
            s = last.get(i)
            if s is None:
                if self._high is not None and i <= self._high:
                    raise RuntimeError("frame %d: id %d appears after its track was closed (ids are issued in increasing "
                                       "order; the largest so far is %d)" % (t, i, self._high))
                count[i] = 0
            elif t - s > self.reach:
                raise RuntimeError("frame %d: id %d appears %d frames after frame %d, beyond the reach of %d frames: the "
                                   "track was %s" % (t, i, t - s, s, self.reach,
                                                     "dead" if count[i] < self.min_track_len else "out of reach"))
            count[i] += 1
            last[i] = t
        if len(ids):
            m = int(ids.max())
            self._high = m if self._high is None else max(self._high, m)
        self._frames.append((t, ids))
        self.frames_seen = t + 1
        out = self._emit(t, final=False)
        for i in [i for i, s in last.items() if s < self.emitted and t >= s + self.reach]:
            del last[i], count[i]                                # out of reach and in no pending frame: nothing asks again
        return out

    def close(self):
        """End of the stream: every open track is dead; -> the remaining frames."""
        if self.closed:
            return []
        self.closed = True
        out = self._emit(self.frames_seen - 1, final=True)
        self._count.clear()
        self._last.clear()
        return out

    def _emit(self, t, final):
        out, M, R = [], self.min_track_len, self.reach
        count, last = self._count, self._last
        while self._frames:
            f, ids = self._frames[0]
            keep = np.ones((len(ids),), dtype=bool)
            settled = True
            for j, i in enumerate(ids.tolist()):
                if count[i] >= M:
                    continue
                if final or t >= last[i] + R:
                    keep[j] = False
                else:
                    settled = False
                    break
            if not settled:
                break
            self._frames.popleft()
            self.emitted = f + 1
            wait = t - f
            self.max_wait = max(self.max_wait, wait)
            self.wait_sum += wait
            self.rows_dropped += len(ids) - int(keep.sum())
            out.append((f, keep))
        return out


class OnlineSpotter:
    """One video as a stream.  `push(frames)` takes HxWx3 uint8 frames (BGR, as `eval.read_frame` yields) and returns
    `[(frame_index, rows), ...]` for the frames that settled, `rows` being what `results.frame_lines` / `clip_lines` produce
    for that frame after the offline post-processing; `push_inputs(inputs)` is the same for callers that already hold
    prepared inputs (`GoMBatchPredictor.prepare` / `prepare_device`); `close()` runs what is left and returns the rest.

    Frames are buffered and the detector only runs on FULL steps of `model.frames_per_step` frames (`close()` runs the
    tail), so a stream uses one captured graph shape -- `_detect_graphed` keys its graphs by the step size and each pins its
    activation pool.  Build the model with `frames_per_step=1` for per-frame latency.  Several steps pushed in ONE call keep
    the overlap of step j's tracker with step j + 1's detector (`GoMatching.stream_inference`); one step per call cannot.

    Device memory: a ring of `cap = (D + R + 2 * frames_per_step) * NUM_QUERIES` rows, `bd [cap,25,4]` f32 and
    `recs [cap,25]` int64, allocated once.  Every tracked step's boundaries and character ids are copied in by the step (two
    copies; `Instances._gom["det"]` / `["b"]` identify the step's tensors as they do for `dist.pack_records`; foreign
    Instances are copied per frame).  From then on a pending frame needs only its host mirror (ids, count, ring slot, scale
    pair), and `instances[i]` becomes None once frame i has been emitted and is older than the tracker window.  The ring is
    never overwritten: a step that does not fit first gathers what has settled, and raises if that is not enough.

    Per push, for the frames that settled: ONE descriptor upload, ONE `ops.result_rows_gather` launch, ONE copy back, then
    `results.finish_rows` on the host -- the function the offline path ends in.  (A single push of more steps than the ring
    has room for gathers in between.)

    device_text=True: the gathered words stay on the device.  Only the words `results.finish_points` needs come back, the
    rectangle points go up, `ops.result_text` formats the settled frames (csrc/result_text.hip) and `push` / `close()` return
    `[(first frame, frame count, json bytes, xml bytes), ...]` for `VideoResultWriter.add_text` instead of row lists.

    device_vote=True (with device_text=True): every gather's words and keep flags also go to a `results.TrackVote` -- only
    settled rows reach it, the rows the offline path keeps -- and `close()` leaves the bytes of preds/res_<video>.txt in
    `track_txt` for `VideoResultWriter.close`.  The vote's log, 112 bytes per row, is the one thing a session holds that grows
    with the video.

    device_lexicon=a `lexicon.RowCorrection` (with device_text=True and device_vote=True): every gather's rows are also corrected
    by the video's lexicon where they lie (csrc/lexicon_rows.hip: the correction is per row, only the vote waits for `close()`);
    the items `push` / `close()` return carry the corrected json and xml bytes as a fifth and sixth element, for a second
    `VideoResultWriter` rooted at <out>/lexicon, and `close()` leaves the vote over the corrected words in `lexicon_txt`.

    draw=a `show.Atlas`, or True for a fresh one (with device_ingest=True): the session also draws.  A pixel ring `ring_px` u8
    `[cap_frames,H,W,3]` is allocated once, when the first frame's size is known (41 slots at the shipped configs with 8 frames
    per step: 113 MB at 1280x720), beside `ring_bd` / `ring_recs` and under their rule: slot f % cap_frames, the same tail,
    never overwritten.  A frame of another size is refused with a `show.ShowError` before the push runs anything.  Every step
    copies its frames' source pixels (`inputs[j]["frame_u8"]`: device to device for frames decoded on the GPU, an upload for
    host tensors) into their slots, ordered with the step's other ring copies.  For the frames that settle, the gather builds
    their scene from their finished rows with `show._scene_of_rows`, the offline function (under device_text=True the row
    lists are built for the drawing only), and runs the fill and outline launches and ONE `gom_overlay_compose_gather_u8`
    launch from the ring into a dense tensor; the next copy into the ring waits for that launch's event.  `take_drawn()`
    hands the drawn frames out, `[(first frame, CUDA u8 [n,H,W,3]), ...]`, covering exactly the frames whose rows or text the
    same `push` / `close()` returned -- `show.draw_clip` of those frames and rows, byte for byte.  What `push` / `close()`
    return does not change, and encoding is the caller's choice.  Without `draw` the session allocates, launches and returns
    what it always did."""

    def __init__(self, cfg, model, decoder, device_ingest=True, time_cost=None, min_extent=5, device_text=False,
                 device_vote=False, device_lexicon=None, draw=None):
        import torch
        self.device_text = bool(device_text)
        self._atlas = None                                       # draw: the label bitmaps, carried from gather to gather
        if draw is not None and draw is not False:
            from . import show as _show
            if not device_ingest:
                raise ValueError("draw takes the frames' source pixels from the inputs' frame_u8: it needs device_ingest=True")
            self._atlas = _show.Atlas() if draw is True else draw
        self.ring_px = None                                      # draw: u8 [cap_frames,H,W,3], allocated with the first frame
        self._drawn = []                                         # draw: (first frame, CUDA u8 [n,H,W,3]) not yet taken
        self._px_free = None                                     # draw: event after the last launch that read ring slots
        self._main, self._sources = None, None
        if device_vote and not device_text:
            raise ValueError("device_vote=True votes over the rows device_text=True leaves on the GPU: it needs device_text=True")
        if device_lexicon is not None and not (device_text and device_vote):
            raise ValueError("device_lexicon corrects the rows on the GPU: it needs device_text=True and device_vote=True")
        from . import results as _results
        self._vote = _results.TrackVote(decoder) if device_vote else None
        self.track_txt = None                                    # device_vote=True: the txt file's bytes, from `close()` on
        self._lexicon = device_lexicon
        self.lexicon_txt = None                                  # device_lexicon: the corrected txt file's bytes, from `close()` on
        if device_lexicon is not None:
            device_lexicon.vote = _results.TrackVote(decoder)
        from .predictor import GoMBatchPredictor, new_time_cost
        self.cfg, self.model, self.decoder, self.min_extent = cfg, model, decoder, min_extent
        self.predictor = GoMBatchPredictor(cfg, model, device_ingest=device_ingest)
        self.time_cost = new_time_cost() if time_cost is None else time_cost
        self.settler = TrackSettler(model.test_len, model.min_track_len)
        self.step = int(model.frames_per_step)
        self.nq = int(cfg.MODEL.TRANSFORMER.NUM_QUERIES)
        self.cap_frames = self.settler.latency_bound + self.settler.reach + 2 * self.step
        cap = self.cap_frames * self.nq
        self.ring_bd = torch.empty((cap, 25, 4), dtype=torch.float32, device=model.device)
        self.ring_recs = torch.empty((cap, 25), dtype=torch.int64, device=model.device)
        self.instances, self.id_count = [], 0
        self._buffer = []                                        # prepared inputs short of a full step
        self._sizes = []                                         # source (height, width) of the frames of the running call
        self._meta = {}                                          # pending frame -> (ring row of its first instance, sx, sy, ids)
        self._ready = []                                         # settled (frame, keep mask) whose rows are still in the ring
        self._out = []
        self._ring_tail = 0                                      # first frame whose ring slot is still in use
        self._released = 0                                       # instances[:_released] are None
        self.frames_seen = 0
        self.seconds, self.rows_seconds = 0.0, 0.0               # the timed window (detector, tracker, gather) / finish_rows
        self.gather_launches = 0
        self.max_live_instances, self.ring_high_water = 0, 0
        self.closed = False
        self._in_run = False

    # ---------------------------------------------------------------------------------------- the public surface
    @property
    def latency_bound(self):
        """A frame leaves at most this many frames after it was tracked (plus what the step buffer holds back)."""
        return self.settler.latency_bound

    @property
    def pending(self):
        """Frames taken in and not yet returned (buffered ones included)."""
        return self.frames_seen - self.settler.emitted

    @property
    def max_wait(self):
        return self.settler.max_wait

    def push(self, frames):
        prepare = self.predictor.prepare_device if self.predictor.device_ingest else self.predictor.prepare
        inputs = []
        for f in frames:                                         # one by one: every frame is scaled back to its OWN size
            inputs.extend(prepare([f])[0])
        return self.push_inputs(inputs)

    def push_inputs(self, inputs):
        if self.closed:
            raise RuntimeError("the session is closed")
        if self._atlas is not None:
            self._check_sizes(inputs)
        self._buffer.extend(inputs)
        self.frames_seen += len(inputs)
        full = len(self._buffer) // self.step * self.step
        if full:
            run, self._buffer = self._buffer[:full], self._buffer[full:]
            self._run(run)
            self._gather()
        return self._take()

    def close(self):
        if self.closed:
            return []
        self.closed = True
        if self._buffer:
            run, self._buffer = self._buffer, []
            self._run(run)
        self._ready.extend(self.settler.close())
        self._gather()
        self.instances = []
        if self._vote is not None:
            t0 = time.time()
            self.track_txt = self._vote.finish()
            if self._lexicon is not None:
                self.lexicon_txt = self._lexicon.vote.finish()
            self.rows_seconds += time.time() - t0
        return self._take()

    def take_drawn(self):
        """draw: the frames that settled since the last call with their tracked text drawn on them, as
        `[(first frame, CUDA u8 [n,H,W,3]), ...]` in frame order -- exactly the frames whose rows or text `push` / `close()`
        returned since.  The tensors are the caller's: encoding and writing them is the caller's choice."""
        out, self._drawn = self._drawn, []
        return out

    # ---------------------------------------------------------------------------------------- inside
    def _take(self):
        out, self._out = self._out, []
        return out

    def _check_sizes(self, inputs):
        """draw: every frame of a session has the size of its first one -- refused before the push runs anything -- and the
        pixel ring is allocated once, when that size is known: cap_frames slots, slot f % cap_frames for frame f, the tail
        and the never-overwritten guarantee of `ring_bd` / `ring_recs`."""
        import torch
        from .show import ShowError
        for x in inputs:
            src = x.get("frame_u8")
            if src is None or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
                raise ValueError("draw needs every input's source pixels: frame_u8, a uint8 [H,W,3] tensor")
            hw = tuple(int(v) for v in src.shape[:2])
            if self.ring_px is None:
                self.ring_px = torch.empty((self.cap_frames,) + hw + (3,), dtype=torch.uint8, device=self.model.device)
            if hw != tuple(self.ring_px.shape[1:3]):
                raise ShowError("the frames of a clip must share one size: a frame of %d x %d in a stream of %d x %d"
                                % (hw[1], hw[0], self.ring_px.shape[2], self.ring_px.shape[1]))

    def _draw(self, first, rows_per_frame):
        """draw: frames first .. first + len(rows_per_frame) - 1 have settled -- their scene from their finished rows (the
        offline function), the fill and outline launches and ONE gather-compose launch from their ring slots into a dense
        tensor.  An event after the launch is what the next copy into the ring waits for, whichever stream it runs on."""
        import torch
        from . import show as _show
        t0 = time.time()
        slots = [(first + i) % self.cap_frames for i in range(len(rows_per_frame))]
        drawn = _show.draw_gather_resident(self.ring_px, slots, rows_per_frame, self.cfg.MODEL.TRANSFORMER.VOC_SIZE, self._atlas)
        self._px_free = torch.cuda.Event()
        self._px_free.record()
        if self._main is not None:                               # (a gather inside a step runs on the tracker stream)
            drawn.record_stream(self._main)
        self._drawn.append((first, drawn))
        self.rows_seconds += time.time() - t0

    def _run(self, inputs):
        import torch
        t0 = time.time()
        self._sizes = [(x["height"], x["width"]) for x in inputs]
        self._frame0 = len(self.instances)
        if self._atlas is not None:                              # draw: `_on_step` copies the frames' source pixels
            self._sources = [x["frame_u8"] for x in inputs]
            self._main = torch.cuda.current_stream()
            self._src_ready = torch.cuda.Event()                 # the frames were made on this stream (a decode, an upload)
            self._src_ready.record()
        with torch.no_grad():
            self._in_run = True
            try:
                self.instances, self.id_count = self.model.stream_inference(inputs, self._frame0, self.id_count, self.instances,
                                                                             self.time_cost, on_step=self._on_step)
            finally:
                self._in_run = False
                self._sources = None
        self.seconds += time.time() - t0

    def _on_step(self, dets, first):
        """Runs on the tracker stream right after `dets` (frames first, first + 1, ...) got their ids."""
        import torch
        model, nq, cap_f, B = self.model, self.nq, self.cap_frames, len(dets)
        self.max_live_instances = max(self.max_live_instances, len(self.instances) - self._released)
        if first + B - self._ring_tail > cap_f:
            self._gather()                                       # frees the slots of everything that has settled
            if first + B - self._ring_tail > cap_f:
                raise RuntimeError("online ring overflow: frames %d..%d do not fit beside the %d pending frames from %d on "
                                   "(%d slots)" % (first, first + B - 1, first - self._ring_tail, self._ring_tail, cap_f))
        self.ring_high_water = max(self.ring_high_water, first + B - self._ring_tail)
        gom = [getattr(d, "_gom", None) or {} for d in dets]
        det = gom[0].get("det")
        whole = det is not None and all(g.get("det") is det and g.get("b") == j for j, g in enumerate(gom)) \
            and tuple(det["bd"].shape[:2]) == (B, nq) and tuple(det["recs"].shape[:2]) == (B, nq)
        if whole:                                                # the step's own tensors: two copies (four where the ring wraps)
            bd, recs = det["bd"].reshape(B * nq, 25, 4), det["recs"].reshape(B * nq, 25)
            done = 0
            while done < B:
                s0 = (first + done) % cap_f
                m = min(B - done, cap_f - s0)
                self.ring_bd[s0 * nq:(s0 + m) * nq].copy_(bd[done * nq:(done + m) * nq])
                self.ring_recs[s0 * nq:(s0 + m) * nq].copy_(recs[done * nq:(done + m) * nq])
                done += m
        if self._atlas is not None:                              # draw: the frames' source pixels, beside their rows
            torch.cuda.current_stream().wait_event(self._src_ready)
            if self._px_free is not None:                        # (what read these slots last has been launched: order it)
                torch.cuda.current_stream().wait_event(self._px_free)
            for j in range(B):                                   # device to device for frames decoded on the GPU
                self.ring_px[(first + j) % cap_f].copy_(self._sources[first - self._frame0 + j], non_blocking=True)
        for j, d in enumerate(dets):
            f, n = first + j, len(d)
            if n > nq:
                raise RuntimeError("frame %d has %d instances, a ring slot holds NUM_QUERIES = %d" % (f, n, nq))
            row0 = (f % cap_f) * nq
            if not whole and n:                                  # foreign Instances: per frame
                self.ring_bd[row0:row0 + n].copy_(d.bd.detach().reshape(n, 25, 4).to(torch.float32))
                self.ring_recs[row0:row0 + n].copy_(d.recs.detach().reshape(n, 25).to(torch.int64))
            ids = model._host(d)["ids"]
            sx, sy = model.output_scale(d.image_size, self._sizes[f - self._frame0])
            self._meta[f] = (row0, np.float32(sx), np.float32(sy), np.array(ids, dtype=np.int64))
            self._ready.extend(self.settler.push(ids))
        # an emitted frame that the tracker window has left is not needed any more (`track_frames` touches
        # instances[real - test_len] for the last time when frame `real` is appended)
        t = first + B - 1
        stop = min(self.settler.emitted, t - model.test_len)
        for i in range(self._released, stop):
            self.instances[i] = None
        self._released = max(self._released, stop)

    def _gather_text(self, ready, counts, rows, ids, sxs, sys_, t0):
        """`_gather` for device_text=True: the same upload and launch, then the text of the settled frames, at most
        `results.TEXT_FRAMES_PER_CALL` frames per `ops.result_text` call."""
        from . import ops, results
        first = ready[0][0]
        assert [f for f, _ in ready] == list(range(first, first + len(ready))), "settled frames leave in frame order"
        words_d = None
        if sum(counts):
            desc = ops.result_rows_desc(np.concatenate(rows), np.concatenate(ids), np.concatenate(sxs), np.concatenate(sys_))
            words_d = ops.result_rows_gather(self.ring_bd, self.ring_recs, desc, self.decoder.voc_size, upload=self.model._h2d)
            self.gather_launches += 1
            dt = time.time() - t0
            self.time_cost["post_process"] += dt
            if not self._in_run:
                self.seconds += dt
        t0 = time.time()
        step = results.TEXT_FRAMES_PER_CALL
        offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        for a in range(0, len(ready), step):
            b = min(a + step, len(ready))
            r0, r1 = int(offsets[a]), int(offsets[b])
            if r1 > r0:                                          # (the copy of the text back waits for the launches: the ring
                text = results.rows_text(words_d[r0:r1], offsets[a:b + 1] - r0, first + a, self.decoder, self.min_extent,
                                         vote=self._vote, lexicon=self._lexicon)
            else:                                                #  slots may be rewritten afterwards)
                text = results.host_text_of_empty_frames(first + a, b - a) * (2 if self._lexicon is not None else 1)
            self._out.append((first + a, b - a) + tuple(text))
        if self._atlas is not None:                              # the row lists, for the drawing only (as `write_video` does)
            lines = results.finish_rows(self.model._d2h(words_d), self.decoder, self.min_extent) if words_d is not None else []
            self._draw(first, [[r for r in lines[int(offsets[i]):int(offsets[i + 1])] if r is not None]
                               for i in range(len(ready))])
        self.rows_seconds += time.time() - t0
        self._ring_tail = ready[-1][0] + 1

    def _gather(self):
        """Rows of every settled frame: one upload, one launch, one copy back; then their ring slots are free."""
        from . import ops, results
        ready, self._ready = self._ready, []
        if not ready:
            return
        t0 = time.time()
        rows, ids, sxs, sys_, counts = [], [], [], [], []
        for f, keep in ready:
            row0, sx, sy, fids = self._meta.pop(f)
            k = np.nonzero(keep)[0]
            counts.append(len(k))
            rows.append(row0 + k)
            ids.append(fids[k])
            sxs.append(np.full((len(k),), sx, np.float32))
            sys_.append(np.full((len(k),), sy, np.float32))
        total = sum(counts)
        lines = []
        if self.device_text:
            self._gather_text(ready, counts, rows, ids, sxs, sys_, t0)
            return
        if total:
            desc = ops.result_rows_desc(np.concatenate(rows), np.concatenate(ids), np.concatenate(sxs), np.concatenate(sys_))
            words_d = ops.result_rows_gather(self.ring_bd, self.ring_recs, desc, self.decoder.voc_size, upload=self.model._h2d)
            words = self.model._d2h(words_d)                     # waits for the launch: the slots may be rewritten afterwards
            self.gather_launches += 1
            dt = time.time() - t0
            self.time_cost["post_process"] += dt
            if not self._in_run:                                 # (a gather inside a step is inside `_run`'s window already)
                self.seconds += dt
            t0 = time.time()
            lines = results.finish_rows(words, self.decoder, self.min_extent)
            self.rows_seconds += time.time() - t0
        o, first = 0, len(self._out)
        for (f, _), c in zip(ready, counts):
            self._out.append((f, [r for r in lines[o:o + c] if r is not None]))
            o += c
        if self._atlas is not None:
            assert [f for f, _ in ready] == list(range(ready[0][0], ready[0][0] + len(ready))), "settled frames leave in frame order"
            self._draw(ready[0][0], [rows for _, rows in self._out[first:]])
        self._ring_tail = ready[-1][0] + 1
