"""The host-side settler of the online session (gomatching_amd/online.py) against the offline rule: the rows it keeps are the
rows `_remove_short_track` keeps (`np.unique(..., return_counts=True)` over the WHOLE trace, ids with fewer than M detections
dropped), frames come out in order, no frame waits longer than max(M - 1, 0) * max(L - 1, 1) frames, `close()` flushes, and an
id that returns after its death raises.  No torch, no GPU."""
import numpy as np
import pytest

from gomatching_amd.online import TrackSettler

CASES = [(6, 5), (6, 1), (6, 0), (2, 5), (3, 4), (1, 5)]           # (test_len L, min_track_len M)


def make_trace(L, seed, frames=300):
    """Seeded id trace under the reach constraint: a track seen in frame s can only be seen again in a frame t <= s + R,
    R = max(L - 1, 1); ids are issued in increasing order.  Births (many of them short-lived), drop-outs inside the reach,
    deaths, and empty frames."""
    g = np.random.default_rng(seed)
    R = max(L - 1, 1)
    live = {}                                                      # id -> last frame seen
    next_id, out = 1, []
    for t in range(frames):
        if t % 41 == 17 or g.random() < 0.04:                      # an empty frame (tracks may survive it when R > 1)
            out.append(np.zeros((0,), np.int64))
            live = {i: s for i, s in live.items() if t - s < R}
            continue
        ids = []
        for i, s in list(live.items()):
            if t - s > R:                                          # out of reach: gone for good
                del live[i]
                continue
            p_die = 0.25 if i % 3 == 0 else 0.02                   # every third track is fragile: it mostly dies short
            if g.random() < p_die:
                del live[i]
                continue
            if t - s < R and g.random() < 0.25:                    # drops out of this frame, still within reach next frame
                continue
            ids.append(i)
            live[i] = t
        for _ in range(int(g.integers(0, 3)) if len(live) < 8 else 0):
            ids.append(next_id)
            live[next_id] = t
            next_id += 1
        g.shuffle(ids)
        out.append(np.asarray(ids, np.int64))
    return out


def offline_keep(trace, M):
    ids = np.concatenate(trace) if trace else np.zeros((0,), np.int64)
    uniq, counts = np.unique(ids, return_counts=True)
    short = uniq[counts < M]
    return [~np.isin(f, short) for f in trace]


def run(trace, L, M):
    s = TrackSettler(L, M)
    emitted, waits = [], []
    for t, ids in enumerate(trace):
        for f, keep in s.push(ids):
            emitted.append((f, keep))
            waits.append(t - f)
        assert s.pending == t + 1 - len(emitted)
    tail = s.close()
    for f, keep in tail:
        emitted.append((f, keep))
        waits.append(len(trace) - 1 - f)
    return s, emitted, waits, len(tail)


@pytest.mark.parametrize("L,M", CASES)
def test_settler_keeps_what_the_offline_rule_keeps(L, M):
    bound = max(M - 1, 0) * max(L - 1, 1)
    dropped = waited = tails = 0
    for seed in range(12):
        trace = make_trace(L, 100 * L + 10 * M + seed)
        want = offline_keep(trace, M)
        s, emitted, waits, n_tail = run(trace, L, M)
        assert s.latency_bound == bound
        assert [f for f, _ in emitted] == list(range(len(trace)))                 # every frame, once, in order
        for (f, keep), w in zip(emitted, want):
            assert keep.dtype == bool and np.array_equal(keep, w), (seed, f)
        assert max(waits) <= bound and s.max_wait == max(waits), (seed, max(waits), bound)
        assert s.rows_dropped == sum(int((~w).sum()) for w in want)
        dropped += s.rows_dropped
        waited += sum(1 for w in waits if w > 0)
        tails += n_tail
        assert s.close() == []
    if M > 1:                                                       # the traces do exercise removal and waiting
        assert dropped > 0 and waited > 0, (dropped, waited)
    else:                                                           # M <= 1 keeps every row and settles every frame at once
        assert dropped == 0 and waited == 0 and tails == 0


def test_settler_state_stays_bounded_on_a_long_stream():
    s = TrackSettler(6, 5)
    peak = 0
    for ids in make_trace(6, 3, frames=3000):
        s.push(ids)
        peak = max(peak, len(s._count), len(s._last), s.pending)
    assert peak <= 21 + 60, peak                                    # D + 1 pending frames; tracks of the last D + R frames


def test_close_flushes_open_tracks_as_dead():
    s = TrackSettler(6, 5)
    assert s.push([1, 2]) == [] and s.push([1, 2]) == [] and s.push([1]) == []
    out = s.close()
    assert [f for f, _ in out] == [0, 1, 2]
    assert all(not k.any() for _, k in out)                         # 3 and 2 detections: both tracks are short
    with pytest.raises(RuntimeError):
        s.push([1])


def test_confirmed_track_releases_its_past_frames():
    s = TrackSettler(6, 3)
    assert s.push([7]) == [] and s.push([7]) == []
    out = s.push([7])                                               # third detection: confirmed, frames 0..2 leave at once
    assert [f for f, _ in out] == [0, 1, 2] and all(k.all() for _, k in out)


def test_an_id_that_returns_after_its_death_raises():
    s = TrackSettler(3, 4)                                          # reach 2
    s.push([1, 2])
    s.push([2])
    s.push([2])                                                     # t = 2 >= s(1) + R: track 1 is dead
    with pytest.raises(RuntimeError, match=r"frame 3: id 1 "):
        s.push([1, 2])
    s = TrackSettler(3, 1)                                          # a dead id that was already forgotten (its frames left)
    for ids in ([1], [2], [2], [2], [2]):
        s.push(ids)
    assert 1 not in s._last
    with pytest.raises(RuntimeError, match=r"frame 5: id 1 "):
        s.push([1])
