"""Write tests/golden/score_mot.json: seeded synthetic tracking sequences (object ids, hypothesis ids and the sparse
distances of every frame) together with what the reference's own vendored `motmetrics` computes for them.

    python tools/gen_golden_score.py --reference <reference checkout>

CPU only.  The vendored copy (tools/Evaluation_Protocol_ArtVideo/motmetrics of the reference) is imported unmodified, with its
scipy solver; its `io` module wants `xmltodict`, which nothing used here calls, so an empty module of that name is put into
sys.modules first (this generator's own stub).  Only data is written: ids, distances and the metric values.
`gomatching_amd.score.MOTAccumulator` is held to this file by tests/test_score_cpu.py.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["num_frames", "num_matches", "num_switches", "num_false_positives", "num_misses", "num_detections", "num_objects",
           "num_predictions", "num_unique_objects", "mostly_tracked", "partially_tracked", "mostly_lost", "mota", "motp", "idf1",
           "idp", "idr", "precision", "recall"]


def hand_sequences():
    """Each frame: (frame id, object ids, hypothesis ids, [(i, j, distance)])."""
    seqs = {}
    # two objects whose hypotheses swap in frame 3: two identity switches
    seqs["identity_switch"] = [
        (1, [1, 2], [10, 20], [(0, 0, 0.1), (1, 1, 0.2)]),
        (2, [1, 2], [10, 20], [(0, 0, 0.15), (1, 1, 0.25)]),
        (3, [1, 2], [10, 20], [(0, 1, 0.3), (1, 0, 0.35)]),
        (4, [1, 2], [10, 20], [(0, 1, 0.1), (1, 0, 0.1)]),
    ]
    # object 1 is lost for two frames (its hypothesis is there but too far), then found again by the same hypothesis; object 2
    # is lost for a frame without hypotheses and found again by another one (a switch after the gap); frame 5 has no ground truth
    seqs["lost_and_refound"] = [
        (1, [1, 2], [10, 20], [(0, 0, 0.2), (1, 1, 0.3)]),
        (2, [1, 2], [10, 20], [(1, 1, 0.3)]),
        (3, [1, 2], [10], []),
        (4, [1, 2], [], []),
        (5, [], [10, 30], []),
        (6, [1, 2], [10, 30], [(0, 0, 0.25), (1, 1, 0.4)]),
        (8, [1, 2], [10, 30], [(0, 0, 0.25), (0, 1, 0.05), (1, 1, 0.45)]),
    ]
    # no hypothesis in the whole video
    seqs["no_hypotheses"] = [(k, [1, 2, 3][:1 + k % 3], [], []) for k in range(1, 7)]
    # more hypotheses than objects, with competing candidates and equal distances
    seqs["more_hypotheses"] = [
        (1, [5], [1, 2, 3, 4], [(0, 1, 0.3), (0, 2, 0.3), (0, 3, 0.4)]),
        (2, [5, 6], [1, 2, 3, 4, 7], [(0, 2, 0.2), (0, 1, 0.1), (1, 1, 0.1), (1, 4, 0.45)]),
        (3, [5, 6], [2, 3, 7], [(0, 0, 0.3), (1, 0, 0.2), (1, 2, 0.2), (0, 1, 0.35)]),
        (4, [6], [2, 3, 7, 8, 9], [(0, 3, 0.05)]),
    ]
    return seqs


def random_sequence(rng, frames, max_obj, extra_hyp, p_seen, p_swap):
    """Objects with persistent ids enter and leave; each is followed by a hypothesis that is sometimes missing, sometimes
    replaced by a new id or swapped with a neighbour's; spurious hypotheses and spurious finite distances are added."""
    next_o, next_h = 1, 100
    alive = {}                                                   # object -> its hypothesis
    out = []
    fid = 0
    for _ in range(frames):
        fid += 1 + int(rng.rand() < 0.1)
        for o in list(alive):
            if rng.rand() < 0.08:
                del alive[o]
        while len(alive) < max_obj and rng.rand() < 0.5:
            alive[next_o] = next_h
            next_o, next_h = next_o + 1, next_h + 1
        if rng.rand() < 0.06:
            out.append((fid, [], [int(h) for h in rng.permutation(list(alive.values()))[:2]], []))
            continue
        keys = list(alive)
        if len(keys) >= 2 and rng.rand() < p_swap:
            a, b = rng.choice(len(keys), 2, replace=False)
            alive[keys[a]], alive[keys[b]] = alive[keys[b]], alive[keys[a]]
        oids = [int(o) for o in rng.permutation(keys)]
        hids, pairs = [], []
        if rng.rand() >= 0.06:
            for o in oids:
                if rng.rand() < 0.05:
                    alive[o] = next_h
                    next_h += 1
                if rng.rand() < p_seen:
                    hids.append(alive[o])
            for _ in range(rng.randint(0, extra_hyp + 1)):
                hids.append(next_h)
                next_h += 1
            hids = [int(h) for h in rng.permutation(hids)]
            for i, o in enumerate(oids):
                for j, h in enumerate(hids):
                    if h == alive[o] and rng.rand() < 0.92:
                        pairs.append((i, j, float(np.round(rng.uniform(0.0, 0.5), 6))))
                    elif rng.rand() < 0.08:
                        pairs.append((i, j, float(np.round(rng.uniform(0.2, 0.5), 6))))
        out.append((fid, oids, hids, pairs))
    return out


def reference_metrics(mm, frames):
    acc = mm.MOTAccumulator(auto_id=False)
    for fid, oids, hids, pairs in frames:
        d = np.full((len(oids), len(hids)), np.nan)
        for i, j, v in pairs:
            d[i, j] = v
        acc.update(oids, hids, d, fid)
    res = mm.metrics.create().compute(acc, metrics=METRICS, return_dataframe=False)
    out = {}
    for k in METRICS:
        v = res[k]
        out[k] = int(v) if isinstance(v, (int, np.integer)) else float(v)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--output", default=os.path.join(ROOT, "tests", "golden", "score_mot.json"))
    args = ap.parse_args()
    vendored = os.path.join(args.reference, "tools", "Evaluation_Protocol_ArtVideo")
    if not os.path.isdir(os.path.join(vendored, "motmetrics")):
        sys.exit("error: no vendored motmetrics under %s" % vendored)
    sys.modules.setdefault("xmltodict", types.ModuleType("xmltodict"))
    sys.path.insert(0, vendored)
    import motmetrics as mm
    assert mm.lap.default_solver == "scipy", mm.lap.default_solver
    seqs = hand_sequences()
    rng = np.random.RandomState(7)
    seqs["random_sparse"] = random_sequence(rng, 40, 4, 1, 0.9, 0.05)
    seqs["random_crowded"] = random_sequence(rng, 60, 9, 3, 0.8, 0.15)
    seqs["random_flicker"] = random_sequence(rng, 50, 6, 2, 0.55, 0.1)
    doc = {"metrics": METRICS, "sequences": []}
    for name, frames in seqs.items():
        exp = reference_metrics(mm, frames)
        doc["sequences"].append({"name": name, "expected": exp,
                                 "frames": [{"frameid": f, "oids": o, "hids": h, "pairs": [list(p) for p in pr]}
                                            for f, o, h, pr in frames]})
        print(name, exp)
    with open(args.output, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
