"""Write tests/golden/score_overall.json: the OVERALL row that the reference's own vendored `motmetrics` computes
(`MetricsHost.compute_many(..., generate_overall=True)`) over several groupings of the sequences of tests/golden/score_mot.json.

    python tools/gen_golden_score_overall.py --reference <reference checkout>

CPU only.  The vendored copy (tools/Evaluation_Protocol_ArtVideo/motmetrics of the reference) is imported unmodified at
generation time, as tools/gen_golden_score.py does; only data is written: the names of each grouping's sequences, every
sequence's row and the OVERALL row.  `gomatching_amd.score_json.overall` is held to this file by tests/test_score_json_cpu.py.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["num_frames", "num_matches", "num_switches", "num_false_positives", "num_misses", "num_detections", "num_objects",
           "num_predictions", "num_unique_objects", "mostly_tracked", "partially_tracked", "mostly_lost", "idfp", "idfn", "idtp",
           "mota", "motp", "idf1", "idp", "idr", "precision", "recall"]
GROUPS = [
    ["identity_switch", "lost_and_refound", "more_hypotheses"],
    ["no_hypotheses", "random_sparse", "identity_switch"],
    ["random_sparse", "random_crowded", "random_flicker", "lost_and_refound"],
    ["no_hypotheses"],
    ["identity_switch", "lost_and_refound", "no_hypotheses", "more_hypotheses", "random_sparse", "random_crowded", "random_flicker"],
]


def accumulator(mm, frames):
    acc = mm.MOTAccumulator(auto_id=False)
    for fr in frames:
        d = np.full((len(fr["oids"]), len(fr["hids"])), np.nan)
        for i, j, v in fr["pairs"]:
            d[int(i), int(j)] = v
        acc.update(fr["oids"], fr["hids"], d, fr["frameid"])
    return acc


def plain(v):
    return int(v) if isinstance(v, (int, np.integer)) else float(v)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--sequences", default=os.path.join(ROOT, "tests", "golden", "score_mot.json"))
    ap.add_argument("--output", default=os.path.join(ROOT, "tests", "golden", "score_overall.json"))
    args = ap.parse_args()
    vendored = os.path.join(args.reference, "tools", "Evaluation_Protocol_ArtVideo")
    if not os.path.isdir(os.path.join(vendored, "motmetrics")):
        sys.exit("error: no vendored motmetrics under %s" % vendored)
    sys.modules.setdefault("xmltodict", types.ModuleType("xmltodict"))
    sys.path.insert(0, vendored)
    import motmetrics as mm
    assert mm.lap.default_solver == "scipy", mm.lap.default_solver
    with open(args.sequences) as f:
        seqs = {s["name"]: s["frames"] for s in json.load(f)["sequences"]}
    doc = {"metrics": METRICS, "groups": []}
    for names in GROUPS:
        summary = mm.metrics.create().compute_many([accumulator(mm, seqs[n]) for n in names], metrics=METRICS, names=names,
                                                   generate_overall=True)
        rows = {idx: {k: plain(summary.loc[idx, k]) for k in METRICS} for idx in summary.index}
        doc["groups"].append({"names": names, "rows": [rows[n] for n in names], "overall": rows["OVERALL"]})
        print(names, rows["OVERALL"])
    with open(args.output, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
