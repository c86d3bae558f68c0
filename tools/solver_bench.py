"""Times the fused clipped-AdamW step (csrc/optim.hip) against torch.optim.AdamW (its default multi-tensor path) +
clip_grad_norm_ on the same tensors, at the head sizes of the full icdar15 (LSTMatcher) and pp_dstext (SHA_FFN_CRSATTN) configs.
One process, the two alternating, device events around STEPS steps after a warm-up, REPEATS repeats; prints microseconds per
step (median and min..max over the repeats) and the fused step's achieved bytes per second, counted as 36 B per parameter
(g twice, p m v read and written) against 8 TB/s.  Then the split of one `Trainer.step` on the test suite's small clip.

    python tools/solver_bench.py [--steps 300] [--repeats 5] > profiles/solver_bench.log

`--dropout P`: instead of all that, the cost of MODEL.ASSO_HEAD.DROPOUT = P in the head's forward and backward on that clip:
one process, one model, the trainer's dropout state switched between 0 and P from repeat to repeat (alternating), the split's
own repeats, with the bytes the dropout passes move.

    python tools/solver_bench.py --dropout 0.1 > profiles/dropout_bench.log
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gomatching_amd import solver  # noqa: E402
from gomatching_amd.config import setup_cfg  # noqa: E402
from gomatching_amd.weights import canonical_keys, synth_state_dict  # noqa: E402

DEV = "cuda"


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def bench_head(builtin, steps, repeats):
    cfg = setup_cfg(builtin=builtin)
    shapes = [tuple(s) for k, s in canonical_keys(cfg).items() if k.startswith("roi_heads.")]
    n = sum(int(np.prod(s)) for s in shapes)
    gen = torch.Generator(device=DEV).manual_seed(0)
    mine = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen) * 0.05) for s in shapes]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    for p, q in zip(mine, theirs):
        p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
        q.grad = p.grad.clone()
    fused = solver.ClippedAdamW([{"params": [p]} for p in mine], lr=5e-5, weight_decay=1e-4, clip_value=0.1)
    ref = torch.optim.AdamW([{"params": [p]} for p in theirs], lr=5e-5, weight_decay=1e-4)
    keep = [q.grad.clone() for q in theirs]

    def torch_step():
        for q, g in zip(theirs, keep):                            # clip_grad_norm_ scales in place: hand it the same gradient again
            q.grad = g                                            # (no copy: after the first step coef ~ 1 of an already clipped g)
        torch.nn.utils.clip_grad_norm_(theirs, 0.1)
        ref.step()
    for _ in range(20):
        fused.step()
        torch_step()
    torch.cuda.synchronize()
    f, t = [], []
    for _ in range(repeats):
        f.append(timed(fused.step, steps))
        t.append(timed(torch_step, steps))
    fm, tm = statistics.median(f), statistics.median(t)
    print("%-10s %2d tensors %6.2f M parameters, %d steps x %d repeats" % (builtin, len(shapes), n / 1e6, steps, repeats))
    print("  fused clipped AdamW         %8.1f us/step  (min %.1f .. max %.1f)   %.2f TB/s at 36 B/parameter = %.0f %% of 8 TB/s" % (
        fm, min(f), max(f), 36.0 * n / fm / 1e6, 100 * 36.0 * n / fm / 1e6 / 8.0))
    print("  torch AdamW + clip_grad_norm_ %6.1f us/step  (min %.1f .. max %.1f)" % (tm, min(t), max(t)))
    verdict = "faster beyond the spread" if max(f) < min(t) else ("slower beyond the spread" if min(f) > max(t) else "within the spread")
    print("  fused / torch = %.2f: the fused step is %s" % (fm / tm, verdict))
    return fm, tm


def trainer_split():
    """One Trainer.step on the suite's 4-frame 96x128 clip (mini icdar15: 16 queries; the head has its full 32.8 M parameters)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import mini_cfg
    from gomatching_amd import training
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip
    cfg = mini_cfg("icdar15", device="cuda")
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    cfg.SOLVER.WARMUP_ITERS = 0
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    batch = make_training_clip()
    tr = solver.Trainer(cfg, model, None)
    for _ in range(3):
        tr.step(batch)
    sync = torch.cuda.synchronize
    det, fwd, bwd, opt = [], [], [], []
    for _ in range(10):
        sync(); t0 = time.perf_counter()
        with torch.no_grad():
            raw, kind = model._raw_input(batch)
            feats = model.backbone.forward(model._normalise(raw, kind))
            model.detection_transformer.forward([feats[k] for k in model.feature_names])
        sync(); t1 = time.perf_counter()
        losses = training.forward_losses(model, batch)
        total = sum(losses.values())
        sync(); t2 = time.perf_counter()
        tr.optimizer.zero_grad()
        total.backward()
        sync(); t3 = time.perf_counter()
        tr.optimizer.step()
        sync(); t4 = time.perf_counter()
        det.append(t1 - t0); fwd.append(t2 - t1 - (t1 - t0)); bwd.append(t3 - t2); opt.append(t4 - t3)
    ms = lambda x: 1e3 * statistics.median(x)
    print("Trainer.step split, 4 frames of 96x128, %d queries, 32.8 M trainable parameters (median of 10, host-synchronised):" % cfg.MODEL.TRANSFORMER.NUM_QUERIES)
    print("  frozen detector forward %.2f ms | head forward + losses (host target logic included) %.2f ms | backward %.2f ms | "
          "optimizer step %.2f ms" % (ms(det), ms(fwd), ms(bwd), ms(opt)))
    print("  (the head figure is forward_losses minus the stand-alone detector time: it assumes the detector costs the same inside it)")
    model.close()


def dropout_cost(p, repeats=10, rounds=5):
    """Head forward and backward of the split's clip with dropout 0 and `p`, alternating in one process on one model."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import mini_cfg
    from gomatching_amd import ops, training
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip
    cfg = mini_cfg("icdar15", device="cuda")
    cfg.MODEL.ASSO_HEAD.DROPOUT = p
    cfg.SOLVER.WARMUP_ITERS = 0
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    batch = make_training_clip()
    tr = solver.Trainer(cfg, model, None, seed=7)
    state = tr.dropout
    sync = torch.cuda.synchronize
    # bytes of the dropout passes, counted where they are launched (fp32; forward and backward)
    count = {"bytes": 0, "launches": 0}
    orig = (ops.dropout, ops.softmax_dropout_rows_, ops.softmax_dropout_rows_backward, ops.relu_backward_scaled)

    def counted(fn, per_element):
        def run(x, *a, **k):
            count["bytes"] += 4 * per_element(x, k) * x.numel()
            count["launches"] += 1
            return fn(x, *a, **k)
        return run
    ops.dropout = counted(orig[0], lambda x, k: 3 if k.get("residual") is not None else 2)
    ops.softmax_dropout_rows_ = counted(orig[1], lambda x, k: 3)             # read scores, write P and P~ (the softmax alone: 2)
    ops.softmax_dropout_rows_backward = counted(orig[2], lambda x, k: 5)     # P and dP~ read in both passes, dS written (as without)
    ops.relu_backward_scaled = counted(orig[3], lambda x, k: 3)              # as relu_backward

    def one(with_dropout):
        model.dropout_state = state if with_dropout else None
        if with_dropout:
            state.begin_forward(0)
        sync(); t0 = time.perf_counter()
        with torch.no_grad():
            raw, kind = model._raw_input(batch)
            feats = model.backbone.forward(model._normalise(raw, kind))
            model.detection_transformer.forward([feats[k] for k in model.feature_names])
        sync(); t1 = time.perf_counter()
        losses = training.forward_losses(model, batch)
        total = sum(losses.values())
        sync(); t2 = time.perf_counter()
        tr.optimizer.zero_grad()
        total.backward()
        sync(); t3 = time.perf_counter()
        return 1e3 * (t2 - t1 - (t1 - t0)), 1e3 * (t3 - t2)
    for _ in range(3):
        one(False), one(True)
    count["bytes"] = count["launches"] = 0
    one(True)
    nbytes, launches = count["bytes"], count["launches"]
    ops.dropout, ops.softmax_dropout_rows_, ops.softmax_dropout_rows_backward, ops.relu_backward_scaled = orig
    print("dropout cost, head forward + losses | backward on 4 frames of 96x128, %d queries (median of %d, host-synchronised), "
          "%d rounds alternating P = 0 / P = %g:" % (cfg.MODEL.TRANSFORMER.NUM_QUERIES, repeats, rounds, p))
    meds = {False: [], True: []}
    for r in range(rounds):
        for flag in (False, True):
            runs = [one(flag) for _ in range(repeats)]
            f, b = statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs)
            meds[flag].append((f, b))
            print("  round %d  P = %-4g forward %.2f ms   backward %.2f ms" % (r, p if flag else 0, f, b))
    for flag in (False, True):
        f, b = [x[0] for x in meds[flag]], [x[1] for x in meds[flag]]
        print("  P = %-4g forward %.2f ms (%.2f .. %.2f)   backward %.2f ms (%.2f .. %.2f)" % (
            p if flag else 0, statistics.median(f), min(f), max(f), statistics.median(b), min(b), max(b)))
    df = statistics.median(x[0] for x in meds[True]) - statistics.median(x[0] for x in meds[False])
    db = statistics.median(x[1] for x in meds[True]) - statistics.median(x[1] for x in meds[False])
    print("  added by P = %g: forward %+.2f ms, backward %+.2f ms; the dropout launches of one step (%d) move %.2f MB, "
          "%.1f us at 5.7 TB/s" % (p, df, db, launches, nbytes / 1e6, nbytes / 5.7e6))
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--dropout", type=float, default=None, metavar="P",
                    help="measure the head's forward / backward with MODEL.ASSO_HEAD.DROPOUT 0 and P, alternating, and nothing else")
    a = ap.parse_args()
    print("solver_bench: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if a.dropout is not None:
        dropout_cost(a.dropout)
        return
    for builtin in ("icdar15", "pp_dstext"):
        bench_head(builtin, a.steps, a.repeats)
    if not a.no_split:
        trainer_split()


if __name__ == "__main__":
    main()
