"""GPU: the fused full-model-clipped AdamW step (csrc/optim.hip behind gomatching_amd/solver.py::ClippedAdamW) against the
float64 statement (tests/solver_statement.py) with bounds taken from the REFERENCE optimizer's own fp32 error
(tests/golden/solver_adamw.npz), its reproducibility, the trainer loop, and inference with the trained head.

The rule of every comparison with the statement, per tensor and per quantity (p, exp_avg, exp_avg_sq):
    max |gpu - f64| <= 2 x (max |reference fp32 - f64|) + one fp32 spacing at the largest magnitude
(another correct fp32 evaluation order errs by as much as torch's, with independent sign)."""
import os

import numpy as np
import pytest
import torch

import solver_statement as S
from helpers import mini_cfg, golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHAIN = 25                    # longest chain of fp32 additions in the norm reduction, as stated in csrc/optim.hip


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fixture_optimizer(g, params=None):
    from gomatching_amd.solver import ClippedAdamW
    n = int(g["n_tensors"])
    if params is None:
        params = [torch.nn.Parameter(torch.from_numpy(g["init_%d" % i].copy()).to(DEV)) for i in range(n)]
    opt = ClippedAdamW([{"params": [p]} for p in params], lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]),
                       eps=float(g["eps"]), weight_decay=float(g["weight_decay"]), clip_value=float(g["clip_value"]))
    return params, opt


def _run(g, params, opt, first, last, norms=None):
    for step in range(first, last):
        for p, x in zip(params, S.fixture_gradients(int(g["seed"]), step)):
            p.grad = None if x is None else torch.from_numpy(x).to(DEV)
        opt.step()
        if norms is not None:
            norms.append(opt._norm.clone())


def _check_against_statement(name, got, want64, ref_err):
    err = float(np.max(np.abs(got.astype(np.float64) - want64))) if got.size else 0.0
    bound = 2.0 * ref_err + S.spacing(want64)
    print("%-28s max|gpu - f64| %.3e   reference's %.3e   bound %.3e" % (name, err, ref_err, bound))
    return err <= bound, (name, err, ref_err, bound)


def test_fixture_steps_match_the_statement_within_twice_the_reference_error():
    g = golden("solver_adamw.npz")
    p64, m64, v64, t64, totals, coefs = S.run_statement(g)
    params, opt = _fixture_optimizer(g)
    norms = []
    _run(g, params, opt, 0, S.STEPS, norms)
    torch.cuda.synchronize()
    failures = []
    for i, p in enumerate(params):
        st = opt.state[p]
        assert int(st["step"]) == t64[i] == int(g["ref_step_%d" % i])
        for name, got, want in (("p", p, p64[i]), ("exp_avg", st["exp_avg"], m64[i]), ("exp_avg_sq", st["exp_avg_sq"], v64[i])):
            ok, info = _check_against_statement("tensor %d %s" % (i, name), got.detach().cpu().numpy(), want,
                                                float(g["ref_err_%s_%d" % (name, i)]))
            if not ok:
                failures.append(info)
    assert not failures, failures
    # the reported total norm of every step: (chain + 2) x 2^-24 relative; the coefficient follows from it in fp32
    got = torch.stack(norms).cpu().numpy().astype(np.float64)
    for step in range(S.STEPS):
        rel = abs(got[step, 0] - totals[step]) / totals[step]
        print("step %2d  total %.9g  f64 %.17g  rel %.3e   coef %.9g" % (step, got[step, 0], totals[step], rel, got[step, 1]))
        assert rel <= (CHAIN + 2) * 2.0 ** -24, (step, rel)
        assert (got[step, 1] < 1.0) == (coefs[step] < 1.0) and abs(got[step, 1] - coefs[step]) <= 4 * 2.0 ** -24 * coefs[step] + (CHAIN + 2) * 2.0 ** -24
    assert opt.grad_norm() == float(got[-1, 0]) and opt.clip_coefficient() == float(got[-1, 1])
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gomatching_amd", "csrc", "optim.hip")).read()
    assert "16 + 6 + 3 = 25" in src                              # the chain length this test's bound is built from


def test_tensor_without_gradient_is_not_touched_and_the_others_do_not_notice():
    from gomatching_amd.solver import ClippedAdamW
    gen = torch.Generator().manual_seed(3)
    shapes = [(33, 7), (4100,), (64,)]
    init = [torch.randn(s, generator=gen) * 0.1 for s in shapes]
    grads = [[torch.randn(s, generator=gen) * 0.01 for s in shapes] for _ in range(3)]

    def make(idx):
        ps = [torch.nn.Parameter(init[i].clone().to(DEV)) for i in idx]
        return ps, ClippedAdamW([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in zip(idx, ps)], weight_decay=0.01, clip_value=0.05)
    ps, opt = make([0, 1, 2])
    for p, x in zip(ps, grads[0]):
        p.grad = x.to(DEV)
    opt.step()
    before = [t.clone() for t in (ps[1], opt.state[ps[1]]["exp_avg"], opt.state[ps[1]]["exp_avg_sq"])]
    for k in (1, 2):                                             # two steps with tensor 1 absent
        ps[0].grad, ps[1].grad, ps[2].grad = grads[k][0].to(DEV), None, grads[k][2].to(DEV)
        opt.step()
    torch.cuda.synchronize()
    st = opt.state[ps[1]]
    assert int(st["step"]) == 1 and int(opt.state[ps[0]]["step"]) == 3
    for a, b in zip(before, (ps[1], st["exp_avg"], st["exp_avg_sq"])):
        assert _same_bits(a, b)
    # the same three steps with tensor 1 absent from the optimizer after the first step: tensors 0 and 2 get the same bits
    qs, other = make([0, 1, 2])
    for p, x in zip(qs, grads[0]):
        p.grad = x.to(DEV)
    other.step()
    two = ClippedAdamW([{"params": [qs[0]], "lr": 1e-3}, {"params": [qs[2]], "lr": 3e-3}], weight_decay=0.01, clip_value=0.05)
    for q in (qs[0], qs[2]):
        two.state[q] = other.state[q]
    for k in (1, 2):
        qs[0].grad, qs[2].grad = grads[k][0].to(DEV), grads[k][2].to(DEV)
        two.step()
    torch.cuda.synchronize()
    for a, b in ((ps[0], qs[0]), (ps[2], qs[2])):
        assert _same_bits(a, b) and _same_bits(opt.state[a]["exp_avg"], two.state[b]["exp_avg"])
        assert _same_bits(opt.state[a]["exp_avg_sq"], two.state[b]["exp_avg_sq"])
    assert _same_bits(opt._norm, two._norm)


@pytest.mark.parametrize("layout", ["params_and_grads_off_by_one", "all_four_off_by_one", "every_array_its_own_offset"])
def test_odd_sizes_and_misaligned_views_give_the_bits_of_aligned_tensors(layout):
    """Sizes 1, 3, 5, 1031 (and two that cross the 4096-element chunk) as views that start one element (or 1, 2, 3, 0 elements)
    into their storage: every output bit equals that of the same values in separately allocated, aligned tensors."""
    from gomatching_amd.solver import ClippedAdamW
    sizes = [1, 3, 5, 1031, 4101, 8195]
    offs = {"params_and_grads_off_by_one": (1, 1, 0, 0), "all_four_off_by_one": (1, 1, 1, 1), "every_array_its_own_offset": (1, 2, 3, 0)}[layout]
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(n, generator=gen) * 0.1 for n in sizes]
    grads = [[torch.randn(n, generator=gen) * (0.02 if k == 0 else 2e-4) for n in sizes] for k in range(2)]   # one clipped, one unclipped step

    def view(n, off):
        t = torch.zeros(n + 8, device=DEV)[off:off + n]
        assert t.data_ptr() % 16 == (4 * off) % 16 and t.is_contiguous()
        return t

    def run(o):
        ps = []
        for x, n in zip(init, sizes):
            p = torch.nn.Parameter(view(n, o[0]))
            p.data.copy_(x)
            ps.append(p)
        opt = ClippedAdamW([{"params": [p]} for p in ps], lr=1e-3, weight_decay=0.01, clip_value=0.1)
        for p, n in zip(ps, sizes):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view(n, o[2]), "exp_avg_sq": view(n, o[3])}
        norms = []
        for k in range(2):
            for p, x, n in zip(ps, grads[k], sizes):
                gbuf = view(n, o[1])
                gbuf.copy_(x)
                p.grad = gbuf
            opt.step()
            norms.append(opt._norm.clone())
        torch.cuda.synchronize()
        return ps, opt, norms
    a_ps, a_opt, a_norms = run((0, 0, 0, 0))
    b_ps, b_opt, b_norms = run(offs)
    assert float(a_norms[0][1]) < 1.0 and float(a_norms[1][1]) == 1.0
    for x, y in zip(a_norms, b_norms):
        assert _same_bits(x, y)
    for n, a, b in zip(sizes, a_ps, b_ps):
        assert _same_bits(a, b), (layout, n)
        assert _same_bits(a_opt.state[a]["exp_avg"], b_opt.state[b]["exp_avg"]), (layout, n)
        assert _same_bits(a_opt.state[a]["exp_avg_sq"], b_opt.state[b]["exp_avg_sq"]), (layout, n)
        assert not torch.equal(a.detach().cpu(), init[sizes.index(n)])


def test_two_runs_and_a_resumed_run_give_the_same_bits():
    g = golden("solver_adamw.npz")
    runs = []
    for _ in range(2):
        params, opt = _fixture_optimizer(g)
        norms = []
        _run(g, params, opt, 0, S.STEPS, norms)
        runs.append((params, opt, norms))
    # save after step 6, load into a fresh optimizer over fresh parameters, steps 7-12
    params, opt = _fixture_optimizer(g)
    _run(g, params, opt, 0, 6)
    saved = {"optimizer": opt.state_dict(), "params": [p.detach().cpu().clone() for p in params]}
    fresh = [torch.nn.Parameter(x.clone().to(DEV)) for x in saved["params"]]
    fresh, opt2 = _fixture_optimizer(g, fresh)
    opt2.load_state_dict(saved["optimizer"])
    assert all(opt2.state[p]["exp_avg"].device.type == "cuda" and opt2.state[p]["step"].device.type == "cpu" for p in fresh)
    norms2 = []
    _run(g, fresh, opt2, 6, S.STEPS, norms2)
    torch.cuda.synchronize()
    (p1, o1, n1), (p2, o2, n2) = runs
    for i in range(len(p1)):
        for other_p, other_o in ((p2, o2), (fresh, opt2)):
            assert _same_bits(p1[i], other_p[i]), i
            assert int(o1.state[p1[i]]["step"]) == int(other_o.state[other_p[i]]["step"])
            for k in ("exp_avg", "exp_avg_sq"):
                assert _same_bits(o1.state[p1[i]][k], other_o.state[other_p[i]][k]), (i, k)
    for a, b in zip(n1, n2):
        assert _same_bits(a, b)
    for a, b in zip(n1[6:], norms2):
        assert _same_bits(a, b)


def _against_torch_on_the_cpu(tag, keys, opt, gpu, init, lr, wd, clip, scales):
    """Steps of seeded gradients (one scale per step) through `opt` on the GPU, torch.optim.AdamW + clip_grad_norm_ on CPU
    tensors and the float64 statement; the 2 x rule with torch's own error as the reference error, and the norm bound."""
    gen = torch.Generator().manual_seed(6)
    cpu = [torch.nn.Parameter(x.clone()) for x in init]
    ref = torch.optim.AdamW([{"params": [p]} for p in cpu], lr=lr, weight_decay=wd)
    p64 = [x.numpy().astype(np.float64) for x in init]
    m64, v64, t64 = [np.zeros_like(x) for x in p64], [np.zeros_like(x) for x in p64], [0] * len(p64)
    clipped = []
    for step, scale in enumerate(scales):
        grads = [torch.randn(s, generator=gen) * scale for _, s in keys]
        for p, q, x in zip(gpu, cpu, grads):
            p.grad, q.grad = x.to(DEV), x.clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_(cpu, clip)
        ref.step()
        tot, coef = S.clipped_adamw_step_f64(p64, [x.numpy() for x in grads], m64, v64, t64, [lr] * len(p64), [wd] * len(p64),
                                             (0.9, 0.999), 1e-8, clip)
        clipped.append(coef < 1.0)
        rel = abs(opt.grad_norm() - tot) / tot
        print("%s step %d: total %.9g (f64 %.12g, rel %.2e), coef %.6g" % (tag, step, opt.grad_norm(), tot, rel, coef))
        assert rel <= (CHAIN + 2) * 2.0 ** -24
    failures = []
    for i, (k, _) in enumerate(keys):
        for name, got, r, want in (("p", gpu[i], cpu[i], p64[i]), ("exp_avg", opt.state[gpu[i]]["exp_avg"], ref.state[cpu[i]]["exp_avg"], m64[i]),
                                   ("exp_avg_sq", opt.state[gpu[i]]["exp_avg_sq"], ref.state[cpu[i]]["exp_avg_sq"], v64[i])):
            ref_err = float(np.max(np.abs(r.detach().numpy().astype(np.float64) - want)))
            ok, info = _check_against_statement("%s %s" % (k, name), got.detach().cpu().numpy(), want, ref_err)
            if not ok:
                failures.append(info)
    assert not failures, failures
    return clipped


@pytest.mark.parametrize("builtin", ["icdar15", "pp_dstext"])
def test_real_head_sizes_within_twice_the_error_of_torch_adamw(builtin):
    """Every `roi_heads.*` tensor of the full config, 3 steps (clipped, clipped, unclipped) of seeded gradients.  The reference
    error is measured in this test: torch.optim.AdamW + clip_grad_norm_ on CPU tensors against the numpy float64 statement."""
    from gomatching_amd.config import setup_cfg
    from gomatching_amd.solver import build_optimizer, solver_cfg
    from gomatching_amd.weights import canonical_keys
    cfg = setup_cfg(builtin=builtin)
    keys = [(k, tuple(s)) for k, s in canonical_keys(cfg).items() if k.startswith("roi_heads.")]
    total = sum(int(np.prod(s)) for _, s in keys)
    assert total == {"icdar15": 32794881, "pp_dstext": 11802624}[builtin] and any(int(np.prod(s)) == 1 for _, s in keys) == bool(cfg.MODEL.ROI_HEADS.WITH_RESR)
    S_ = solver_cfg(cfg)
    lr, wd, clip = S_.BASE_LR, S_.WEIGHT_DECAY, S_.CLIP_GRADIENTS.CLIP_VALUE
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) * 0.05 for _, s in keys]
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    opt = build_optimizer(cfg, [(k, p) for (k, _), p in zip(keys, gpu)])
    assert len(opt.param_groups) == len(keys) and opt.clip_value == clip
    assert _against_torch_on_the_cpu(builtin, keys, opt, gpu, init, lr, wd, clip, (1e-3, 1e-3, 1e-6)) == [True, True, False]


def test_a_table_of_more_tensors_than_one_launch_takes():
    """110 tensors of mixed sizes: the table is split into three launches of at most 48 tensors (csrc/optim.hip), the later ones
    starting at a non-zero chunk number; sizes from 1 element to a few chunks, some not multiples of 4.  Same rule as at the real
    head sizes; the reported norm covers all three launches' partials."""
    from gomatching_amd.solver import ClippedAdamW
    sizes = [(1 + (37 * i * i + 11 * i) % 9000,) for i in range(110)]
    assert len(sizes) > 2 * 48 and min(s[0] for s in sizes) < 4 and max(s[0] for s in sizes) > 2 * 4096 and any(s[0] % 4 for s in sizes)
    keys = [("t%03d" % i, s) for i, s in enumerate(sizes)]
    gen = torch.Generator().manual_seed(8)
    init = [torch.randn(s, generator=gen) * 0.05 for _, s in keys]
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in init]
    opt = ClippedAdamW([{"params": [p]} for p in gpu], lr=1e-3, weight_decay=0.01, clip_value=0.1)
    assert _against_torch_on_the_cpu("110 tensors", keys, opt, gpu, init, 1e-3, 0.01, 0.1, (1e-2, 1e-5, 1e-2)) == [True, False, True]


def _trainer_setup(tmp_path, base_lr):
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.solver import Trainer
    from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip
    from gomatching_amd.weights import synth_state_dict
    cfg = mini_cfg("icdar15", device="cuda")
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.0
    cfg.SOLVER.WARMUP_ITERS = 0
    cfg.SOLVER.BASE_LR = base_lr
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    batch = make_training_clip()
    return cfg, sd, model, Trainer(cfg, model, str(tmp_path)), batch


def test_trainer_lowers_the_loss_on_one_clip(tmp_path):
    """`Trainer` on the mini config and the synthetic clip of test_wrapper_forward_returns_the_loss_dict_and_trains_only_the_head
    (DROPOUT 0, WARMUP_ITERS 0): BASE_LR 2e-4, N = 8 steps on the same clip; every loss finite, the last total below the first.

    BASE_LR and N were chosen on the CPU (tools/solver_rehearsal.py: the losses of oracle/train_oracle.py on the CPU detector,
    torch.optim.AdamW + clip_grad_norm_(0.1)); that rehearsal's totals, steps 0..8:
        1057.19, 137.88, 508.61, 149.09, 103.45, 58.51, 13.99, 24.80, 5.06      (BASE_LR 2e-4; not monotone, 200x down at the end)
        1057.19, 346.28,  12.56, 189.76, 124.64, 59.68, 66.49, 44.61, 52.66     (BASE_LR 5e-5: 20x down)
    (the synthetic weights give association logits in the hundreds, hence the size of the first losses).  Then `save()`, and
    `eval.load_weights` of the file gives a model state whose head equals the trained one and whose detector is untouched."""
    from gomatching_amd import eval as gom_eval
    cfg, sd, model, trainer, batch = _trainer_setup(tmp_path, 2e-4)
    assert torch.equal(trainer.params["roi_heads.rescoring_head.weight"].cpu(), sd["detection_transformer.ctrl_point_class.0.weight"])
    assert len(trainer.optimizer.param_groups) == len(trainer.params)
    history = []
    for _ in range(9):
        history.append(trainer.step(batch))
        print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in history[-1].items()})
    for h in history:
        assert {"loss_long_asso", "loss_short_asso", "loss_res", "total_loss", "lr", "grad_norm", "iteration"} <= set(h)
        assert all(np.isfinite(h[k]) for k in h)
        assert h["lr"] == pytest.approx(2e-4 * 0.5 * (1 + np.cos(np.pi * (h["iteration"] - 1) / 30000)), rel=1e-12)
    assert history[-1]["total_loss"] < history[0]["total_loss"]           # the loss before the 9th step = after 8 steps
    path = trainer.save("model_final.pth")
    got = gom_eval.load_weights(path)
    for k, p in trainer.params.items():
        assert torch.equal(got[k], p.detach().cpu()), k
    assert not torch.equal(got["roi_heads.asso_head.fc1.weight"], torch.as_tensor(sd["roi_heads.asso_head.fc1.weight"]))
    for k, v in sd.items():
        if not k.startswith("roi_heads."):
            assert torch.equal(got[k], torch.as_tensor(v)), k
    # resume: a fresh trainer continues at the saved iteration with the saved moments
    cfg2, _, model2, trainer2, _ = _trainer_setup(tmp_path, 2e-4)
    assert trainer2.resume() == trainer.iteration == 9
    k0 = "roi_heads.asso_head.fc1.weight"
    assert torch.equal(trainer2.params[k0].cpu(), trainer.params[k0].cpu())
    for k, p in trainer.params.items():
        assert _same_bits(p, trainer2.params[k]), k
        for name in ("exp_avg", "exp_avg_sq"):
            assert _same_bits(trainer.optimizer.state[p][name], trainer2.optimizer.state[trainer2.params[k]][name]), (k, name)
        assert int(trainer.optimizer.state[p]["step"]) == int(trainer2.optimizer.state[trainer2.params[k]]["step"]) >= 1
    a, b = trainer.step(batch), trainer2.step(batch)
    assert a["lr"] == b["lr"] and a["iteration"] == b["iteration"] == 10 and np.isfinite(b["total_loss"])
    assert abs(a["total_loss"] - b["total_loss"]) <= 1e-3 * max(1.0, abs(a["total_loss"]))     # same weights, same clip
    model.close()
    model2.close()


def test_load_head_runs_inference_with_the_trained_head(tmp_path):
    """After training steps, `load_head` gives `batch_inference` the ids, texts and box bits of a `GoMatching` built from
    scratch with the same weights; the association scores differ from the untrained model's."""
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.predictor import new_time_cost
    from gomatching_amd.synth import make_clip
    cfg, sd, model, trainer, batch = _trainer_setup(tmp_path, 2e-4)
    frames = [{"image": torch.as_tensor(f.astype("float32").transpose(2, 0, 1)), "height": 96, "width": 128}
              for f in make_clip(6, 96, 128, clip_id=2)]

    def track(m):
        insts, idc = m.batch_inference(frames, 0, 0, [], new_time_cost())
        torch.cuda.synchronize()
        return [{"track_ids": x.track_ids.cpu().numpy(), "recs": x.recs.cpu().numpy(), "pred_boxes": x.pred_boxes.tensor.cpu().numpy(),
                 "scores": x.scores.cpu().numpy()} for x in insts], int(idc)

    before, _ = track(model)
    again, _ = track(model)                                                # the second call captures the detector graph and replays it
    assert any(isinstance(v, dict) for v in model._graphs.values())        # ... so load_head meets a CAPTURED graph (old rescoring pointers)
    for a, w in zip(before, again):
        assert all(a[k].tobytes() == w[k].tobytes() for k in a)
    w_before = model.roi_heads.fcs[0][0].clone()
    for _ in range(3):
        trainer.step(batch)
    assert torch.equal(model.roi_heads.fcs[0][0], w_before)                # inference still holds the old head
    trainer.sync_inference()
    assert not any(isinstance(v, dict) for v in model._graphs.values())    # dropped: re-captured on the next use
    assert not torch.equal(model.roi_heads.fcs[0][0], w_before)
    assert torch.equal(model.roi_heads.fcs[0][0].cpu(), trainer.params["roi_heads.asso_head.fc1.weight"].detach().cpu())
    track(model)                                                           # captures again (new pointers); the next call replays
    after, idc_a = track(model)
    assert any(isinstance(v, dict) for v in model._graphs.values())
    scratch = GoMatching(cfg, trainer.state_dict(), device=DEV)
    want, idc_w = track(scratch)
    assert idc_a == idc_w and len(after) == len(want) == len(frames)
    for a, w in zip(after, want):
        for k in a:
            assert a[k].shape == w[k].shape and a[k].tobytes() == w[k].tobytes(), k
    assert sum(len(a["track_ids"]) for a in after) > 0
    # the association scores of the trained head differ from the untrained model's (same reid input, both matchers)
    untrained = GoMatching(cfg, sd, device=DEV)
    x = torch.randn((24, cfg.MODEL.ASSO_HEAD.FC_DIM), generator=torch.Generator().manual_seed(2)).to(DEV)
    s_new = model.roi_heads._forward_transformer(x, [12, 12], 1)
    s_old = untrained.roi_heads._forward_transformer(x, [12, 12], 1)
    s_scr = scratch.roi_heads._forward_transformer(x, [12, 12], 1)
    assert _same_bits(s_new, s_scr) and not torch.equal(s_new, s_old)
    for m in (model, scratch, untrained):
        m.close()
