"""CPU: the host side of training the association head (gomatching_amd/solver.py): the float64 statement against the
reference's optimizer (tests/golden/solver_adamw.npz, tools/gen_golden_solver.py), the SOLVER keys, the schedule, the
param-group rule, optimizer-state exchange with torch.optim.AdamW, checkpoints, and the Detectron2 drop-in.  No GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

import solver_statement as S
from helpers import mini_cfg, golden
from gomatching_amd import solver
from gomatching_amd.config import BUILTIN, setup_cfg
from gomatching_amd.weights import canonical_keys, synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_reproduces_the_reference_optimizer():
    """Statement and fixture agree before either judges a kernel: per tensor within the error the generator recorded."""
    g = golden("solver_adamw.npz")
    assert [tuple(g["shape_%d" % i]) for i in range(int(g["n_tensors"]))] == S.SHAPES and int(g["steps"]) == S.STEPS
    for i, s in enumerate(S.SHAPES):
        assert np.array_equal(S.fixture_parameters(int(g["seed"]))[i], g["init_%d" % i])
    p, m, v, t, totals, coefs = S.run_statement(g)
    assert np.allclose(totals, g["total_norm_f64"], rtol=1e-14, atol=0) and np.allclose(coefs, g["coef_f64"], rtol=1e-14, atol=0)
    assert 0 < sum(c < 1.0 for c in coefs) < S.STEPS                       # both clip branches
    assert t == [int(g["ref_step_%d" % i]) for i in range(len(t))] and t[2] == S.STEPS - 2
    for i in range(len(p)):
        for name, x in (("p", p[i]), ("exp_avg", m[i]), ("exp_avg_sq", v[i])):
            err = float(np.max(np.abs(g["ref_%s_%d" % (name, i)].astype(np.float64) - x)))
            rec = float(g["ref_err_%s_%d" % (name, i)])
            assert err <= rec * (1 + 1e-9) + 1e-300, (i, name, err, rec)
        assert float(g["ref_err_p_%d" % i]) <= 1e-7                            # the reference's own fp32 error is small
        assert float(np.max(np.abs(p[i] - g["init_%d" % i]))) >= 1e-4             # ... against a real movement


def _closed_form(it, max_iter=30000, warmup=1000, factor=1e-3):
    x, w = it / max_iter, warmup / max_iter
    c = lambda u: 0.5 * (1 + math.cos(math.pi * u))
    return c(x) if x >= w else c(w) * (factor + (1 - factor) * x / w)


def test_warmup_cosine_schedule_and_solver_keys():
    cfg = setup_cfg(builtin="icdar15")
    for it in (0, 1, 500, 999, 1000, 1001, 15000, 29999, 30000):
        assert abs(solver.warmup_cosine_lr(it, cfg) - _closed_form(it)) <= 1e-15, it
    assert solver.warmup_cosine_lr(0, cfg) == pytest.approx(1e-3 * _closed_form(1000), rel=1e-12)
    assert solver.warmup_cosine_lr(15000, cfg) == pytest.approx(0.5, abs=1e-15) and solver.warmup_cosine_lr(30000, cfg) == 0.0
    assert solver.warmup_cosine_lr(1000, cfg) < 1.0                       # the warm-up ends ON the cosine, not at 1
    with open(os.path.join(ROOT, "tests", "golden", "solver_configs.json")) as f:
        ref = json.load(f)
    assert sorted(ref) == sorted(BUILTIN)
    for name in BUILTIN:
        cfg = setup_cfg(builtin=name)
        assert json.loads(json.dumps(cfg.SOLVER)) == ref[name], name         # the yaml's SOLVER block, as the reference wrote it
        s = solver.solver_cfg(cfg)
        assert s.OPTIMIZER == "ADAMW" and s.USE_CUSTOM_SOLVER and s.LR_SCHEDULER_NAME == "WarmupCosineLR"
        C = s.CLIP_GRADIENTS
        assert C.ENABLED and C.CLIP_TYPE == "full_model" and C.CLIP_VALUE == 0.1 and C.NORM_TYPE == 2.0
        assert s.BASE_LR == ref[name]["BASE_LR"] == 5e-5 and s.MAX_ITER == 30000 and s.CHECKPOINT_PERIOD == 5000
        assert s.WEIGHT_DECAY == 1e-4 and s.WARMUP_ITERS == 1000 and s.WARMUP_FACTOR == 1e-3 and s.WARMUP_METHOD == "linear"
        assert s.TRAIN_ITER == -1 and s.CUSTOM_MULTIPLIER == 1.0 and s.CUSTOM_MULTIPLIER_NAME == []
    from gomatching_amd import config
    assert "SOLVER" not in config._DEFAULTS                               # inference-path keys only
    assert solver.solver_cfg(config.get_cfg()).OPTIMIZER == "SGD"         # the reference's default without a yaml


def _head(cfg, frozen=()):
    out = []
    for k, shape in canonical_keys(cfg).items():
        p = torch.nn.Parameter(torch.zeros(tuple(shape)), requires_grad=k.startswith("roi_heads.") and k not in frozen)
        out.append((k, p))
    return out


def test_build_optimizer_groups_and_refusals():
    cfg = mini_cfg("icdar15")
    cfg.SOLVER.CUSTOM_MULTIPLIER = 3.0
    cfg.SOLVER.CUSTOM_MULTIPLIER_NAME = ["short_term_matcher"]
    frozen = ("roi_heads.rescoring_head.weight", "roi_heads.rescoring_head.bias")
    named = _head(cfg, frozen) + [("roi_heads.fake_backbone_adapter.weight", torch.nn.Parameter(torch.zeros(3)))]
    opt = solver.build_optimizer(cfg, named)
    assert isinstance(opt, solver.ClippedAdamW) and isinstance(opt, torch.optim.Optimizer) and opt.clip_value == 0.1
    want = [(k, p) for k, p in named if p.requires_grad]
    assert len(opt.param_groups) == len(want) and all(len(g["params"]) == 1 for g in opt.param_groups)
    ids = {id(g["params"][0]) for g in opt.param_groups}
    assert all(id(p) not in ids for k, p in named if not k.startswith("roi_heads.") or k in frozen)
    for (k, p), g in zip(want, opt.param_groups):
        assert g["params"][0] is p
        lr = 5e-5 * (0.1 if "backbone" in k else 1.0) * (3.0 if "short_term_matcher" in k else 1.0)
        assert g["lr"] == lr and g["weight_decay"] == 1e-4 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8, k
    assert any("backbone" in k for k, _ in want) and any("short_term_matcher" in k for k, _ in want)
    assert len(solver.build_optimizer(cfg, named + named).param_groups) == len(want)       # no duplicates
    for key, value, match in (("OPTIMIZER", "SGD", "OPTIMIZER"), ("CLIP_TYPE", "norm", "CLIP_TYPE"), ("CLIP_TYPE", "value", "CLIP_TYPE"),
                              ("NORM_TYPE", 1.0, "NORM_TYPE")):
        bad = mini_cfg("icdar15")
        (bad.SOLVER if key == "OPTIMIZER" else bad.SOLVER.CLIP_GRADIENTS)[key] = value
        with pytest.raises(NotImplementedError, match=match):
            solver.build_optimizer(bad, named)
    off = mini_cfg("icdar15")
    off.SOLVER.CLIP_GRADIENTS.ENABLED = False
    assert solver.build_optimizer(off, named).clip_value == 0.0


def test_optimizer_state_goes_to_torch_adamw_and_back():
    shapes = [(5, 7), (3,), (1,)]
    mine = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    opt = solver.ClippedAdamW([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(mine)], 1e-3, weight_decay=1e-4, clip_value=0.1)
    gen = torch.Generator().manual_seed(1)
    for i, p in enumerate(mine[:2]):                                        # the third tensor has no state yet
        opt.state[p] = {"step": torch.tensor(float(3 + i)), "exp_avg": torch.randn(shapes[i], generator=gen),
                        "exp_avg_sq": torch.rand(shapes[i], generator=gen)}
    sd = opt.state_dict()
    assert set(sd["state"]) == {0, 1} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    theirs = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    ref = torch.optim.AdamW([{"params": [p]} for p in theirs])
    ref.load_state_dict(sd)
    for i, p in enumerate(theirs[:2]):
        st = ref.state[p]
        assert float(st["step"]) == 3 + i
        assert torch.equal(st["exp_avg"], opt.state[mine[i]]["exp_avg"]) and torch.equal(st["exp_avg_sq"], opt.state[mine[i]]["exp_avg_sq"])
    assert [g["lr"] for g in ref.param_groups] == [1e-3, 2e-3, 3e-3] and ref.param_groups[0]["weight_decay"] == 1e-4
    # a step of torch's optimizer, then its state back into a fresh ClippedAdamW
    for p in theirs:
        p.grad = torch.ones_like(p)
    ref.step()
    back = solver.ClippedAdamW([{"params": [torch.nn.Parameter(torch.zeros(s))]} for s in shapes], clip_value=0.1)
    back.load_state_dict(ref.state_dict())
    ps = [g["params"][0] for g in back.param_groups]
    for i, p in enumerate(ps):
        st, rt = back.state[p], ref.state[theirs[i]]
        assert st["step"].device.type == "cpu" and float(st["step"]) == float(rt["step"]) == (4 + i if i < 2 else 1)
        assert torch.equal(st["exp_avg"], rt["exp_avg"]) and torch.equal(st["exp_avg_sq"], rt["exp_avg_sq"])
    assert [g["lr"] for g in back.param_groups] == [1e-3, 2e-3, 3e-3]
    again = back.state_dict()
    for k in sd["state"]:
        assert float(again["state"][k]["step"]) == float(ref.state_dict()["state"][k]["step"])
    opt.zero_grad()                                                         # torch's meaning: gradients become None
    mine[0].grad = torch.ones_like(mine[0])
    opt.zero_grad()
    assert mine[0].grad is None


def test_checkpoint_is_read_by_the_eval_command_line(tmp_path):
    from gomatching_amd import eval as gom_eval
    cfg = mini_cfg("icdar15")
    sd = synth_state_dict(cfg, seed=5, as_torch=False)                      # plain dict of numpy arrays
    opt = solver.ClippedAdamW([torch.nn.Parameter(torch.zeros(3))], clip_value=0.1)
    path = solver.save_checkpoint(str(tmp_path / "sub" / "model_final.pth"), sd, opt.state_dict(), iteration=41)
    raw = torch.load(path, map_location="cpu")
    assert set(raw) == {"model", "optimizer", "iteration"} and raw["iteration"] == 41 and "param_groups" in raw["optimizer"]
    got = gom_eval.load_weights(path)
    keys = canonical_keys(cfg)
    assert set(keys) <= set(got)
    for k, shape in keys.items():
        assert tuple(got[k].shape) == tuple(shape) and np.array_equal(got[k].numpy(), sd[k]), k


def test_detectron2_drop_in_builds_groups_over_the_head_only():
    from oracle import ref_shim
    from gomatching_amd.compat import d2_register
    from gomatching_amd.compat.solver import build_custom_optimizer
    ref_shim.install_stand_ins()
    from detectron2.modeling.meta_arch.build import META_ARCH_REGISTRY
    d2_register.register(META_ARCH_REGISTRY)
    cfg = mini_cfg("icdar15")
    model = META_ARCH_REGISTRY.get(d2_register.ARCH_NAME)(cfg)
    opt = build_custom_optimizer(cfg, model)
    assert isinstance(opt, solver.ClippedAdamW)
    names = {id(p): n for n, p in model.named_parameters()}
    got = [names[id(g["params"][0])] for g in opt.param_groups]
    assert got and all(n.startswith("roi_heads.") for n in got)
    assert sorted(got) == sorted(n for n, p in model.named_parameters() if p.requires_grad)
    assert all(g["params"][0] is dict(model.named_parameters())[n] for g, n in zip(opt.param_groups, got))   # the live parameters
    assert all(g["lr"] == 5e-5 for g in opt.param_groups) and opt.clip_value == 0.1
    for v in model.roi_heads.rescoring_head.parameters():                    # train_net.py:103-104
        v.requires_grad = False
    assert len(build_custom_optimizer(cfg, model).param_groups) == len(got) - 2


def test_entry_points_reject_bad_tables_without_a_gpu():
    """Argument checks of gom_clipped_adamw_* run before any HIP call (no device needed)."""
    import ctypes
    from gomatching_amd import lib
    L = lib.load()
    INVALID = 1
    p = 0x1000                                                     # non-null, aligned, never dereferenced
    ws = ctypes.c_void_p(0x2000)

    def table(*rows):
        t = (lib.OptimTensor * max(len(rows), 1))()
        for i, r in enumerate(rows):
            t[i] = lib.OptimTensor(*r)
        return t
    good = (p, p, p, p, 5000, 1, 1e-3, 0.01)
    step = lambda t, n, partials=ws, n_partials=16, norm=ws: L.gom_clipped_adamw_step(t, n, 0.9, 0.999, 1e-8, 0.1, partials, n_partials, norm, None)
    assert L.gom_clipped_adamw_partials(table(good, (p, p, p, p, 4096, 1, 1e-3, 0.0), (p, p, p, p, 0, 1, 1e-3, 0.0)), 3) == 3   # 2 + 1 + 0 chunks
    assert L.gom_clipped_adamw_partials(None, 1) == -1 and step(None, 1) == INVALID
    assert L.gom_clipped_adamw_partials(table(good), 0) == -1 and step(table(good), 0) == INVALID and step(table(good), -2) == INVALID
    for bad in ((p, p, p, p, -1, 1, 1e-3, 0.01), (None, p, p, p, 8, 1, 1e-3, 0.01), (p, None, p, p, 8, 1, 1e-3, 0.01),
                (p, p, p, None, 8, 1, 1e-3, 0.01), (p, p, p, p, 8, 0, 1e-3, 0.01), (p + 2, p, p, p, 8, 1, 1e-3, 0.01)):
        assert L.gom_clipped_adamw_partials(table(good, bad), 2) == -1, bad
        assert step(table(good, bad), 2) == INVALID, bad
    assert step(table(good), 1, n_partials=1) == INVALID           # workspace smaller than the two chunks
    assert step(table(good), 1, partials=None) == INVALID and step(table(good), 1, norm=None) == INVALID
    assert L.gom_clipped_adamw_step(table(good), 1, 1.0, 0.999, 1e-8, 0.1, ws, 16, ws, None) == INVALID     # beta1 = 1


def test_solver_cfg_takes_config_nodes_only_and_unsupported_groups_raise():
    with pytest.raises(TypeError):
        solver.solver_cfg(None)
    with pytest.raises(TypeError):
        solver.warmup_cosine_lr(0, "configs/x.yaml")

    class Yacs(dict):                                              # what a Detectron2 node offers: items() and dump()
        def dump(self):
            import yaml
            return yaml.safe_dump({"SOLVER": {"OPTIMIZER": "ADAMW", "MAX_ITER": 7}})
    obj = type("Node", (), {"dump": Yacs().dump, "items": lambda self: []})()
    s = solver.solver_cfg(obj)
    assert s.OPTIMIZER == "ADAMW" and s.MAX_ITER == 7 and s.WEIGHT_DECAY == 1e-4
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    for key in ("amsgrad", "maximize"):
        opt = solver.ClippedAdamW([p])
        opt.param_groups[0][key] = True
        with pytest.raises(NotImplementedError, match=key):
            opt.step()
    opt = solver.ClippedAdamW([p])                                  # a refused step (CPU tensors) leaves the step count alone
    with pytest.raises(Exception):
        opt.step()
    assert float(opt.state[p]["step"]) == 0.0
