"""Training the association head: the recipe between `losses.backward()` and the next iteration.

The reference's side of it is `do_train` (train_net.py:50-151) with `build_custom_optimizer` (gomatching/costom_solver.py:20-78)
and Detectron2's `build_lr_scheduler`; all eight shipped configs use one recipe: `SOLVER.OPTIMIZER: ADAMW`, full-model
gradient clipping at 0.1 (L2), `WarmupCosineLR`, `FREEZE_TYPE: "ExceptROIheads"`.  Here:

  * `solver_cfg(cfg)`            the SOLVER keys that recipe reads, with defaults;
  * `ClippedAdamW`               a `torch.optim.Optimizer` whose `step()` is the fused HIP step of csrc/optim.hip
                                 (`gom_clipped_adamw_step`: norm partials, clip coefficient, update -- launches only);
  * `build_optimizer`            the param-group rule of costom_solver.py:28-44;
  * `warmup_cosine_lr`           the learning-rate multiplier of `WarmupCosineLR`;
  * `save_checkpoint`, `Trainer` the loop, checkpoints `python -m gomatching_amd.eval` reads, resume.

UNPINNED: Detectron2 is not a dependency and not available where this was written.  The SOLVER defaults in `_D2_DEFAULTS`
and the schedule in `warmup_cosine_lr` are restated from Detectron2 v0.6's published source (detectron2/config/defaults.py,
detectron2/solver/build.py, fvcore/common/param_scheduler.py), as `Boxes` / `nms` are elsewhere in this tree; no test here
compares them with a Detectron2 run.  The optimizer arithmetic IS pinned: tests/golden/solver_adamw.npz holds what the
reference's own optimizer class computes (tools/gen_golden_solver.py).

`MODEL.ASSO_HEAD.DROPOUT` (0.1 in every shipped config) is applied by the training forward at the reference's sites
(training.py, `matcher_transformer`; csrc/dropout.hip).  The mask stream is this project's own -- the reference's distribution,
not torch's bits: a counter-based generator keyed by the trainer's `seed` and indexed by (site, iteration, rank), so a resumed
run reproduces an uninterrupted one and ranks draw different masks.  `Trainer` prints p and the seed once and keeps the seed
in its checkpoints ("dropout_seed").
"""
import math
import os

import torch

from .config import CfgNode, _wrap, _unwrap, _merge

# Detectron2 v0.6 defaults of the SOLVER keys the recipe reads (UNPINNED, see the module doc-string)
_D2_DEFAULTS = {
    "LR_SCHEDULER_NAME": "WarmupMultiStepLR", "MAX_ITER": 40000, "BASE_LR": 0.001, "MOMENTUM": 0.9, "NESTEROV": False,
    "WEIGHT_DECAY": 0.0001, "WARMUP_FACTOR": 1.0 / 1000, "WARMUP_ITERS": 1000, "WARMUP_METHOD": "linear",
    "CHECKPOINT_PERIOD": 5000, "IMS_PER_BATCH": 16,
    "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0},
}
# the reference's own additions (gomatching/config.py:36-42)
_GOM_DEFAULTS = {"RESET_ITER": False, "TRAIN_ITER": -1, "USE_CUSTOM_SOLVER": False, "OPTIMIZER": "SGD", "BACKBONE_MULTIPLIER": 1.0,
                 "CUSTOM_MULTIPLIER": 1.0, "CUSTOM_MULTIPLIER_NAME": []}


def solver_cfg(cfg):
    """The SOLVER block of `cfg` over the defaults above -> CfgNode.  `cfg` is left as it is (`config._DEFAULTS` holds
    inference-path keys only; a yaml's SOLVER block is kept by `merge_from_file` as written)."""
    if not isinstance(cfg, dict):
        if hasattr(cfg, "dump") and hasattr(cfg, "items"):       # a yacs / Detectron2 CfgNode
            import yaml
            cfg = yaml.safe_load(cfg.dump())
        else:
            raise TypeError("solver_cfg: expected a config node or dict, got %s" % type(cfg).__name__)
    d = {}
    _merge(d, _D2_DEFAULTS)
    _merge(d, _GOM_DEFAULTS)
    _merge(d, _unwrap(cfg.get("SOLVER") or {}))
    return _wrap(d)


def warmup_cosine_lr(iteration, cfg):
    """Multiplier of every group's base learning rate at `iteration` under `LR_SCHEDULER_NAME: "WarmupCosineLR"`, as Detectron2
    v0.6's `build_lr_scheduler` composes it (LRMultiplier over WarmupParamScheduler(CosineParamScheduler(1, 0), WARMUP_FACTOR,
    min(WARMUP_ITERS / MAX_ITER, 1), WARMUP_METHOD)).  With x = iteration / MAX_ITER, w = min(WARMUP_ITERS / MAX_ITER, 1) and
    c(x) = (1 + cos(pi x)) / 2:

        x >= w :  c(x)
        x <  w :  "linear":   c(w) (WARMUP_FACTOR + (1 - WARMUP_FACTOR) x / w)
                  "constant": c(w) WARMUP_FACTOR

    (the warm-up ramps to the cosine's value at its END, c(w), not to 1).  UNPINNED (module doc-string)."""
    S = solver_cfg(cfg)
    if S.LR_SCHEDULER_NAME != "WarmupCosineLR":
        raise NotImplementedError("SOLVER.LR_SCHEDULER_NAME %r: only WarmupCosineLR is built (every shipped config)" %
                                  (S.LR_SCHEDULER_NAME,))
    x = float(iteration) / float(S.MAX_ITER)
    w = min(float(S.WARMUP_ITERS) / float(S.MAX_ITER), 1.0)
    c = lambda u: 0.5 * (1.0 + math.cos(math.pi * u))
    if x >= w:
        return c(x)
    if S.WARMUP_METHOD == "linear":
        return c(w) * (S.WARMUP_FACTOR + (1.0 - S.WARMUP_FACTOR) * x / w)
    if S.WARMUP_METHOD == "constant":
        return c(w) * S.WARMUP_FACTOR
    raise ValueError("SOLVER.WARMUP_METHOD %r" % (S.WARMUP_METHOD,))


class ClippedAdamW(torch.optim.Optimizer):
    """AdamW with full-model gradient clipping: `FullModelGradientClippingOptimizer(torch.optim.AdamW)` of costom_solver.py:55-73
    as ONE fused step on the GPU (`ops.clipped_adamw_step`).  `param_groups` and `state` are torch's (`step` a CPU scalar
    tensor, `exp_avg`, `exp_avg_sq`), so a scheduler can drive `group["lr"]`, and `state_dict()` loads into a
    `torch.optim.AdamW` over same-shaped parameters and back.

    `step()` launches the kernels and nothing else on the device; it never waits for the GPU.  A parameter whose `grad` is None
    is skipped entirely (no decay, no moment update, its step count stays).  The gradients are left as they are: the clipped
    gradient is formed in registers (the reference scales `p.grad` in place).  `grad_norm()` returns the last step's total norm.
    Constructing the optimizer and loading state need no GPU; `step()` needs dense CONTIGUOUS fp32 CUDA parameters and gradients
    on one device and raises otherwise (torch.optim.AdamW accepts a non-contiguous gradient; autograd hands the head contiguous
    ones); a refused step changes nothing, step counts included.  betas and eps are the optimizer's, not a group's: the fused
    step takes one value of each.  `amsgrad` / `maximize` groups (a checkpoint of a torch.optim.AdamW that used them) raise."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip_value=0.0):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("ClippedAdamW: invalid hyper-parameter (lr %r, betas %r, eps %r, weight_decay %r)" %
                             (lr, betas, eps, weight_decay))
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.clip_value = float(clip_value)
        self._norm = None            # device [2]: {total norm, clip coefficient} of the last step
        self._workspace = None

    def _uniform(self, key):
        vals = [g[key] for g in self.param_groups]
        first = tuple(vals[0]) if isinstance(vals[0], (tuple, list)) else vals[0]
        for v in vals[1:]:
            if (tuple(v) if isinstance(v, (tuple, list)) else v) != first:
                raise NotImplementedError("ClippedAdamW: per-group %s is not built (the fused step takes one value)" % key)
        return first

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():                           # torch keeps `step` where the checkpoint had it; the host reads it
            if "step" in st:
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import ops
        beta1, beta2 = self._uniform("betas")
        eps = self._uniform("eps")
        rows, states = [], []
        for group in self.param_groups:
            for key in ("amsgrad", "maximize"):
                if group.get(key):
                    raise NotImplementedError("ClippedAdamW: param group with %s=True is not built" % key)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("ClippedAdamW does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                states.append(st)
                rows.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], int(st["step"]) + 1, group["lr"], group["weight_decay"]))
        if rows:
            self._norm, self._workspace = ops.clipped_adamw_step(rows, beta1, beta2, eps, self.clip_value, self._workspace,
                                                                 self._norm)
            for st, row in zip(states, rows):                    # only a step that was launched counts
                st["step"] += 1
                torch.autograd.graph.increment_version(row[0])   # written through raw pointers: tell autograd (and the META_ARCH
                                                                 # wrapper, which rebuilds its head on a version change)
        return loss

    def grad_norm(self):
        """Total L2 norm of the last step's gradients, before clipping (waits for the step; for logging, train_net.py:40-47)."""
        return None if self._norm is None else float(self._norm[0])

    def clip_coefficient(self):
        return None if self._norm is None else float(self._norm[1])


def build_optimizer(cfg, named_parameters):
    """`build_custom_optimizer` (costom_solver.py:20-78) over (name, parameter) pairs: one group per trainable parameter,
    `lr = BASE_LR` (x BACKBONE_MULTIPLIER for names containing "backbone", x CUSTOM_MULTIPLIER for names containing one of
    CUSTOM_MULTIPLIER_NAME); no per-group weight decay for ADAMW, so the optimizer-level WEIGHT_DECAY applies; clipping from
    CLIP_GRADIENTS.  What no shipped config uses raises here, naming the key."""
    S = solver_cfg(cfg)
    if S.OPTIMIZER != "ADAMW":
        raise NotImplementedError("SOLVER.OPTIMIZER %r: only ADAMW is built (every shipped config)" % (S.OPTIMIZER,))
    C = S.CLIP_GRADIENTS
    if C.ENABLED and C.CLIP_TYPE != "full_model":
        raise NotImplementedError("SOLVER.CLIP_GRADIENTS.CLIP_TYPE %r: only full_model is built" % (C.CLIP_TYPE,))
    if C.ENABLED and float(C.NORM_TYPE) != 2.0:
        raise NotImplementedError("SOLVER.CLIP_GRADIENTS.NORM_TYPE %r: only the L2 norm is built" % (C.NORM_TYPE,))
    groups, memo = [], set()
    for key, value in named_parameters:
        if not value.requires_grad or id(value) in memo:
            continue
        memo.add(id(value))
        lr = S.BASE_LR
        if "backbone" in key:
            lr = lr * S.BACKBONE_MULTIPLIER
        if any(k in key for k in S.CUSTOM_MULTIPLIER_NAME):
            lr = lr * S.CUSTOM_MULTIPLIER
        groups.append({"params": [value], "lr": lr})
    if not groups:
        raise ValueError("build_optimizer: no trainable parameter")
    clip = float(C.CLIP_VALUE) if (C.ENABLED and C.CLIP_VALUE > 0.0) else 0.0
    return ClippedAdamW(groups, S.BASE_LR, weight_decay=S.WEIGHT_DECAY, clip_value=clip)


def save_checkpoint(path, model_state, optimizer_state=None, iteration=0, dropout_seed=None, data_seed=None):
    """Write {"model", "optimizer", "iteration"} (and "dropout_seed" when the run drops, "data_seed" when the run's clips come
    from `data.build_vts_train_loader`) with torch.save: `model_state` = the
    FULL state dict (frozen detector + current
    head) as {canonical key: tensor or array}, stored as CPU tensors -- what `eval.load_weights` / `normalize_state_dict` read,
    and the layout Detectron2's checkpointer writes."""
    import numpy as np
    model = {}
    for k, v in model_state.items():
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else torch.as_tensor(v)
        model[k] = t.detach().cpu().clone()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    ck = {"model": model, "optimizer": optimizer_state, "iteration": int(iteration)}
    if dropout_seed is not None:
        ck["dropout_seed"] = int(dropout_seed)
    if data_seed is not None:
        ck["data_seed"] = int(data_seed)
    torch.save(ck, tmp)
    os.replace(tmp, path)
    return path


class Trainer:
    """`do_train` (train_net.py:50-151) for the native `GoMatching` model: the detector is frozen, `model.trainable_parameters()`
    (the head) trains.

        trainer = Trainer(cfg, model, "out")
        for clip in clips:                      # what `forward_losses` takes: the mapper's output (data.build_vts_train_loader)
            metrics = trainer.step(clip)        # {"loss_...": float, "total_loss", "lr", "grad_norm", "iteration"}
        trainer.save("model_final.pth")         # python -m gomatching_amd.eval --opts MODEL.WEIGHTS out/model_final.pth

    Mirrored: the rescoring-head rule of :97-105 (the head starts from the detector's `ctrl_point_class` unless '_rescore' is
    in MODEL.WEIGHTS, in which case it is frozen), INFERENCE_TH_TEST = INFERENCE_TH_TRAIN (:167), the finite check (:125),
    a checkpoint every CHECKPOINT_PERIOD iterations and at the end, `max_iter` = TRAIN_ITER when >= 0.

    `seed`: the seed of the dropout mask stream (MODEL.ASSO_HEAD.DROPOUT > 0; training.DropoutState).  None = `cfg.SEED` when
    the config has one >= 0, else drawn once from the operating system and printed.  It is written into every checkpoint and
    restored by `resume()`, so that iteration i of a resumed run draws the masks iteration i of the uninterrupted run drew."""

    def __init__(self, cfg, model, output_dir, inference_th_train=0.3, seed=None, motion_whole_batch=False):
        self.cfg, self.model, self.output_dir = cfg, model, output_dir
        # motion clips (still images) as ONE padded batch with per-frame extents instead of one pass per frame size
        # (training.detect_for_training(whole_batch=...)); video clips are one batch either way
        self.motion_whole_batch = model.motion_whole_batch = bool(motion_whole_batch)
        self.solver = S = solver_cfg(cfg)
        self.max_iter = S.MAX_ITER if S.TRAIN_ITER < 0 else S.TRAIN_ITER
        T = cfg.MODEL.TRANSFORMER
        th = T.get("INFERENCE_TH_TRAIN", inference_th_train)       # adet/config/config.py:80 default 0.3
        T.INFERENCE_TH_TEST = th                                    # ASSO_THRESH_TEST stays, as under train_net.py (only eval.py:220 ties it)
        model.set_score_threshold(th)
        params = model.trainable_parameters()
        self.frozen_keys = set()
        if cfg.MODEL.ROI_HEADS.WITH_RESR:
            if "_rescore" not in str(cfg.MODEL.WEIGHTS):
                with torch.no_grad():
                    for leaf in ("weight", "bias"):
                        src = model._sd["detection_transformer.ctrl_point_class.0." + leaf]
                        params["roi_heads.rescoring_head." + leaf].copy_(torch.as_tensor(src).float().reshape(
                            params["roi_heads.rescoring_head." + leaf].shape))
                print("using deepsolo classifier")
            else:
                for leaf in ("weight", "bias"):
                    params["roi_heads.rescoring_head." + leaf].requires_grad_(False)
                    self.frozen_keys.add("roi_heads.rescoring_head." + leaf)
                print("using trained rescoring head")
        self.seed, self.dropout = seed, None
        self.data_seed = None                                    # set by whoever feeds `step` from a seeded loader (train.py)
        if cfg.MODEL.ASSO_HEAD.DROPOUT > 0:
            from . import training
            if seed is None:
                seed = cfg.get("SEED", -1)
                seed = training.new_dropout_seed() if seed is None or int(seed) < 0 else seed
            self.seed = int(seed)
            self.dropout = training.DropoutState(cfg.MODEL.ASSO_HEAD.DROPOUT, self.seed, 0, training.distributed_rank())
            print("MODEL.ASSO_HEAD.DROPOUT = %g, dropout seed %d" % (self.dropout.p, self.seed))
        model.dropout_state = self.dropout                       # what training.forward_losses reads
        self.params = params
        self.optimizer = build_optimizer(cfg, params.items())
        for g in self.optimizer.param_groups:
            g["initial_lr"] = g["lr"]
        self.iteration = 0
        self._set_lr()
        trainable = sum(p.numel() for p in params.values() if p.requires_grad)
        print("trainble params:{} M".format(trainable / 1e6))

    def _set_lr(self):
        m = warmup_cosine_lr(self.iteration, self.cfg)
        for g in self.optimizer.param_groups:
            g["lr"] = g["initial_lr"] * m

    def step(self, batched_inputs):
        from . import training
        if self.dropout is not None:
            self.dropout.begin_forward(self.iteration)
        losses = training.forward_losses(self.model, batched_inputs, motion_whole_batch=self.motion_whole_batch)
        total = sum(v for k, v in losses.items() if "loss" in k)
        if not bool(torch.isfinite(total).all()):
            raise FloatingPointError("non-finite loss at iteration %d: %r" % (self.iteration, {k: float(v) for k, v in losses.items()}))
        self.optimizer.zero_grad()
        if total.requires_grad:
            total.backward()
        training.allreduce_gradients(list(self.params.values()))
        self.optimizer.step()
        lr = self.optimizer.param_groups[0]["lr"]
        self.iteration += 1
        self._set_lr()
        out = {k: float(v) for k, v in losses.items()}
        out.update(total_loss=float(total), lr=lr, grad_norm=self.optimizer.grad_norm(), iteration=self.iteration)
        if self.output_dir and (self.iteration % self.solver.CHECKPOINT_PERIOD == 0 or self.iteration == self.max_iter):
            self.save("model_final.pth" if self.iteration == self.max_iter else "model_%07d.pth" % (self.iteration - 1))
        return out

    def head_state(self):
        """{key: CPU tensor} of the head as trained so far."""
        return {k: p.detach().cpu().clone() for k, p in self.params.items()}

    def state_dict(self):
        sd = {k: torch.as_tensor(v).detach().cpu() for k, v in self.model._sd.items()}
        sd.update(self.head_state())
        return sd

    def save(self, name="model_final.pth"):
        path = name if os.path.isabs(name) else os.path.join(self.output_dir, name)
        save_checkpoint(path, self.state_dict(), self.optimizer.state_dict(), self.iteration - 1,
                        self.seed if self.dropout is not None else None, data_seed=self.data_seed)
        with open(os.path.join(os.path.dirname(path), "last_checkpoint"), "w") as f:
            f.write(os.path.basename(path))
        return path

    def resume(self, path=None):
        """Continue from a checkpoint written by `save()` (default: the one `last_checkpoint` names): head weights, optimizer
        state, the iteration count, the dropout seed and the data seed (a checkpoint without one keeps this trainer's own).  Returns the iteration
        training continues at."""
        if path is None:
            with open(os.path.join(self.output_dir, "last_checkpoint")) as f:
                path = os.path.join(self.output_dir, f.read().strip())
        ck = torch.load(path, map_location="cpu")
        with torch.no_grad():
            for k, p in self.params.items():
                p.copy_(ck["model"][k].reshape(p.shape))
        self.optimizer.load_state_dict(ck["optimizer"])
        for g in self.optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.iteration = int(ck.get("iteration", -1)) + 1
        if ck.get("dropout_seed") is not None:
            self.seed = int(ck["dropout_seed"])
            if self.dropout is not None:
                self.dropout.seed = self.seed
        if ck.get("data_seed") is not None:
            self.data_seed = int(ck["data_seed"])
        self._set_lr()
        return self.iteration

    def sync_inference(self):
        """Make the model's inference path (tracker, rescoring) use the head as trained so far (`GoMatching.load_head`)."""
        self.model.load_head(self.head_state())
        return self.model
