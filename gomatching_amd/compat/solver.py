"""Drop-in for the reference's `gomatching.costom_solver` under Detectron2: one changed import in train_net.py:34,

    from gomatching_amd.compat.solver import build_custom_optimizer

and `do_train` (train_net.py:50-151) trains `GoMatchingMI355X` with the fused clipped-AdamW step of csrc/optim.hip: the returned
`ClippedAdamW` is a `torch.optim.Optimizer` over the wrapper's LIVE `nn.Parameter`s (one param group per trainable parameter),
so `build_lr_scheduler(cfg, optimizer)` drives its `group["lr"]` and `DetectionCheckpointer(..., optimizer=optimizer)` saves and
restores it.  The step bumps the parameters' versions, which is what makes the wrapper rebuild its HIP head for inference."""
from ..solver import ClippedAdamW, build_optimizer  # noqa: F401
from .d2_register import _cfg_of


def build_custom_optimizer(cfg, model):
    """Same signature as costom_solver.py:20: `cfg` a Detectron2 (yacs) CfgNode or this package's, `model` an nn.Module."""
    return build_optimizer(_cfg_of(cfg), model.named_parameters(recurse=True))
