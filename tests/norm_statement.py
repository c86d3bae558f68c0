"""float64 statements of the norm kernels (csrc/norm.hip: LayerNorm with an optional residual, GroupNorm(32, 256) channels-last;
csrc/swin.hip: LayerNorm over any width), their bounds, and the inputs shared by tests/test_norm_statement_cpu.py and
tests/test_norm_forms_gpu.py (same generators, same seeds: the same bits).

    LayerNorm   v = x + residual;  y = (v - mean(v)) / sqrt(var(v) + eps) * gamma + beta         per row, var = mean((v - mean)^2)
    GroupNorm   the same per (image, group of 8 consecutive channels) over all HW rows of [B, HW, 256]

Bounds.  Moderate data: the project's 2e-5 + 1e-5 |ref| (tests/test_ops_gpu.py, test_layernorm_groupnorm), here against float64.
Offset rows (mean >> spread) have no project number; the kernel is measured against the reference instead, by the project's "within
twice the reference's own error" rule (tests/test_solver_gpu.py): max|gpu - fp64| <= 2 max|F.layer_norm fp32 on the CPU - fp64| on the
same input, plus one ulp of the largest output.  A constant row of few significant bits must give beta exactly."""
import numpy as np

EPS = 1e-5
LN_KINDS = ("moderate", "const", "offset1", "offset001")
GN_KINDS = ("moderate", "offset50")
f32 = np.float32


def layernorm64(x, gamma, beta, residual=None, eps=EPS):
    v = np.asarray(x, np.float64)
    if residual is not None:
        v = v + np.asarray(residual, np.float64)
    mean = v.mean(-1, keepdims=True)
    var = ((v - mean) ** 2).mean(-1, keepdims=True)
    return (v - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def groupnorm64(x, gamma, beta, eps=EPS, groups=32):
    """x [B, HW, C] channels-last; group g = channels g * C / groups .. (g + 1) * C / groups - 1."""
    v = np.asarray(x, np.float64)
    B, HW, C = v.shape
    vg = v.reshape(B, HW, groups, C // groups)
    mean = vg.mean((1, 3), keepdims=True)
    var = ((vg - mean) ** 2).mean((1, 3), keepdims=True)
    y = ((vg - mean) / np.sqrt(var + eps)).reshape(B, HW, C)
    return y * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def moderate_bound(ref):
    return 2e-5 + 1e-5 * np.abs(ref)


def ln_inputs(kind, rows, D, residual, seed=0):
    """-> x, r | None, gamma, beta (float32).
      moderate   3 randn + 1
      const      row i holds 1.5 (i even) or -3.25 (i odd) in every column; with a residual x = value - 0.5, r = 0.5
      offset1    1000 + randn: the mean dwarfs the spread (a one-pass variance loses it)
      offset001  1000 + 0.01 randn
    The residual of the random kinds is randn (0.001 randn for offset001, which keeps the spread of the sum at 0.01)."""
    assert kind in LN_KINDS
    g = np.random.default_rng(1000 * LN_KINDS.index(kind) + 10 * rows + D + (5 if residual else 0) + seed)
    gamma, beta = (g.random(D) + 0.5).astype(f32), g.standard_normal(D).astype(f32)
    r = None
    if kind == "const":
        x = np.repeat(np.where(np.arange(rows) % 2 == 0, 1.5, -3.25)[:, None], D, 1)
        if residual:
            x, r = x - 0.5, np.full((rows, D), 0.5)
    else:
        z = g.standard_normal((rows, D))
        x = {"moderate": 3 * z + 1, "offset1": 1000 + z, "offset001": 1000 + 0.01 * z}[kind]
        if residual:
            r = g.standard_normal((rows, D)) * (0.001 if kind == "offset001" else 1.0)
    return x.astype(f32), None if r is None else r.astype(f32), gamma, beta


def ln_reference_error(x, r, gamma, beta):
    """(max|F.layer_norm fp32 on the CPU - fp64|, one ulp of the largest output): the offset rows' yardstick.  The residual is added
    in fp32 first, as the kernel's own input would be."""
    import torch
    import torch.nn.functional as F
    v = torch.from_numpy(x) if r is None else torch.from_numpy(x) + torch.from_numpy(r)
    cpu = F.layer_norm(v, (x.shape[-1],), torch.from_numpy(gamma), torch.from_numpy(beta), EPS).numpy()
    ref = layernorm64(x, gamma, beta, r)
    return float(np.abs(cpu.astype(np.float64) - ref).max()), float(np.spacing(f32(np.abs(ref).max())))


def gn_inputs(kind, B, HW, seed=0):
    """-> x [B, HW, 256], gamma, beta (float32): moderate = 2 randn + 0.5, offset50 = 50 + randn."""
    assert kind in GN_KINDS
    g = np.random.default_rng(100 * GN_KINDS.index(kind) + 1000 * B + HW + seed)
    z = g.standard_normal((B, HW, 256))
    x = 2 * z + 0.5 if kind == "moderate" else 50 + z
    return x.astype(f32), (g.random(256) + 0.5).astype(f32), g.standard_normal(256).astype(f32)


LN_D, LN_ROWS = (256, 1024), (1, 3, 4, 5, 130)              # four rows per workgroup: rows % 4 in {1, 3, 0, 1, 2}
LN_ANY_D, LN_ANY_ROWS = (96, 192, 384, 768, 1536), (1, 3, 5, 9)    # 96: eight rows per workgroup (32 lanes a row), else four
GN_HW, GN_B = (1, 255, 256, 257, 600), (1, 3)               # gn_stats_kernel: blocks of 256 rows, fp64 atomics across blocks
