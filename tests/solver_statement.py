"""The float64 statement of one full-model-clipped AdamW step, and the seeded gradients of tests/golden/solver_adamw.npz.

Used by tools/gen_golden_solver.py (to record how far the reference's fp32 optimizer is from it), by tests/test_solver_cpu.py
(statement against fixture) and by tests/test_solver_gpu.py (kernel against statement).  numpy only.

The update, per iteration (costom_solver.py:55-73 = clip_grad_norm_(all parameters, clip) then torch.optim.AdamW.step):
    total = sqrt(sum over every gradient element of g^2);  coef = min(1, clip / (total + 1e-6))   (clip <= 0: coef = 1)
    for every tensor that HAS a gradient:  t += 1;  g' = coef g;  p *= 1 - lr wd;  m = b1 m + (1 - b1) g';
        v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
A tensor without a gradient is not touched and its t does not advance.
"""
import numpy as np

SHAPES = [(37, 129), (1031,), (64, 65), (5,), (3, 1024)]
GRAD_SCALES = [1e-1, 1e-2, 1e-3, 1e-5, 1e-6]
STEPS = 12
SKIP = {(1, 2), (3, 2)}                  # (zero-based step, tensor): no gradient -- tensor 2 at the 2nd and the 4th step


def clipped_adamw_step_f64(p, g, m, v, t, lr, wd, betas, eps, clip):
    """In place on lists of float64 arrays p, m, v and the list of ints t; g[i] is None for a tensor without a gradient;
    lr / wd: one value per tensor.  Returns (total, coef) as Python floats."""
    b1, b2 = betas
    total = float(np.sqrt(sum(float(np.sum(np.asarray(x, np.float64) ** 2)) for x in g if x is not None)))
    coef = min(1.0, clip / (total + 1e-6)) if clip > 0 else 1.0
    for i, x in enumerate(g):
        if x is None:
            continue
        t[i] += 1
        gs = coef * np.asarray(x, np.float64)
        p[i] *= 1.0 - lr[i] * wd[i]
        m[i][...] = b1 * m[i] + (1.0 - b1) * gs
        v[i][...] = b2 * v[i] + (1.0 - b2) * gs * gs
        p[i] -= (lr[i] / (1.0 - b1 ** t[i])) * m[i] / (np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t[i]) + eps)
    return total, coef


def fixture_parameters(seed, shapes=SHAPES):
    """The fixture's initial parameters: N(0, 0.05) in float32."""
    rng = np.random.default_rng([seed, 0])
    return [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in shapes]


def fixture_gradients(seed, step, shapes=SHAPES, scales=GRAD_SCALES, skip=SKIP):
    """Gradients of zero-based `step`: per tensor N(0, 1) * scale in float32 with 10 % exact zeros; every third step is scaled by
    1e-3 (the whole model's norm then stays under the clip value 0.1); None where (step, tensor) is in `skip`.  One generator per
    step, every tensor drawn whether it is used or not, so a step can be regenerated on its own."""
    rng = np.random.default_rng([seed, 1 + step])
    out = []
    for i, (s, sc) in enumerate(zip(shapes, scales)):
        x = rng.standard_normal(s)
        keep = rng.random(s) >= 0.1
        x = (x * keep * sc * (1e-3 if step % 3 == 2 else 1.0)).astype(np.float32)
        out.append(None if (step, i) in skip else x)
    return out


def abs_sum(grads):
    """float64 sum of |g| over a step's gradients: tells a drifted random generator from a wrong kernel."""
    return float(sum(np.sum(np.abs(x.astype(np.float64))) for x in grads if x is not None))


def spacing(x):
    """One fp32 spacing at the largest magnitude of x."""
    a = np.float32(np.max(np.abs(x))) if np.size(x) else np.float32(0)
    return float(np.spacing(a))


def run_statement(g, steps=None):
    """The fixture's steps through the float64 statement -> (p, m, v, t, totals, coefs)."""
    n = int(g["n_tensors"])
    seed = int(g["seed"])
    p = [g["init_%d" % i].astype(np.float64) for i in range(n)]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    t = [0] * n
    totals, coefs = [], []
    for step in range(int(g["steps"]) if steps is None else steps):
        grads = fixture_gradients(seed, step)
        assert abs(abs_sum(grads) - float(g["grad_abs_sum_f64"][step])) <= 1e-12 * float(g["grad_abs_sum_f64"][step]), \
            "the seeded gradients of step %d are not the ones the fixture was made with (numpy generator drift)" % step
        total, coef = clipped_adamw_step_f64(p, grads, m, v, t, [float(g["lr"])] * n, [float(g["weight_decay"])] * n,
                                               tuple(g["betas"]), float(g["eps"]), float(g["clip_value"]))
        totals.append(total)
        coefs.append(coef)
    return p, m, v, t, totals, coefs
