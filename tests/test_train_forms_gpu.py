"""GPU: the eight autograd Functions of gomatching_amd/training.py and the kernels of csrc/train.hip, each alone, against the
float64 statements of tests/train_statement.py on every case of its tables.  The only assertions on values are
|got - exp| <= bound on EVERY element (the bound derived in train_statement.py, nothing measured), exact zeros where the layout
promises them, and for the chain max|got - f64| <= 2 x the spread of the float32 statement under eight reorderings on the CPU
(train_statement.chain_statement).  Row-strided operands live in NaN-filled buffers: a read beside a view poisons the result.
Each test prints its worst |err| / bound."""
import numpy as np
import pytest
import torch

import dropout_statement as D
import train_statement as S
from helpers import mini_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
STREAM = (S.P_DROP,) + S.STREAM                       # (p, seed, site, iteration, rank) as ops.dropout takes it
SENTINEL = -7.0
INVALID_ARG = 1


def _fn():
    from gomatching_amd import training
    return training._fn()


def _ops():
    from gomatching_amd import ops
    return ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows_view(a, before=2, after=1):
    """a [M, K] as rows before .. before + M of a NaN-filled [before + M + after, K] buffer (as reid[lo:hi] is a row slice)."""
    M, K = a.shape
    buf = torch.full((before + M + after, K), float("nan"), device=DEV)
    buf[before:before + M] = _dev(a)
    return buf[before:before + M]


def _cols_view(a, left=4, right=4, buf=None, at=None):
    """a [L, E] as columns of a NaN-filled wider row (leading dimension and offset stay multiples of 4 floats)."""
    L, E = a.shape
    if buf is None:
        buf = torch.full((L, left + E + right), float("nan"), device=DEV)
        at = left
    buf[:, at:at + E] = _dev(a)
    return buf[:, at:at + E]


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, want, what, worst_of):
    """got {name: tensor or array}; want {name: (exp, bound)}: every element inside; keeps the worst ratio per name."""
    for k, (exp, bound) in want.items():
        g = got[k]
        g = _np(g) if torch.is_tensor(g) else np.asarray(g)
        assert g.shape == exp.shape, (what, k, g.shape, exp.shape)
        r, at = S.worst(g, exp, bound)
        worst_of[k] = max(worst_of.get(k, 0.0), r)
        assert r <= 1.0, "%s %s: |got - exp| / bound = %.3g at flat index %d (got %r, exp %r, bound %.3g)" % (
            what, k, r, at, g.reshape(-1)[at], exp.reshape(-1)[at], bound.reshape(-1)[at])


def _report(name, worst_of):
    print("%s: worst |err| / bound  %s" % (name, "  ".join("%s %.4f" % kv for kv in sorted(worst_of.items()))))


# ------------------------------------------------------------------------------------------ Linear, LinearReluDrop
def _linear_gpu(case, drop):
    M, N, K, bias, relu = case
    x, w, b, dy = S.linear_inputs(M, N, K, bias)
    xv = _rows_view(x).requires_grad_()
    wd = _dev(w).requires_grad_()
    bd = None if b is None else _dev(b).requires_grad_()
    if drop:
        y = _fn()["LinearReluDrop"].apply(xv, wd, bd, STREAM)
    else:
        y = _fn()["Linear"].apply(xv, wd, bd, relu)
    y.backward(_dev(dy))
    torch.cuda.synchronize()
    got = {"y": y, "dx": xv.grad, "dw": wd.grad}
    if bd is not None:
        got["db"] = bd.grad
    mult = S.mask_mult((M, N), S.P_DROP) if drop and M else None
    return got, S.linear64(x, w, b, relu, dy, mult, float(D.scale_f32(S.P_DROP)))


@pytest.mark.parametrize("M", S.LINEAR_M)
def test_linear(M):
    w1, w2 = {}, {}
    for case in S.LINEAR_CASES:
        if case[0] != M:
            continue
        got, want = _linear_gpu(case, False)
        _check(got, want, ("Linear", case), w1)
        if case[4]:
            got, want = _linear_gpu(case, True)
            _check(got, want, ("LinearReluDrop", case), w2)
    _report("Linear M=%d" % M, w1)
    _report("LinearReluDrop M=%d" % M, w2)
    if M == 0:                                                                         # zeros of the right shapes, no launch error
        got, _ = _linear_gpu((0, 5, 8, True, True), False)
        assert tuple(got["y"].shape) == (0, 5) and tuple(got["dx"].shape) == (0, 8)
        assert tuple(got["dw"].shape) == (5, 8) and tuple(got["db"].shape) == (5,)
        assert not got["dw"].any() and not got["db"].any()


def test_linear_seam_pair():
    """N K = 2^18: the dgrad dY W (128 or 129 rows, 256 outputs, depth 1024) and the forward run on split-K at 128 rows and on
    the tile kernel at 129; the two runs share their first 128 rows, and those rows of dX are inside the bound on both sides."""
    first = {}
    for M in S.SEAM_M:
        assert (0 < M <= 128 and S.SEAM[0] * S.SEAM[1] >= 2 ** 18 and S.SEAM[1] >= 256) == (M == 128)
        w = {}
        got, want = _linear_gpu((M, S.SEAM[0], S.SEAM[1], True, False), False)
        _check(got, want, ("Linear seam", M), w)
        _report("Linear seam M=%d" % M, w)
        first[M] = (_np(got["dx"])[:128], want["dx"][0][:128], want["dx"][1][:128])
    assert np.array_equal(first[128][1], first[129][1])                                # the same statement rows ...
    for M in S.SEAM_M:                                                                 # ... met from both sides of the line
        r, _ = S.worst(*first[M])
        print("Linear seam M=%d: first 128 rows of dX, worst |err| / bound %.4f" % (M, r))
        assert r <= 1.0


# ------------------------------------------------------------------------------------------ Attention, AttentionDrop
def _attention_gpu(case, drop):
    heads, hd, Lq, Lk = case
    E = heads * hd
    q, k, v, do = S.attention_inputs(heads, hd, Lq, Lk)
    qv = _cols_view(q).requires_grad_()
    kv = torch.full((Lk, 2 * E + 4), float("nan"), device=DEV)                        # k | v | 4 NaN columns, as _mha cuts them
    kv_k = _cols_view(k, buf=kv, at=0).requires_grad_()
    kv_v = _cols_view(v, buf=kv, at=E).requires_grad_()
    if drop:
        out = _fn()["AttentionDrop"].apply(qv, kv_k, kv_v, heads, STREAM)
    else:
        out = _fn()["Attention"].apply(qv, kv_k, kv_v, heads)
    P = out.grad_fn.saved_tensors[3]
    out.backward(_dev(do))
    torch.cuda.synchronize()
    mult = S.mask_mult((heads, Lq, Lk), S.P_DROP) if drop and Lq and Lk else None
    return {"out": out, "P": P, "dq": qv.grad, "dk": kv_k.grad, "dv": kv_v.grad}, S.attention64(q, k, v, heads, do, mult)


@pytest.mark.parametrize("drop", [False, True], ids=["Attention", "AttentionDrop"])
def test_attention(drop):
    w = {}
    for case in S.ATTN_CASES:
        got, want = _attention_gpu(case, drop)
        _check(got, want, ("attention", case, drop), w)
        Lk = case[3]
        assert not bool(got["P"][:, :, Lk:].any()), ("padding columns of the saved P", case)
    _report("AttentionDrop" if drop else "Attention", w)
    for case in S.ATTN_EMPTY:                                                          # Lq = 0, Lk = 0: zeros of the right shapes
        got, want = _attention_gpu(case, drop)
        _check(got, want, ("attention", case, drop), {})


# ------------------------------------------------------------------------------------------ softmax_rows_backward
def test_softmax_rows_backward():
    ops = _ops()
    from gomatching_amd import lib
    w = {}
    for rows, cols in S.SOFTMAX_CASES:
        P, dP = S.softmax_bwd_inputs(rows, cols)
        ld = S.softmax_ld(cols)
        Pb = torch.full((rows, ld), float("nan"), device=DEV)
        dPb = torch.full((rows, ld), float("nan"), device=DEV)
        Pb[:, :cols], dPb[:, :cols] = _dev(P), _dev(dP)
        exp, bound = S.softmax_bwd_case64(P, dP)
        dS = ops.softmax_rows_backward(Pb, dPb, cols, S.SOFTMAX_SCALE)                 # the wrapper: a zeroed dS of P's layout
        torch.cuda.synchronize()
        assert tuple(dS.shape) == (rows, ld) and not bool(dS[:, cols:].any()), ("padding columns of dS", rows, cols)
        _check({"dS": dS[:, :cols]}, {"dS": (exp, bound)}, ("softmax_rows_backward", rows, cols), w)
        out = torch.full((rows + 1, ld), SENTINEL, device=DEV)                         # the library entry: a sentinel around what it owns
        lib.check(lib.load().gom_softmax_rows_backward_f32(ops._p(Pb), ops._p(dPb), ops._p(out), rows, cols, ld,
                                                           S.SOFTMAX_SCALE, ops._stream()), "gom_softmax_rows_backward_f32")
        torch.cuda.synchronize()
        assert bool((out[:rows, cols:] == SENTINEL).all()) and bool((out[rows] == SENTINEL).all()), (rows, cols)
        assert torch.equal(out[:rows, :cols], dS[:, :cols])
    _report("softmax_rows_backward", w)


# ------------------------------------------------------------------------------------------ asso_ce, AssoCE
@pytest.mark.parametrize("R", S.ASSO_ROWS)
def test_asso_ce(R):
    ops = _ops()
    w = {}
    for case in S.ASSO_CASES:
        if case[0] != R:
            continue
        l, offs, gt = S.asso_inputs(*case)
        ld_, od, gd = _dev(l), _dev(offs), _dev(gt)
        for gs in S.ASSO_SCALES:
            want = S.asso_ce64(l, offs, gt, gs)
            g = torch.tensor([gs], dtype=torch.float32, device=DEV)
            loss_only, none = ops.asso_ce(ld_, od, gd)
            none2, grad_only = ops.asso_ce(ld_, od, gd, want_loss=False, grad_scale=g)
            loss, grad = ops.asso_ce(ld_, od, gd, grad_scale=g)
            torch.cuda.synchronize()
            assert none is None and none2 is None
            _check({"loss": loss, "dlogits": grad}, want, ("asso_ce", case, gs), w)
            assert torch.equal(loss_only, loss) and torch.equal(grad_only, grad), (case, gs)
    _report("asso_ce rows=%d" % R, w)


def test_assoce_and_focalsum():
    wa, wf = {}, {}
    up = torch.tensor(S.UPSTREAM, device=DEV)
    for count in S.SUM_COUNTS:
        l, offs, gt = S.asso_inputs(1, (2,) * count, "unit")
        gt = np.maximum(gt, 0)                                                         # every pair counts: `count` summed values
        lt = _dev(l).requires_grad_()
        total = _fn()["AssoCE"].apply(lt, _dev(offs), _dev(gt))
        total.backward(up)
        torch.cuda.synchronize()
        assert total.dim() == 0
        _check({"total": total, "dlogits": lt.grad}, S.assoce_sum64(l, offs, gt, S.UPSTREAM), ("AssoCE", count), wa)
        x, t = S.focal_inputs(255)
        x, t = x[:count].copy(), t[:count].copy()
        xt = _dev(x.reshape(-1, 1)).requires_grad_()
        total = _fn()["FocalSum"].apply(xt, _dev(t.reshape(-1, 1)), 0.25, 2.0)
        total.backward(up)
        torch.cuda.synchronize()
        _check({"total": total, "dx": xt.grad.view(-1)}, S.focalsum64(x, t, 0.25, 2.0, S.UPSTREAM), ("FocalSum", count), wf)
    _report("AssoCE", wa)
    _report("FocalSum", wf)


# ------------------------------------------------------------------------------------------ sigmoid_focal
def test_sigmoid_focal():
    ops = _ops()
    w = {}
    for n, (alpha, gamma) in S.FOCAL_CASES:
        x, t = S.focal_inputs(n)
        xd, td = _dev(x), _dev(t)
        want = S.focal64(x, t, alpha, gamma)
        loss_only, none = ops.sigmoid_focal(xd, td, alpha, gamma, want_grad=False)
        none2, grad_only = ops.sigmoid_focal(xd, td, alpha, gamma, want_loss=False)
        loss, dx = ops.sigmoid_focal(xd, td, alpha, gamma)
        torch.cuda.synchronize()
        assert none is None and none2 is None
        _check({"loss": loss, "dx": dx}, want, ("sigmoid_focal", n, alpha, gamma), w)
        assert torch.equal(loss_only, loss) and torch.equal(grad_only, dx)
    _report("sigmoid_focal", w)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch():
    ops = _ops()
    from gomatching_amd import lib
    L = lib.load()
    l, offs, gt = S.asso_inputs(4, (3, 0, 2), "unit")
    ld_, od, gd = _dev(l), _dev(offs), _dev(gt)
    R, N = l.shape
    loss = torch.full((R, 3), SENTINEL, device=DEV)
    dl = torch.full((R, N), SENTINEL, device=DEV)
    g = torch.ones(1, device=DEV)
    p, st = ops._p, ops._stream
    # neither loss nor dlogits
    assert L.gom_asso_ce_f32(p(ld_), N, p(od), 3, p(gd), R, None, p(g), None, st()) == INVALID_ARG
    # dlogits without grad_scale
    assert L.gom_asso_ce_f32(p(ld_), N, p(od), 3, p(gd), R, p(loss), None, p(dl), st()) == INVALID_ARG
    # ld < cols
    P, dP = S.softmax_bwd_inputs(4, 65)
    dS = torch.full((4, 65), SENTINEL, device=DEV)
    assert L.gom_softmax_rows_backward_f32(p(_dev(P)), p(_dev(dP)), p(dS), 4, 65, 64, S.SOFTMAX_SCALE, st()) == INVALID_ARG
    torch.cuda.synchronize()
    for t in (loss, dl, dS):
        assert bool((t == SENTINEL).all()), "a refused call wrote to its output"
    # and the next valid call is as usual
    assert L.gom_asso_ce_f32(p(ld_), N, p(od), 3, p(gd), R, p(loss), p(g), p(dl), st()) == 0
    torch.cuda.synchronize()
    _check({"loss": loss, "dlogits": dl}, S.asso_ce64(l, offs, gt, 1.0), "asso_ce after the refusals", {})


# ------------------------------------------------------------------------------------------ the chain
def _chain_cfg(variant):
    name, n_enc, n_dec, _ = S.chain_layers(variant)
    cfg = mini_cfg("icdar15")
    A = cfg.MODEL.ASSO_HEAD
    A.NUM_HEADS, A.NUM_ENCODER_LAYERS, A.NUM_DECODER_LAYERS = S.CHAIN_HEADS, n_enc, n_dec
    if variant == "shared":
        cfg.MODEL.ROI_HEADS.NAME = "SHA_FFN_CRSATTN"
    assert (cfg.MODEL.ROI_HEADS.NAME == "SHA_FFN_CRSATTN") == (variant == "shared")
    return cfg


@pytest.mark.parametrize("variant,frames,p", S.CHAIN_CASES, ids=["%s-%s-%s" % (v, "_".join(map(str, f)), p) for v, f, p in S.CHAIN_CASES])
def test_chain(variant, frames, p):
    """matcher_transformer -> the feats memory^T logits (a Linear whose weight is an activation) -> _detr_asso_loss, E = 32,
    4 heads, FFN 48: wiring (sites, slices, which gradient goes to which tensor), every output and every parameter gradient,
    all elements, against the float64 chain; bound: 2 x the float32 statement's spread under eight reorderings."""
    from gomatching_amd import training
    exp, spread = S.chain_statement(variant, frames, p)
    cfg = _chain_cfg(variant)
    params = {k: torch.nn.Parameter(_dev(v)) for k, v in S.chain_params(variant).items()}
    reid0, offs, gt, num = S.chain_inputs(frames)
    N = reid0.shape[0]
    reid = _rows_view(reid0).requires_grad_()
    seed, iteration, rank = S.CHAIN_STREAM
    state = None if p is None else training.DropoutState(p, seed, iteration, rank)
    feats, memory = training.matcher_transformer(params, cfg, reid, variant == "short", dropout=state)
    logits = _fn()["Linear"].apply(feats, memory, None, False)
    loss = training._detr_asso_loss(logits, gt.astype(np.int64), np.arange(N), list(frames), True)   # row i is its own track
    loss.backward()
    torch.cuda.synchronize()
    if state is not None:
        assert state.site == exp["sites"]
    got = {"feats": feats, "memory": memory, "logits": logits, "loss": loss, "d reid": reid.grad}
    for k, q in params.items():
        assert q.grad is not None, k
        got["d " + k] = q.grad
    assert set(got) == set(spread)
    failures, worst = [], 0.0
    for k in sorted(got):
        g = _np(got[k]).astype(np.float64)
        assert g.shape == exp[k].shape, k
        err = float(np.abs(g - exp[k]).max())
        err = float("inf") if np.isnan(err) else err
        ratio = 0.0 if err == 0 else err / spread[k] if spread[k] > 0 else float("inf")
        worst = max(worst, ratio)
        print("chain %-7s %-12s p %-4s %-72s max|gpu - f64| %.3e  spread %.3e  ratio %.3f" % (variant, frames, p, k[:72], err, spread[k], ratio))
        if not err <= 2 * spread[k]:
            failures.append((k, err, spread[k]))
    print("chain %s %s p %s: worst max|gpu - f64| / spread %.3f" % (variant, frames, p, worst))
    assert not failures, failures
