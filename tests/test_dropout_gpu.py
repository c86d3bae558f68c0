"""GPU: training-mode dropout of the association head (csrc/dropout.hip, gomatching_amd/training.py, solver.Trainer, the
META_ARCH wrapper) against the host statement of the mask stream and a float64 restatement of the matcher
(tests/dropout_statement.py).

Bounds.  Mask bits, kept values, the backward's mask, p = 0, reproducibility and resume are EXACT (bit for bit).  Where float32
arithmetic is compared with float64, the bound is twice the error the path WITHOUT dropout shows against the same statement
with masks of ones on the same inputs, measured in the test (another correct fp32 evaluation errs by as much, with independent
sign); the softmax kernels add a floor of one fp32 spacing at the largest value.  In the matcher test errors are taken
relative to the largest magnitude of the tensor they belong to, in its own run: a dropped run's activations and gradients have
other magnitudes than the undropped run's (kept values are scaled by 1 / (1 - p)), and an fp32 error scales with them."""
import math
import os

import numpy as np
import pytest
import torch

import dropout_statement as D
from helpers import mini_cfg, golden
from gomatching_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
STREAM = (7, 3, 5, 1)                        # (seed, site, iteration, rank) of the kernel tests


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _stream(p, s=STREAM):
    return (p, s[0], s[1], s[2], s[3])


def _layouts(rows, cols, values):
    """The same values as a contiguous [rows, cols] tensor, inside wider rows (ld = the next multiple of 4 plus 4: 116 for 111 and
    for 112 columns), and contiguous but starting one float into its allocation -> ([(name, input view, output view)], the wide
    output's whole buffer, filled with -7)."""
    ld = (cols + 3) // 4 * 4 + 4
    a = values.clone()
    wide, wide_out = torch.zeros((rows, ld), device=DEV), torch.full((rows, ld), -7.0, device=DEV)
    wide[:, :cols] = values
    off = torch.zeros(rows * cols + 1, device=DEV)[1:].view(rows, cols)
    off.copy_(values)
    off_out = torch.zeros(rows * cols + 1, device=DEV)[1:].view(rows, cols)
    assert a.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off_out.data_ptr() % 16 == 4 and ld % 4 == 0
    return [("ld=%d" % cols, a, torch.empty_like(a)), ("ld=%d" % ld, wide[:, :cols], wide_out[:, :cols]), ("offset", off, off_out)], wide_out


# ------------------------------------------------------------------------------------------ 1. mask bits
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_bits_equal_the_statement_in_every_layout(p):
    from gomatching_amd import ops
    scale_bits = int(np.float32(D.scale_f32(p)).view(np.int32))
    for n in (1, 3, 4, 5, 255, 256, 257, 4099):                   # one row
        y = ops.dropout(torch.ones(n, device=DEV), _stream(p))
        keep = D.keep_mask(*STREAM, n, p)
        got = y.cpu().numpy()
        assert np.array_equal(got != 0, keep), (p, n)
        assert (got.view(np.int32)[keep] == scale_bits).all() and (got.view(np.int32)[~keep] == 0).all(), (p, n)
    gen = torch.Generator().manual_seed(1)
    for rows, cols in ((37, 111), (37, 112)):                     # 112: the 16-byte path with ld > cols as well
        keep = D.keep_mask(*STREAM, rows * cols, p).reshape(rows, cols)
        for values, res in ((torch.ones(rows, cols), None), (torch.randn(rows, cols, generator=gen), None),
                            (torch.randn(rows, cols, generator=gen), torch.randn(rows, cols, generator=gen))):
            lays, wide_out = _layouts(rows, cols, values.to(DEV))
            rlays = _layouts(rows, cols, res.to(DEV))[0] if res is not None else [(None, None, None)] * 3
            outs = []
            for (name, x, out), (_, r, _) in zip(lays, rlays):
                assert ops.dropout(x, _stream(p), residual=r, out=out) is out
                outs.append(out.clone().contiguous())
            torch.cuda.synchronize()
            assert bool((wide_out[:, cols:] == -7.0).all())       # nothing written beside the view
            want = values.numpy() * D.scale_f32(p)                # one fp32 multiplication ...
            want = np.where(keep, want, np.float32(0))
            if res is not None:
                want = res.numpy() + want                         # ... and one fp32 addition
            for (name, _, _), o in zip(lays, outs):
                assert np.array_equal(o.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32)), (p, rows, cols, name)
                assert _same_bits(o, outs[0]), (p, rows, cols, name)
    # in place, and relu's backward through the dropout: d = dy * scale * (y > 0)
    x = torch.randn(37, 112, generator=gen).to(DEV)
    y = ops.dropout(x, _stream(p))
    z = x.clone()
    ops.dropout(z, _stream(p), out=z)
    assert _same_bits(y, z)
    dy = torch.randn(37, 112, generator=gen).to(DEV)
    d = ops.relu_backward_scaled(dy, y, float(D.scale_f32(p)))
    want = np.where(y.cpu().numpy() > 0, dy.cpu().numpy() * D.scale_f32(p), np.float32(0)).astype(np.float32)
    assert np.array_equal(d.cpu().numpy().view(np.int32), want.view(np.int32))
    with pytest.raises(Exception):
        ops.dropout(x, (1.0, 7, 0, 0, 0))


# ------------------------------------------------------------------------------------------ 2. the backward's mask
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_backward_regenerates_the_mask(p):
    from gomatching_amd import training
    drop = training._fn()["DropAdd"].apply
    gen = torch.Generator().manual_seed(2)
    for shape in ((5,), (37, 111), (64, 128)):
        n = int(np.prod(shape))
        keep = D.keep_mask(*STREAM, n, p).reshape(shape)
        w = torch.randn(shape, generator=gen)
        want = np.where(keep, w.numpy() * D.scale_f32(p), np.float32(0)).astype(np.float32)
        x = torch.randn(shape, generator=gen).to(DEV).requires_grad_()
        (drop(None, x, _stream(p)) * w.to(DEV)).sum().backward()
        assert np.array_equal(x.grad.cpu().numpy().view(np.int32), want.view(np.int32)), (p, shape)
        x2 = x.detach().clone().requires_grad_()
        r = torch.randn(shape, generator=gen).to(DEV).requires_grad_()
        (drop(r, x2, _stream(p)) * w.to(DEV)).sum().backward()
        assert np.array_equal(x2.grad.cpu().numpy().view(np.int32), want.view(np.int32)), (p, shape)
        assert _same_bits(r.grad, w.to(DEV)), (p, shape)


# ------------------------------------------------------------------------------------------ 3. softmax with dropout
def _ulp(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("Lq,Lk", [(1, 1), (3, 5), (25, 25), (100, 130)])
def test_softmax_dropout_forward_and_backward(Lq, Lk, p=0.1):
    """p = 0.1, the value of every shipped config.  The bound is ABSOLUTE and taken from the kernels without dropout, whose
    outputs are 1 / (1 - p) times smaller where kept: it is a fair bound while that factor is near 1 (1.11 here), and would
    not be at p = 0.5, where every kept value and with it any correct evaluation's rounding error doubles.  The mask at
    p = 0.5 is checked bit for bit by the two tests above."""
    from gomatching_amd import ops
    heads, hd = 8, 8
    Lkp = (Lk + 3) // 4 * 4
    R = heads * Lq
    scale = 1.0 / math.sqrt(hd)
    gen = torch.Generator().manual_seed(100 * Lq + Lk)
    S = torch.zeros(R, Lkp)
    S[:, :Lk] = torch.randn(R, Lk, generator=gen) * 6.0          # logits of both signs, a few keys hold most of a row
    dP = torch.zeros(R, Lkp)
    dP[:, :Lk] = torch.randn(R, Lk, generator=gen)
    mult = torch.from_numpy(D.keep_mask(*STREAM, R * Lk, p).reshape(R, Lk).astype(np.float64) * float(D.scale_f32(p)))
    P64 = torch.softmax(S[:, :Lk].double() * float(np.float32(scale)), dim=-1)

    def ds64(P, G):                                               # of the fp32 P the kernels are handed
        P = P.double()
        return float(np.float32(scale)) * P * (G - (G * P).sum(-1, keepdim=True))

    # the kernels without dropout: softmax_rows_scaled_, softmax_rows_backward
    P0 = ops.softmax_rows_scaled_(S.to(DEV).clone(), Lk, scale)
    dS0 = ops.softmax_rows_backward(P0, dP.to(DEV), Lk, scale)
    # with dropout
    P1 = S.to(DEV).clone()
    Pd = ops.softmax_dropout_rows_(P1, Lk, scale, _stream(p))
    dS1 = ops.softmax_dropout_rows_backward(P1, dP.to(DEV), Lk, scale, _stream(p))
    torch.cuda.synchronize()
    assert _same_bits(P1, P0)                                     # the undropped P: the existing kernel's bits
    for name, t in (("P", P1), ("P~", Pd), ("dS", dS1)):
        assert bool((t[:, Lk:] == 0).all()), name                 # padding columns stay exactly zero
    assert np.array_equal((Pd[:, :Lk] != 0).cpu().numpy(), (mult.numpy() != 0) & (P1[:, :Lk].cpu().numpy() != 0))
    base_f = float((P0[:, :Lk].cpu().double() - P64).abs().max())
    err_f = float((Pd[:, :Lk].cpu().double() - P64 * mult).abs().max())
    bound_f = max(2 * base_f, _ulp(float((P64 * mult).abs().max())))
    print("(%d, %d) p %.1f  P~: max|gpu - f64| %.3e   undropped kernel's %.3e   bound %.3e" % (Lq, Lk, p, err_f, base_f, bound_f))
    Pc = P0[:, :Lk].cpu()
    want0, want1 = ds64(Pc, dP[:, :Lk].double()), ds64(Pc, dP[:, :Lk].double() * mult)
    base_b = float((dS0[:, :Lk].cpu().double() - want0).abs().max())
    err_b = float((dS1[:, :Lk].cpu().double() - want1).abs().max())
    bound_b = max(2 * base_b, _ulp(float(want1.abs().max())))
    print("(%d, %d) p %.1f  dS: max|gpu - f64| %.3e   undropped kernel's %.3e   bound %.3e" % (Lq, Lk, p, err_b, base_b, bound_b))
    assert err_f <= bound_f and err_b <= bound_b
    # the per-head calls of a [heads, Lq, Lk] tensor address the same stream: head h starts at element h Lq Lk
    h = heads - 1
    Ph = S.to(DEV)[h * Lq:(h + 1) * Lq].clone()
    Pdh = ops.softmax_dropout_rows_(Ph, Lk, scale, _stream(p), elem0=h * Lq * Lk)
    dSh = ops.softmax_dropout_rows_backward(Ph, dP.to(DEV)[h * Lq:(h + 1) * Lq].clone(), Lk, scale, _stream(p), elem0=h * Lq * Lk)
    assert _same_bits(Pdh, Pd[h * Lq:(h + 1) * Lq]) and _same_bits(dSh, dS1[h * Lq:(h + 1) * Lq])
    # generic kernel on P = the fused one's P~ (what the attention backward regenerates)
    again = torch.zeros_like(P1)
    ops.dropout(P1[:, :Lk], _stream(p), out=again[:, :Lk])
    assert _same_bits(again, Pd)


# ------------------------------------------------------------------------------------------ 4. the matcher
_PARAMS = {}


def _head_params(builtin):
    if builtin not in _PARAMS:
        cfg = mini_cfg(builtin)
        sd = synth_state_dict(cfg, seed=7)
        _PARAMS[builtin] = (cfg, {k: torch.as_tensor(v).float() for k, v in sd.items() if k.startswith("roi_heads.") and "matcher" in k})
    return _PARAMS[builtin]


@pytest.mark.parametrize("builtin,short", [("icdar15", False), ("icdar15", True), ("pp_dstext", False)])
def test_matcher_under_dropout_against_float64(builtin, short):
    from gomatching_amd import training
    cfg, host = _head_params(builtin)
    A = cfg.MODEL.ASSO_HEAD
    shared = cfg.MODEL.ROI_HEADS.NAME == "SHA_FFN_CRSATTN"
    name = "roi_heads." + ("shared_matcher" if shared else ("short_term_matcher" if short else "long_term_matcher"))
    n_enc = 0 if shared else A.NUM_ENCODER_LAYERS
    keys = [k for k in host if k.startswith(name + ".")]
    N, F = 37, A.FC_DIM
    gen = torch.Generator().manual_seed(37)
    reid0 = torch.randn(N, F, generator=gen)
    G1, G2 = torch.randn(N, F, generator=gen), torch.randn(N, F, generator=gen)
    p, seed, iteration, rank = 0.1, 7, 4, 1

    def gpu(state):
        params = {k: torch.nn.Parameter(host[k].to(DEV)) for k in keys}
        reid = reid0.to(DEV).requires_grad_()
        feats, memory = training.matcher_transformer(params, cfg, reid, short, dropout=state)
        ((feats * G1.to(DEV)).sum() + (memory * G2.to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        out = {"feats": feats.detach().cpu(), "memory": memory.detach().cpu(), "d reid": reid.grad.cpu()}
        for k in keys:
            if params[k].grad is not None:
                out["d " + k] = params[k].grad.cpu()
        return out

    def f64(masks):
        params = {k: host[k].double().requires_grad_() for k in keys}
        reid = reid0.double().requires_grad_()
        feats, memory = D.matcher_f64(params, name, reid, n_enc, A.NUM_DECODER_LAYERS, A.NUM_HEADS, not shared, masks)
        ((feats * G1.double()).sum() + (memory * G2.double()).sum()).backward()
        out = {"feats": feats.detach(), "memory": memory.detach(), "d reid": reid.grad}
        for k in keys:
            if params[k].grad is not None:
                out["d " + k] = params[k].grad
        return out, masks.site

    state = training.DropoutState(p, seed, iteration, rank)
    got1 = gpu(state)
    sites = 2 * A.NUM_DECODER_LAYERS if shared else 4 * n_enc + 4 * A.NUM_DECODER_LAYERS
    assert state.site == sites
    got0 = gpu(None)
    want1, used = f64(D.Masks(p, seed, iteration, rank))
    assert used == sites
    want0, _ = f64(D.Masks(None, seed))
    assert set(got1) == set(got0) == set(want1) == set(want0) and len(got1) >= 3 + 4
    assert not torch.equal(got1["feats"], got0["feats"])
    failures = []
    for k in sorted(got1):
        rel = lambda g, w: float((g.double() - w).abs().max()) / max(float(w.abs().max()), 1e-300)
        e1, e0 = rel(got1[k], want1[k]), rel(got0[k], want0[k])
        print("%-9s %-70s dropped %.3e   undropped %.3e" % (builtin + ("/s" if short else ""), k[:70], e1, e0))
        if not e1 <= 2 * e0:
            failures.append((k, e1, e0))
    assert not failures, failures


# ------------------------------------------------------------------------------------------ 5. p = 0
def test_p_zero_is_the_path_without_dropout():
    from gomatching_amd import training
    g = golden("train_asso_lst.npz")
    cfg = mini_cfg("icdar15")
    sd = synth_state_dict(cfg, seed=7)
    frames, targets, f = [], [], 0
    while "c0_f%d_pb" % f in g:
        q = lambda k: g["c0_f%d_%s" % (f, k)]
        frames.append({"image_size": (96, 128), "proposal_boxes": torch.as_tensor(q("pb")).to(DEV),
                       "objectness_logits": torch.as_tensor(q("obj")).to(DEV),
                       "query_features": torch.as_tensor(q("qf").astype(np.float32)).to(DEV)})
        targets.append({"image_size": (96, 128), "gt_boxes": torch.as_tensor(q("gt")), "gt_instance_ids": torch.as_tensor(q("ids"))})
        f += 1

    def run(state):
        params = {k: torch.nn.Parameter(torch.as_tensor(v).float().to(DEV)) for k, v in sd.items() if k.startswith("roi_heads.")}
        losses = training.asso_losses(params, cfg, frames, targets, dropout=state)
        (losses["loss_long_asso"] + losses["loss_short_asso"]).backward()
        torch.cuda.synchronize()
        return losses, params
    state = training.DropoutState(0.0, 5)
    (l0, p0), (l1, p1) = run(None), run(state)
    assert state.site == 0                                        # no site is consumed at p = 0
    for k in l0:
        assert _same_bits(l0[k], l1[k]), k
    n = 0
    for k in p0:
        assert (p0[k].grad is None) == (p1[k].grad is None), k
        if p0[k].grad is not None:
            assert _same_bits(p0[k].grad, p1[k].grad), k
            n += 1
    assert n > 20


# ------------------------------------------------------------------------------------------ 6. Trainer
def _trainer(out_dir, seed):
    """The recipe of test_solver_gpu._trainer_setup with the configs' DROPOUT."""
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.solver import Trainer
    from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip
    cfg = mini_cfg("icdar15", device="cuda")
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.1
    cfg.SOLVER.WARMUP_ITERS = 0
    cfg.SOLVER.BASE_LR = 2e-4
    sd = synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS)
    model = GoMatching(cfg, sd, device=DEV)
    return cfg, model, Trainer(cfg, model, str(out_dir), seed=seed), make_training_clip()


def _snapshot(tr):
    out = {}
    for k, q in tr.params.items():
        st = tr.optimizer.state.get(q, {})
        out[k] = (q.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else None,
                  st["exp_avg_sq"].clone() if "exp_avg_sq" in st else None, int(st["step"]) if "step" in st else 0)
    return out


@pytest.fixture(scope="module")
def run11(tmp_path_factory):
    """Three steps at seed 11, a checkpoint after the second; the trainer and its model stay open for the inference check."""
    out = tmp_path_factory.mktemp("seed11")
    cfg, model, tr, batch = _trainer(out, 11)
    hist = [tr.step(batch), tr.step(batch)]
    ck = tr.save("after2.pth")
    hist.append(tr.step(batch))
    yield {"cfg": cfg, "model": model, "trainer": tr, "batch": batch, "history": hist, "checkpoint": ck, "dir": out,
           "final": _snapshot(tr)}
    model.close()


def test_trainer_is_reproducible_per_seed_and_the_seed_matters(run11, tmp_path):
    assert run11["trainer"].dropout is not None and run11["trainer"].seed == 11 and run11["model"].dropout_state is run11["trainer"].dropout
    for h in run11["history"]:
        assert all(np.isfinite(v) for v in h.values()), h
    _, model, tr, batch = _trainer(tmp_path, 11)
    hist = [tr.step(batch) for _ in range(3)]
    for a, b in zip(hist, run11["history"]):
        assert a == b
    for k, (q, m, v, t) in _snapshot(tr).items():
        rq, rm, rv, rt = run11["final"][k]
        assert _same_bits(q, rq) and t == rt, k
        assert (m is None) == (rm is None) and (m is None or (_same_bits(m, rm) and _same_bits(v, rv))), k
    model.close()
    _, model, tr, batch = _trainer(tmp_path, 12)
    first = tr.step(batch)
    assert np.isfinite(first["total_loss"]) and first["total_loss"] != run11["history"][0]["total_loss"]
    model.close()


def test_resumed_run_equals_the_uninterrupted_one(run11, tmp_path):
    ck = torch.load(run11["checkpoint"], map_location="cpu")
    assert ck["dropout_seed"] == 11 and ck["iteration"] == 1
    _, model, tr, batch = _trainer(tmp_path, 99)
    assert tr.seed == 99
    assert tr.resume(run11["checkpoint"]) == 2 and tr.seed == 11 and tr.dropout.seed == 11
    third = tr.step(batch)
    assert third == run11["history"][2]
    for k, (q, m, v, t) in _snapshot(tr).items():
        rq, rm, rv, rt = run11["final"][k]
        assert _same_bits(q, rq) and t == rt, k
        assert (m is None) == (rm is None) and (m is None or (_same_bits(m, rm) and _same_bits(v, rv))), k
    # a checkpoint written without the key (an older file) keeps the trainer's own seed
    del ck["dropout_seed"]
    old = os.path.join(str(tmp_path), "old.pth")
    torch.save(ck, old)
    tr.seed = tr.dropout.seed = 99
    assert tr.resume(old) == 2 and tr.seed == 99 and tr.dropout.seed == 99
    model.close()


def test_inference_never_drops(run11):
    from gomatching_amd import eval as gom_eval
    from gomatching_amd.modeling import GoMatching
    from gomatching_amd.predictor import new_time_cost
    from gomatching_amd.synth import make_clip
    tr, model = run11["trainer"], run11["model"]
    frames = [{"image": torch.as_tensor(f.astype("float32").transpose(2, 0, 1)), "height": 96, "width": 128}
              for f in make_clip(6, 96, 128, clip_id=2)]

    def track(m):
        insts, idc = m.batch_inference(frames, 0, 0, [], new_time_cost())
        torch.cuda.synchronize()
        return [{"track_ids": x.track_ids.cpu().numpy(), "recs": x.recs.cpu().numpy(), "pred_boxes": x.pred_boxes.tensor.cpu().numpy(),
                 "scores": x.scores.cpu().numpy()} for x in insts], int(idc)
    path = tr.save("final.pth")
    tr.sync_inference()
    got, idc = track(model)
    again, _ = track(model)                                       # no randomness between two calls
    scratch = GoMatching(run11["cfg"], gom_eval.load_weights(path), device=DEV)
    want, idc_w = track(scratch)
    scratch.close()
    assert idc == idc_w and len(got) == len(want) == len(frames)
    for a, b, w in zip(got, again, want):
        for k in a:
            assert a[k].shape == w[k].shape and a[k].tobytes() == w[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------ 7. the META_ARCH wrapper
def test_wrapper_drops_in_train_mode_and_advances_its_iteration():
    from gomatching_amd.compat.d2_register import GoMatchingMI355X
    from gomatching_amd.synth import TRAINING_CLS_BIAS, make_training_clip
    from gomatching_amd.weights import expand_for_reference
    cfg = mini_cfg("icdar15", device="cuda")
    cfg.MODEL.ASSO_HEAD.DROPOUT = 0.1
    cfg.SEED = 5
    sd = expand_for_reference(synth_state_dict(cfg, seed=7, cls_bias=TRAINING_CLS_BIAS))
    batch = make_training_clip()

    def make():
        m = GoMatchingMI355X(cfg).to(DEV)
        m.load_state_dict(sd)
        return m.train()
    a = make()
    first, second = a(batch), a(batch)
    st = a.dropout_state
    assert st is not None and (st.p, st.seed, st.iteration, st.rank) == (0.1, 5, 1, 0) and st.site > 0
    assert all(bool(torch.isfinite(v)) for v in list(first.values()) + list(second.values()))
    assert float(first["loss_long_asso"]) != float(second["loss_long_asso"])
    assert a.eval().dropout_state is None
    b = make()
    again = b(batch)
    for k in first:
        assert _same_bits(first[k], again[k]), k
