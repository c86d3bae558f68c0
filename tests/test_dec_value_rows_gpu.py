"""The decoder's sparse value projection (csrc/dec_value_rows.hip, the row-list form of csrc/gemm_k256.hip): the marked rows are
exactly the rows the gather kernel loads, the listed rows carry the dense projection's bits, and nothing else is ever read.

The restatement below follows the kernels' location arithmetic step by step (msda_corners.h): off / n as q = o * (1/n) with one
residual correction, the reference point added, pixel = fma(loc, n, -0.5), the (-1, n) acceptance window, floor, and corners
clamped onto the map -- a sample outside the window loads the map's first pixel block (h_low = w_low = 0).  Every fused multiply-add
is evaluated in float64 and rounded once (the products of two fp32 numbers are exact there)."""
import numpy as np
import pytest
import torch

from helpers import mini_cfg

DEV = "cuda"
F32 = np.float32
CONFIGS = {"four_levels": ((13, 21), (7, 11), (4, 6), (2, 3)), "flat_coarsest": ((13, 21), (7, 11), (4, 6), (1, 3))}
B, NQ, P = 2, 5, 25


def _fma(a, b, c):
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _pixels(raw, ref, levels, fused=True):
    """raw [Q, 384], ref [Q, 2] fp32 -> (loc, pix): [Q, 8, 4, 4, 2] (x, y) fp32 sampling locations and pixel coordinates."""
    Q = raw.shape[0]
    off = raw[:, :256].reshape(Q, 8, 4, 4, 2).astype(F32)
    n = np.array([[w, h] for h, w in levels], F32)[None, None, :, None, :]
    rn = (F32(1.0) / n).astype(F32)
    q = (off * rn).astype(F32)
    q = _fma(_fma(-q, n, off), rn, q)
    loc = (ref.astype(F32).reshape(Q, 1, 1, 1, 2) + q).astype(F32)
    pix = _fma(loc, n, F32(-0.5)) if fused else ((loc * n).astype(F32) - F32(0.5)).astype(F32)
    return loc, pix


def _corner_rows(pix, levels, lsi):
    """pix [Q, 8, 4, 4, 2] -> (rows [Q, 8, 4, 4, 4] int64: the four loaded rows of every sample inside its frame, inside [Q, 8, 4, 4])."""
    rows = np.zeros(pix.shape[:4] + (4,), np.int64)
    inside = np.zeros(pix.shape[:4], bool)
    for l, (H, W) in enumerate(levels):
        w_im, h_im = pix[:, :, l, :, 0], pix[:, :, l, :, 1]
        with np.errstate(invalid="ignore"):
            ins = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        h_low = np.where(ins, np.floor(np.where(ins, h_im, 0)), 0).astype(np.int64)
        w_low = np.where(ins, np.floor(np.where(ins, w_im, 0)), 0).astype(np.int64)
        yc0, yc1 = np.where(h_low >= 0, h_low, 0), np.where(h_low + 1 <= H - 1, h_low + 1, H - 1)
        xc0, xc1 = np.where(w_low >= 0, w_low, 0), np.where(w_low + 1 <= W - 1, w_low + 1, W - 1)
        for i, (y, x) in enumerate(((yc0, xc0), (yc0, xc1), (yc1, xc0), (yc1, xc1))):
            rows[:, :, l, :, i] = lsi[l] + y * W + x
        inside[:, :, l] = ins
    return rows, inside


def _flags(raw, ref, levels, lsi, S, Lq):
    """The restated byte flags [B * S] of one decoder call."""
    rows, _ = _corner_rows(_pixels(raw, ref, levels)[1], levels, lsi)
    frame = (np.arange(raw.shape[0]) // Lq).reshape(-1, 1, 1, 1, 1)
    flags = np.zeros((raw.shape[0] // Lq * S,), np.uint8)
    flags[(frame * S + rows).reshape(-1)] = 1
    return flags


def _geometry(levels):
    lsi = np.concatenate([[0], np.cumsum([h * w for h, w in levels])[:-1]]).astype(np.int64)
    return lsi, int(sum(h * w for h, w in levels))


def _inputs(levels, seed, kind="edges", nans=False):
    """raw [Q, 384] offsets | logits and ref [Q, 2].  "edges": pixel targets on -1, 0, the integers, n - 1 and n, half-way between,
    just outside and far outside every border (`nans`: and a few NaN offsets); "cover": targets spread over the whole map (every row
    loaded); "outside": every sample far outside."""
    rng = np.random.default_rng(seed)
    Q = B * NQ * P
    ref = (rng.integers(1, 64, (Q, 2)) / 64.0).astype(F32)                  # dyadic: the exact targets below are hit exactly often
    raw = rng.standard_normal((Q, 384)).astype(F32)
    off = np.zeros((Q, 8, 4, 4, 2))
    for l, (H, W) in enumerate(levels):
        for ax, n in ((0, W), (1, H)):
            shape = (Q, 8, 4)
            if kind == "cover":
                tgt = rng.uniform(-0.5, n - 0.5, shape)
            elif kind == "outside":
                tgt = rng.choice([-1e6, 1e6], size=shape)
            else:
                # (the plain samples keep to the first third of the axis, so that part of the map stays unread)
                special = np.array([-1.7, -1.0, -0.5, 0.0, 0.5, n - 1.0, n - 0.5, float(n), n + 1.3, -1e6, 3e5])
                ints = rng.integers(0, max(1, n // 3), shape).astype(np.float64)
                pick = rng.integers(0, 8, shape)
                tgt = np.where(pick == 0, special[rng.integers(0, len(special), shape)],
                               np.where(pick <= 3, ints, rng.uniform(-2.0, n / 3.0, shape)))
            off[:, :, l, :, ax] = ((tgt + 0.5) / n - ref[:, ax].astype(np.float64)[:, None, None]) * n
    raw[:, :256] = off.reshape(Q, 256).astype(F32)
    if nans:
        raw[rng.integers(0, Q, 6), rng.integers(0, 256, 6)] = np.nan
    return raw, ref


def _ops():
    from gomatching_amd import ops
    return ops


class _Case:
    """One configuration on the device: memory, a two-layer value weight (the second layer's row slice is used), dense projection, inputs."""

    def __init__(self, name, kind="edges", seed=0):
        ops = _ops()
        self.levels = CONFIGS[name]
        self.lsi_np, self.S = _geometry(self.levels)
        self.raw_np, self.ref_np = _inputs(self.levels, seed + 11, kind)
        self.Lq = NQ * P
        g = torch.Generator().manual_seed(seed + 5)
        self.memory = torch.randn((B * self.S, 256), generator=g).to(DEV)
        self.shapes = torch.tensor(self.levels, dtype=torch.int64, device=DEV)
        self.lsi = torch.from_numpy(self.lsi_np).to(DEV)
        with ops.gemm_mode("f16x3"):
            w = ops.prep_weight((torch.randn((512, 256), generator=g) * 0.06).to(DEV))
            bias = torch.randn((512,), generator=g).to(DEV)
            self.lin_all = ops.K256Linear(w, bias)
            self.lin = ops.K256Linear(w[256:512], bias[256:512])             # a row slice, as a decoder layer's
            self.dense = ops.linear(self.memory, self.lin_all, groups=1)    # [B*S, 512]: the dense launch
        self.raw = torch.from_numpy(self.raw_np).to(DEV)
        self.ref = torch.from_numpy(self.ref_np).to(DEV)
        self.want = _flags(self.raw_np, self.ref_np, self.levels, self.lsi_np, self.S, self.Lq)

    def state(self, fill=0.0):
        st = _ops().DecValueRows(B * self.S, DEV)
        st.value.fill_(fill)
        return st

    def sparse(self, st, raw=None, ref=None):
        """mark -> compact -> row-list GEMM -> gather, as DeepSolo._dec_value_rows and the layer's sampling issue them."""
        ops = _ops()
        raw, ref = self.raw if raw is None else raw, self.ref if ref is None else ref
        ops.dec_value_mark(raw, ref, self.shapes, self.lsi, B, self.Lq, self.S, st)
        ops.dec_value_compact(st)
        ops.linear_rows(self.memory, self.lin, st)
        return ops.msda_fused(raw, ref, st.value, self.S * 256, self.shapes, self.lsi, B, self.Lq)

    def dense_out(self, values, raw=None, ref=None):
        raw, ref = self.raw if raw is None else raw, self.ref if ref is None else ref
        return _ops().msda_fused(raw, ref, values[:, 256:], self.S * values.stride(0), self.shapes, self.lsi, B, self.Lq)


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def case(request):
    return _Case(request.param)


def test_restatement_against_the_oracle_index_arithmetic(monkeypatch):
    """CPU: the restated corner rows of every sample inside the window are the rows `oracle.gom_oracle.ms_deform_attn_forward` gathers
    for the same locations (its pixel coordinate is loc * n - 0.5 in two roundings, so the restatement is taken unfused here)."""
    from oracle import gom_oracle as O
    levels = CONFIGS["four_levels"]
    lsi, S = _geometry(levels)
    raw, ref = _inputs(levels, 3)
    Q, Lq = raw.shape[0], NQ * P
    loc, pix = _pixels(raw, ref, levels, fused=False)
    rows, inside = _corner_rows(pix, levels, lsi)
    assert inside.any() and (~inside).any()
    seen = []
    real = torch.Tensor.index_select
    monkeypatch.setattr(torch.Tensor, "index_select", lambda self, dim, index: (seen.append(index.clone()), real(self, dim, index))[1])
    O.ms_deform_attn_forward(torch.zeros((B, S, 8, 1)), torch.tensor(levels), torch.from_numpy(lsi),
                             torch.from_numpy(loc).view(B, Lq, 8, 4, 4, 2), torch.ones((B, Lq, 8, 4, 4)), q_chunk=0)
    monkeypatch.undo()
    assert len(seen) == 16                                                  # four corners of four levels, in (dy, dx) order
    frame = (np.arange(Q) // Lq).reshape(Q, 1, 1)
    for l in range(4):
        for i in range(4):
            got = (seen[4 * l + i].numpy() // 8).reshape(Q, 8, 4) - frame * S
            assert np.array_equal(got[inside[:, :, l]], rows[:, :, l, :, i][inside[:, :, l]]), (l, i)


@pytest.mark.gpu
def test_flags_equal_the_restatement(case):
    ops = _ops()
    pix = _pixels(case.raw_np, case.ref_np, case.levels)[1]
    for l, (H, W) in enumerate(case.levels):                                # the inputs do sit on the edges they are meant to
        for ax, n in ((0, W), (1, H)):
            # (0 itself is met on power-of-two axes only: next to 0 fp32 is too fine for fma(loc, n, -0.5) to round onto it)
            for edge in (-1.0, n - 1.0, float(n)):
                assert (pix[:, :, l, :, ax] == edge).any(), (l, ax, edge)
            with np.errstate(invalid="ignore"):
                assert (pix[:, :, l, :, ax] < -1).any() and (pix[:, :, l, :, ax] > n).any()
    st = case.state()
    ops.dec_value_mark(case.raw, case.ref, case.shapes, case.lsi, B, case.Lq, case.S, st)
    got = st.flags.cpu().numpy()
    assert np.array_equal(got[:B * case.S], case.want), np.flatnonzero(got[:B * case.S] != case.want)[:8]
    assert not got[B * case.S:].any()
    ops.dec_value_compact(st)
    count = int(st.count.item())
    assert np.array_equal(st.rows[:count].cpu().numpy(), np.flatnonzero(case.want))
    assert count % 32 and count % 128 and count < B * case.S              # a ragged last wave and tile
    # NaN offsets: the sample is outside the window and loads the first pixel block, as in the gather kernel
    raw_np, ref_np = _inputs(case.levels, 21, nans=True)
    assert np.isnan(_pixels(raw_np, ref_np, case.levels)[1]).any()
    st = case.state()
    ops.dec_value_mark(torch.from_numpy(raw_np).to(DEV), torch.from_numpy(ref_np).to(DEV), case.shapes, case.lsi, B, case.Lq, case.S, st)
    assert np.array_equal(st.flags.cpu().numpy()[:B * case.S], _flags(raw_np, ref_np, case.levels, case.lsi_np, case.S, case.Lq))


@pytest.mark.gpu
def test_poisoned_buffers_and_listed_rows(case):
    """Sparse path into a NaN-filled buffer: no NaN reaches the sampling, output = the dense path's, bit for bit; the listed rows are
    the dense rows; the flags are zero again; and the dense path with its UNLISTED rows poisoned gives the same output."""
    want = case.dense_out(case.dense)
    assert not torch.isnan(want).any()
    st = case.state(float("nan"))
    got = case.sparse(st)
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    listed = torch.from_numpy(case.want.astype(bool)).to(DEV)
    assert torch.equal(st.value[listed], case.dense[:, 256:][listed])
    assert bool(torch.isnan(st.value[~listed]).all())
    assert not bool(st.flags.any())
    poisoned = case.dense.clone()
    poisoned[~listed] = float("nan")
    assert torch.equal(case.dense_out(poisoned), want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cover", "outside"])
def test_every_row_and_first_pixels_only(kind):
    """Offsets spread over the whole map list every row; samples all far outside load the first pixel block of every level."""
    c = _Case("four_levels", kind, seed=2)
    st = c.state(float("nan"))
    got = c.sparse(st)
    count = int(st.count.item())
    if kind == "cover":
        assert count == B * c.S
    else:
        assert count == B * 16 and not bool(got.any())                      # every weight is zero
    assert count == int(c.want.sum())
    assert torch.equal(got, c.dense_out(c.dense))


@pytest.mark.gpu
def test_one_row_per_frame():
    """Compaction and the row-list GEMM on a hand-made list: one row per frame, the last row of the last frame among them."""
    ops = _ops()
    c = _Case("flat_coarsest", seed=4)
    st = c.state(float("nan"))
    rows = [7, 2 * c.S - 1]
    st.flags[rows] = 1
    ops.dec_value_compact(st)
    assert int(st.count.item()) == 2 and st.rows[:2].tolist() == rows
    ops.linear_rows(c.memory, c.lin, st)
    assert torch.equal(st.value[rows], c.dense[:, 256:][rows])
    assert int(torch.isnan(st.value).any(1).sum()) == B * c.S - 2 and not bool(st.flags.any())


@pytest.mark.gpu
def test_graph_replay_with_another_count(case):
    """The four launches captured once, replayed on other offsets (another count): what eager gives for them."""
    raw2, ref2 = (torch.from_numpy(a).to(DEV) for a in _inputs(case.levels, 77, "cover"))
    raw, ref = case.raw.clone(), case.ref.clone()
    st = case.state()
    case.sparse(st, raw, ref)                                               # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = case.sparse(st, raw, ref)
    g.replay()
    first, n_first = out.clone(), int(st.count.item())
    assert torch.equal(first, case.dense_out(case.dense))
    raw.copy_(raw2), ref.copy_(ref2)
    g.replay()
    assert int(st.count.item()) == B * case.S != n_first
    assert torch.equal(out, case.dense_out(case.dense, raw2, ref2))
    assert torch.equal(out, case.sparse(case.state(float("nan")), raw2, ref2))


@pytest.mark.gpu
@pytest.mark.parametrize("fused_raw", [True, False])
def test_switch_and_policy_leave_the_predictions_alone(fused_raw):
    """DeepSolo on the features of a 97 x 161 frame: switch off, on, and the policy forced to the dense launch -- the same pred_*; both
    producers of the offsets | logits (the inter block's launch, and the separate product with ops.DEC_ATTN_RAW off)."""
    ops = _ops()
    from gomatching_amd.weights import synth_state_dict
    from gomatching_amd.modeling import DeepSolo
    cfg = mini_cfg("icdar15")
    sd = synth_state_dict(cfg, seed=7)
    gen = torch.Generator().manual_seed(3)
    feats = [(torch.randn((2, h, w, c), generator=gen) * 0.5).to(DEV) for (h, w), c in zip(((13, 21), (7, 11), (4, 6)), (512, 1024, 2048))]
    old = ops.DEC_VALUE_SPARSE, ops.DEC_VALUE_MAX_SHARE, ops.DEC_ATTN_RAW
    outs = {}
    try:
        ops.DEC_ATTN_RAW = fused_raw
        with ops.gemm_mode("f16x3"):
            for name, on, share in (("off", False, old[1]), ("on", True, 1.0), ("dense", True, -1.0)):
                ops.DEC_VALUE_SPARSE, ops.DEC_VALUE_MAX_SHARE = on, share
                net = DeepSolo(cfg, sd, DEV)
                first = net.forward(feats)
                outs[name] = net.forward(feats)                             # the second call runs what the first one decided
                for k in first:
                    if k.startswith("pred_"):
                        assert torch.equal(first[k], outs[name][k]), (name, k)
                if name == "off":
                    assert net.dec_value_share == {} and net.dec_value_dense is None
                else:
                    assert sorted(net.dec_value_share) == list(range(net.n_dec)) and net.dec_value_dense is (name == "dense")
                    assert all(0.0 < s <= 1.0 for s in net.dec_value_share.values())
    finally:
        ops.DEC_VALUE_SPARSE, ops.DEC_VALUE_MAX_SHARE, ops.DEC_ATTN_RAW = old
    keys = [k for k in outs["off"] if k.startswith("pred_")]
    assert len(keys) >= 4
    for name in ("on", "dense"):
        for k in keys:
            assert torch.equal(outs["off"][k], outs[name][k]), (name, k)
