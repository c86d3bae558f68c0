"""The decoder's sparse value projection against the dense launch, by the share of rows listed (ops.DEC_VALUE_MAX_SHARE).

At the bench shape (8 frames of 1000 x 1778: 37 171 tokens each, 100 queries x 25 points) with synthetic queries -- first on fewer
distinct text lines than queries (a detector's queries crowd onto the same words), then with the offsets scaled up until every row is
listed: a layer's three launches (mark, compact, row-list GEMM; csrc/dec_value_rows.hip, csrc/gemm_k256.hip), each
alone and as a triple, ALTERNATING with the dense N = 1536 launch whose sixth a layer has to beat.  Bursts of back-to-back launches,
median of the bursts.  The last line names the share where the triple meets a sixth of the dense launch."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from gomatching_amd import ops

ops.GEMM_MODE = "f16x3"
dev = "cuda"
LEVELS = ((125, 223), (63, 112), (32, 56), (16, 28))
B, NQ, P = 8, 100, 25


def burst(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def ab(fns, rounds=7):
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            ts[i].append(burst(f))
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    g = torch.Generator().manual_seed(0)
    S = sum(h * w for h, w in LEVELS)
    shapes = torch.tensor(LEVELS, dtype=torch.int64, device=dev)
    lsi = torch.tensor([0] + [sum(h * w for h, w in LEVELS[:i]) for i in range(1, 4)], dtype=torch.int64, device=dev)
    memory = torch.randn((B * S, 256), generator=g).to(dev)
    sw = ops.split_weight((torch.randn((1536, 256), generator=g) * 0.06).to(dev), kind="f16x3")
    bias = torch.randn((1536,), generator=g).to(dev)
    dense_lin, lin = ops.K256Linear(sw, bias), ops.K256Linear(sw[:256], bias[:256])
    dense_out = torch.empty((B * S, 1536), device=dev)
    st = ops.DecValueRows(B * S, dev)
    Q = B * NQ * P
    # queries as text lines: a centre per line, the 25 points of a query along a short horizontal run
    centres = torch.rand((B, NQ, 1, 2), generator=g) * 0.8 + 0.1
    run = torch.linspace(-0.04, 0.04, P).view(1, 1, P, 1) * torch.tensor([1.0, 0.05])
    base = torch.randn((Q, 384), generator=g)
    dense = lambda: ops.linear(memory, dense_lin, out=dense_out, groups=1)
    mark = compact = None
    rows = []
    for lines, scale in ((3, 1), (6, 1), (12, 1), (25, 1), (50, 1), (100, 1), (100, 2), (100, 4), (100, 8), (100, 16), (100, 32)):
        ref = (centres[:, torch.arange(NQ) % lines] + run).view(Q, 2).contiguous().to(dev)
        raw = base.clone()
        raw[:, :256] *= scale
        raw = raw.to(dev)
        mark = lambda: ops.dec_value_mark(raw, ref, shapes, lsi, B, NQ * P, S, st)
        compact = lambda: ops.dec_value_compact(st)
        gemm = lambda: ops.linear_rows(memory, lin, st, clear=False)
        st.flags.zero_()
        mark(), compact()
        share = float(st.count.item()) / (B * S)

        def triple():
            mark(), compact(), ops.linear_rows(memory, lin, st)

        t = ab([dense, mark, compact, gemm, triple])
        rows.append((share, t[4], t[0] / 6))
        print("%3d lines, offsets x %2d  share %5.1f %%  mark %5.1f us  compact %5.1f us  row-list GEMM %6.1f us  the three %6.1f us | dense N=1536 "
              "%6.1f us, a sixth %6.1f us" % (lines, scale, 100 * share, t[1], t[2], t[3], t[4], t[0], t[0] / 6), flush=True)
    even = None
    for (s0, a0, d0), (s1, a1, d1) in zip(rows, rows[1:]):
        if a0 <= d0 and a1 > d1:                               # linear between the two measured shares
            f = (d0 - a0) / ((a1 - d1) + (d0 - a0))
            even = s0 + f * (s1 - s0)
    print("the three launches meet a sixth of the dense launch at a share of %s" % ("%.1f %%" % (100 * even) if even is not None else
                                                                                  "-- (not inside the measured range)"))


if __name__ == "__main__":
    main()
