"""CPU: the fp64 attention statement of tests/helpers.py (attention64 and its element-wise bound) is the yardstick of
test_attn_forms_gpu.py.  Here it is pinned on hand-made cases, and on every input set of the GPU file (same generators, same
seeds, same layouts: the same bits) two things are shown about the bound:

  * it is not too tight: a plain fp32 softmax attention on the CPU lies within it;
  * it is not vacuous: the statement computed under each planted mistake of MISTAKES leaves it by more than 10 x somewhere.  A
    worst-case bound grows with Lk, so a randn row of 3904 near-equal weights, or a one-hot row, can hide a dropped key; the
    `edge` inputs carry the sensitivity by construction (helpers.attn_inputs), and they are held to the condition in every case.
    The 10 x is a condition on the inputs, not a measurement.  It is asserted on the `edge` kind only: the other five kinds
    (randn, peaked, overflow, same, widev) are there for the softmax's range and for magnitudes, and on them the GPU comparison
    is a check of range, finiteness and accuracy that need not notice a tail or scale mistake -- logits in the hundreds make
    E_i larger than anything a scale error of 1 / (2 hd) can move, identical keys give the mean of v whatever the logits are.

Which mistake a case can show at all is arithmetic, not choice: with one key the output is v whatever the logits are (no mistake
about K or the scale exists for Lk = 1); key 63 exists from Lk 64, key 64 from Lk 65; the batch strides can be swapped only where
the batch has two dimensions above 1 with different strides."""
import numpy as np
import pytest
import torch

from helpers import (ATTN_CASES, ATTN_SEGMENT_KINDS, ATTN_SEGMENTS, attention64, attention64_views, attn_index, attn_pack,
                     attn_segment_inputs)

U = 2.0 ** -24


def _hand(Lq, Lk, hd=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Lq, hd, generator=g), torch.randn(Lk, hd, generator=g), torch.randn(Lk, hd, generator=g)


def test_one_key_returns_v():
    q, k, v = _hand(5, 1)
    exp, bound = attention64(q, k, v, 32)
    assert torch.equal(exp, v.double().expand(5, 32))
    # one key: p = 1, s = m -- the bound is |v_d| (2 E_i + (2 + 16) U) and the range term
    qs = (q * torch.tensor(1.0 / np.sqrt(32.0), dtype=torch.float32)).double()
    E = 34 * U * (qs.abs() @ k.double().abs().t())
    assert torch.allclose(bound, v.double().abs() * (2 * E + 18 * U) + 2.0 ** -126 * v.abs().max(), rtol=1e-12, atol=0)


def test_identical_keys_give_the_mean_of_v():
    q, k, v = _hand(4, 9)
    exp, _ = attention64(q, k[:1].expand(9, 32).contiguous(), v, 32)
    assert torch.allclose(exp, v.double().mean(0).expand(4, 32), rtol=0, atol=1e-15)


def test_one_key_200_above_the_rest_returns_its_v_row():
    q, k, v = _hand(3, 70, hd=128)
    q[1] = 0
    q[1, 0] = np.sqrt(128.0)                                               # qs = e_0: the logit of key j is k[j, 0]
    k[:, 0] = k[:, 0].clamp(-3, 3)
    k[64, 0] = 203.0
    exp, bound = attention64(q, k, v, 128)
    assert torch.allclose(exp[1], v[64].double(), rtol=0, atol=1e-80)      # the other weights are below e^-197
    assert bool(torch.isfinite(exp).all()) and bool(torch.isfinite(bound).all())


def test_permuting_the_keys_leaves_the_output():
    q, k, v = _hand(6, 67)
    perm = torch.randperm(67, generator=torch.Generator().manual_seed(1))
    a, ba = attention64(q, k, v, 32)
    b, bb = attention64(q, k[perm], v[perm], 32)
    assert torch.allclose(a, b, rtol=0, atol=1e-14) and torch.allclose(ba, bb, rtol=1e-12, atol=0)


def test_batched_call_equals_one_problem_at_a_time():
    g = torch.Generator().manual_seed(2)
    q, k, v = torch.randn(2, 3, 5, 32, generator=g), torch.randn(2, 3, 8, 32, generator=g), torch.randn(2, 3, 8, 32, generator=g)
    exp, bound = attention64(q, k, v, 32)
    for b in range(2):
        for h in range(3):
            e1, b1 = attention64(q[b, h], k[b, h], v[b, h], 32)
            assert torch.allclose(exp[b, h], e1, rtol=0, atol=1e-15) and torch.allclose(bound[b, h], b1, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------ the GPU file's inputs
def _fp32_reference(q, k, v, hd):
    return torch.softmax((q * torch.tensor(1.0 / np.sqrt(hd), dtype=torch.float32)) @ k.transpose(-1, -2), -1) @ v


def _views(case, kind):
    """(q, k, v) as generated, the layout, its buffers, and the statement read back through the op's strides."""
    q, k, v = case.inputs(kind)
    lay = case.layout()
    bufs = attn_pack(lay, q, k, v, case.outer, case.inner)
    w = lay["where"]
    exp, bound = attention64_views(bufs[w["q"][0]], bufs[w["k"][0]], bufs[w["v"][0]], case.outer, case.inner, case.heads, case.hd,
                                   case.Lq, case.Lk, lay["strides"], (w["q"][1], w["k"][1], w["v"][1]))
    return (q, k, v), lay, bufs, exp, bound


def _drop(j):
    def f(q, k, v, hd):
        keep = [i for i in range(k.shape[-2]) if i != j]
        return attention64(q, k[..., keep, :], v[..., keep, :], hd)[0]
    return f


def _swap_v_63_64(q, k, v, hd):
    v = v.clone()
    v[..., [63, 64], :] = v[..., [64, 63], :]
    return attention64(q, k, v, hd)[0]


# name -> (smallest Lk at which it exists, the statement with the mistake in it)
MISTAKES = {
    "drop the last key": (2, lambda q, k, v, hd: _drop(k.shape[-2] - 1)(q, k, v, hd)),
    "drop key 63": (64, _drop(63)),
    "drop key 64": (65, _drop(64)),
    "swap V rows 63 and 64": (65, _swap_v_63_64),
    "hd + 1 in the scale": (2, lambda q, k, v, hd: attention64(q, k, v, hd + 1)[0]),
    "head h + 1's K for head h": (2, lambda q, k, v, hd: attention64(q, k.roll(-1, -3), v, hd)[0]),
}


def _assert_visible(name, alt, exp, bound, what):
    r = float(((alt - exp).abs() / bound).max())
    assert r > 10, "%s: '%s' moves the statement by only %.2f x the bound" % (what, name, r)


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c.id for c in ATTN_CASES])
def test_bound_on_the_gpu_cases(case):
    for kind in case.kinds:
        (q, k, v), lay, bufs, exp, bound = _views(case, kind)
        # the views address exactly what was generated
        e2, b2 = attention64(q, k, v, case.hd)
        assert torch.equal(exp, e2) and torch.equal(bound, b2)
        assert bool(torch.isfinite(exp).all()) and bool(torch.isfinite(bound).all()) and bool((bound > 0).all())
        # not too tight
        err = (_fp32_reference(q, k, v, case.hd).double() - exp).abs()
        assert bool((err <= bound).all()), (case.id, kind, float((err / bound).max()))
        # not vacuous
        if kind != "edge":
            continue
        for name, (min_lk, fn) in MISTAKES.items():
            if case.Lk >= min_lk:
                _assert_visible(name, fn(q, k, v, case.hd), exp, bound, case.id)
        st = lay["strides"]
        if case.outer > 1 and case.inner > 1 and st[0] != st[1]:
            w = lay["where"]
            got = []
            for i, (n, L) in enumerate((("q", case.Lq), ("k", case.Lk), ("v", case.Lk))):
                buf = bufs[w[n][0]]
                idx = attn_index(w[n][1], st[3 * i + 1], st[3 * i], st[3 * i + 2], case.outer, case.inner, case.heads, case.hd, L,
                                 size=buf.numel())
                got.append(buf[idx].nan_to_num(0.0))
            _assert_visible("outer and inner batch strides swapped", attention64(*got, case.hd)[0], exp, bound, case.id)


@pytest.mark.parametrize("s", [i for i, (lq, lk) in enumerate(ATTN_SEGMENTS) if lq and lk])
def test_bound_on_the_segments(s):
    Lq, Lk = ATTN_SEGMENTS[s]
    for kind in ATTN_SEGMENT_KINDS:
        q, k, v = attn_segment_inputs(kind, s)
        exp, bound = attention64(q, k, v, 128)
        err = (_fp32_reference(q, k, v, 128).double() - exp).abs()
        assert bool((err <= bound).all()), (s, kind, float((err / bound).max()))
        if kind == "edge":
            for name, (min_lk, fn) in MISTAKES.items():
                if Lk >= min_lk:
                    _assert_visible(name, fn(q, k, v, 128), exp, bound, "segment %d x %d" % (Lq, Lk))


def test_every_form_and_view_is_covered():
    """The case table names each of the six forms, and each form meets the packed, the kv and the swapped view of helpers.attn_layout
    (all three NaN-filled around the operands) at least once."""
    forms = {c.form for c in ATTN_CASES}
    assert forms == {"rows32", "tile32x32", "tile32x8", "tiny128", "tile128x32", "tile128x8"}
    for f in forms:
        assert {"qkv", "kv", "swapped"} <= {c.view for c in ATTN_CASES if c.form == f}, f
