"""Host restatement of the dropout contract of the association head's training path ("Dropout"):

  * `philox4x32_10` / `keep_mask`: the mask stream in numpy -- Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
    (e >> 2, site, iteration, rank) for logical element e, which uses output word e & 3 and is kept iff
    word >= floor(p 2^32); kept values are scaled by float32(1 / (1 - p));
  * `matcher_f64`: the matcher forward of `matcher_transformer` (roi_heads/transformer.py:60-96 of the reference with
    norm = Identity, `forward_post`) in float64 torch: linear, per-head attention, residuals, with the masks injected at the
    sites in call order.  Differentiable by torch's autograd, which is the statement of the backward.

Independent of gomatching_amd.training (never imported here): written from the contract, not from the code under test."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> the 4 output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _U32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _U32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return int(math.floor(float(p) * 4294967296.0))


def scale_f32(p):
    return np.float32(1.0 / (1.0 - float(p)))


def keep_mask(seed, site, iteration, rank, n, p):
    """bool [n]: element e of the stream (seed, site, iteration, rank) is kept."""
    n = int(n)
    assert (max(n, 1) - 1) >> 2 < 1 << 32
    groups = (n + 3) // 4
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((np.arange(groups, dtype=np.uint64), site, iteration, rank), (seed & 0xFFFFFFFF, seed >> 32))
    flat = np.stack(words, axis=1).reshape(-1)[:n]
    return flat.astype(np.uint64) >= np.uint64(threshold(p))


class Masks:
    """Hands out the multiplier (mask * scale as float64 of the float32 scale) of each site in call order; p = None: ones."""

    def __init__(self, p, seed, iteration=0, rank=0):
        self.p, self.seed, self.iteration, self.rank, self.site = p, seed, iteration, rank, 0

    def next(self, shape):
        import torch
        site = self.site
        self.site += 1
        n = int(np.prod(shape))
        if self.p is None:
            return torch.ones(tuple(shape), dtype=torch.float64)
        keep = keep_mask(self.seed, site, self.iteration, self.rank, n, self.p)
        return torch.from_numpy(keep.astype(np.float64) * float(scale_f32(self.p))).reshape(tuple(shape))


def _mha_f64(q_in, kv_in, params, name, heads, masks):
    import torch
    E = q_in.shape[1]
    w, b = params[name + ".in_proj_weight"], params[name + ".in_proj_bias"]
    q = q_in @ w[:E].T + b[:E]
    k = kv_in @ w[E:2 * E].T + b[E:2 * E]
    v = kv_in @ w[2 * E:].T + b[2 * E:]
    hd = E // heads
    Lq, Lk = q.shape[0], k.shape[0]
    qh = q.reshape(Lq, heads, hd).permute(1, 0, 2)
    kh = k.reshape(Lk, heads, hd).permute(1, 0, 2)
    vh = v.reshape(Lk, heads, hd).permute(1, 0, 2)
    P = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(hd), dim=-1)          # [heads, Lq, Lk]: the logical tensor
    P = P * masks.next(P.shape)
    a = (P @ vh).permute(1, 0, 2).reshape(Lq, E)
    return a @ params[name + ".out_proj.weight"].T + params[name + ".out_proj.bias"]


def _ffn_f64(x, params, p, masks):
    import torch
    h = torch.relu(x @ params[p + "linear1.weight"].T + params[p + "linear1.bias"])
    h = h * masks.next(h.shape)
    return h @ params[p + "linear2.weight"].T + params[p + "linear2.bias"]


def matcher_f64(params, name, reid, n_enc, n_dec, heads, dec_ffn, masks):
    """params: {key: float64 tensor}; name: e.g. "roi_heads.long_term_matcher" -> (feats, memory) in float64."""
    memory = reid
    for i in range(n_enc):
        p = "%s.encoder.layers.%d." % (name, i)
        a = _mha_f64(memory, memory, params, p + "self_attn", heads, masks)
        memory = memory + a * masks.next(a.shape)
        f = _ffn_f64(memory, params, p, masks)
        memory = memory + f * masks.next(f.shape)
    tgt = reid
    for i in range(n_dec):
        p = "%s.decoder.layers.%d." % (name, i)
        a = _mha_f64(tgt, memory, params, p + "multihead_attn", heads, masks)
        tgt = tgt + a * masks.next(a.shape)
        if dec_ffn:
            f = _ffn_f64(tgt, params, p, masks)
            tgt = tgt + f * masks.next(f.shape)
    return tgt, memory
