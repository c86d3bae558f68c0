"""DeepSolo-without-backbone on MI355X, batched over the frames of a step.

Host-side mirror of `DETECTION_TRANSFORMER_WOBACKBONE.forward`
(/root/reference/third_party/adet/modeling/model/detection_transformer_wobackbone.py:159-270) and
`DeformableTransformer.forward` (third_party/adet/layers/deformable_transformer.py:150-215), driving the
HIP kernels through `gomatching_amd.ops`.  Results are identical in meaning; the schedule is not the
reference's:
  * tokens are channels-last from the backbone on, so flatten/transpose/cat are free: GroupNorm writes
    each level straight into the flattened [B,S,256] buffer;
  * sampling_offsets and attention_weights share one GEMM (N = 384) fed by (src + pos) added in the
    operand loader; residual adds ride in GEMM epilogues, LayerNorm fuses the add it needs;
  * the six decoder cross-attention value projections (same memory, six weights,
    ms_deform_attn.py:133) are ONE GEMM with N = 1536 right after the encoder -- or, per layer, the projection of
    just the rows that layer's sampling loads (ops.DEC_VALUE_SPARSE: mark, compact, row-list GEMM);
  * the Bezier-coordinate MLP runs on the nq selected tokens only (the reference runs it on all S
    tokens and gathers afterwards, deformable_transformer.py:185-196) -- same values, ~S/nq fewer FLOPs;
  * instead of zero-filling invalid-proposal rows before enc_output (:136-137), their class logit
    (a constant: the head applied to a zero row) is substituted inside the top-k kernel;
  * position tables (sine encodings + level embed, encoder reference grid, proposal validity) are
    computed on the GPU once per input resolution and cached.
Padding masks: the reference feeds one unpadded image per call (gom_lstmatcher.py:369-371), so masks are
all-False and valid ratios are 1; that is the only case built (frames of one step share a size).
"""
import math

import torch

from .. import ops

_f32 = torch.float32


def _dev(t, device):
    return t.detach().float().contiguous().to(device)


class _SparseValues:
    """What the decoder layers of ONE step get in place of the dense value buffer: the resolution's ops.DecValueRows, the encoder
    memory the listed rows are projected from, and whether this step measures the layers' shares."""

    def __init__(self, state, memory, measure):
        self.state, self.memory, self.measure = state, memory, measure


class DeepSolo:
    def __init__(self, cfg, sd, device, prefix="detection_transformer."):
        T = cfg.MODEL.TRANSFORMER
        self.cfg, self.device = cfg, device
        self.d, self.nq, self.P = T.HIDDEN_DIM, T.NUM_QUERIES, T.NUM_POINTS
        self.nheads, self.L = T.NHEADS, T.NUM_FEATURE_LEVELS
        self.n_enc, self.n_dec = T.ENC_LAYERS, T.DEC_LAYERS
        self.voc = T.VOC_SIZE
        assert self.d == 256 and self.nheads == 8 and self.L == 4 and T.ENC_N_POINTS == 4 and T.DEC_N_POINTS == 4, \
            "kernels are specialised for d_model 256 / 8 heads / 4 levels / 4 points (every shipped config)"
        assert T.BOUNDARY_HEAD
        g = lambda k: _dev(sd[prefix + k], device)
        self.proj = []
        for l in range(3):
            self.proj.append((ops.prep_weight(g("input_proj.%d.0.weight" % l).reshape(self.d, -1).contiguous()),
                              g("input_proj.%d.0.bias" % l), g("input_proj.%d.1.weight" % l),
                              g("input_proj.%d.1.bias" % l)))
        w3 = sd[prefix + "input_proj.3.0.weight"].float().permute(0, 2, 3, 1)          # OHWI
        cin = w3.shape[-1]
        self.proj3_cin = 1 << (cin - 1).bit_length()     # the implicit-GEMM conv wants a power-of-two Cin (Swin: 768 -> 1024)
        if self.proj3_cin != cin:
            w3 = torch.cat([w3, w3.new_zeros(w3.shape[:-1] + (self.proj3_cin - cin,))], -1)
        self.proj3 = (ops.prep_conv_weight(_dev(w3, device)),
                      g("input_proj.3.0.bias"), g("input_proj.3.1.weight"), g("input_proj.3.1.bias"))
        self.point_embed = g("point_embed.weight")                           # [nq*P, 256]
        t = "transformer."
        self.level_embed = g(t + "level_embed")
        self.enc_output = (ops.prep_weight(g(t + "enc_output.weight")), g(t + "enc_output.bias"))
        self.enc_output_norm = (g(t + "enc_output_norm.weight"), g(t + "enc_output_norm.bias"))

        def lin(name):                                       # nn.Linear: weight goes through the GEMM weight policy
            return ops.prep_weight(g(name + ".weight")), g(name + ".bias")

        def norm(name):                                      # LayerNorm gain / bias stay plain fp32 vectors
            return g(name + ".weight"), g(name + ".bias")

        def ffn(p, norm_name):
            """linear1 -> ReLU -> linear2 -> + residual -> norm as ONE launch (csrc/ffn_fused.hip) under the f16x3 back-end:
            the hidden activations never reach HBM (13 KB -> 2 KB per token).  None: the three-launch path."""
            if ops.GEMM_MODE != "f16x3" or not ops.FUSED_FFN or T.DIM_FEEDFORWARD % 32:
                return None
            return ops.FusedFFN(g(p + "linear1.weight"), g(p + "linear1.bias"), g(p + "linear2.weight"),
                                g(p + "linear2.bias"), g(p + norm_name + ".weight"), g(p + norm_name + ".bias"))

        def msda(name):
            w = torch.cat([sd[prefix + name + ".sampling_offsets.weight"],
                           sd[prefix + name + ".attention_weights.weight"]], 0)
            b = torch.cat([sd[prefix + name + ".sampling_offsets.bias"],
                           sd[prefix + name + ".attention_weights.bias"]], 0)
            wv, bv = sd[prefix + name + ".value_proj.weight"], sd[prefix + name + ".value_proj.bias"]
            return {"raw": (ops.prep_weight(_dev(w, device)), _dev(b, device)), "value": lin(name + ".value_proj"),
                    "out": lin(name + ".output_proj"),
                    # encoder: offsets | attention logits | value projection as ONE [640, 256] GEMM
                    "raw_value": (ops.prep_weight(_dev(torch.cat([w, wv], 0), device)),
                                  _dev(torch.cat([b, bv], 0), device))}

        self.enc = []
        self._msda_counter = None                                # one int32 device word: fallback octet groups of a window launch
        self.msda_window_fallback = {}                           # encoder layer -> measured share (ops.MSDA_WINDOW_POLICY)
        for i in range(self.n_enc):
            p = t + "encoder.layers.%d." % i
            attn, n1 = msda(p + "self_attn"), norm(p + "norm1")
            # long problem, N = 640: the row-resident K = 256 kernel's whole-line-store form under the f16x3 back-end
            attn["raw_value"] = ops.k256_linear(*attn["raw_value"])
            self.enc.append({"attn": attn, "norm1": n1, "lin1": lin(p + "linear1"),
                             "lin2": lin(p + "linear2"), "norm2": norm(p + "norm2"), "ffn": ffn(p, "norm2"),
                             # out_proj + residual + norm1 as one launch (csrc/proj_ln.hip) under the f16x3 back-end, else None
                             "out_ln": ops.proj_ln_block(attn["out"], n1)})
        def qlin(pair):
            """A Q-side layer of the decoder (M = frames x queries x points rows): the row-resident K = 256 kernel under
            the f16x3 back-end (csrc/gemm_k256.hip), otherwise the pair as it is (ops.linear serves both)."""
            return ops.k256_linear(*pair)

        E = self.d
        self.dec = []
        for i in range(self.n_dec):
            p = t + "decoder.layers.%d." % i
            wi, bi = ops.prep_weight(g(p + "attn_intra.in_proj_weight")), g(p + "attn_intra.in_proj_bias")
            cross = msda(p + "attn_cross")
            cross["raw"], cross["out"] = qlin(cross["raw"]), qlin(cross["out"])
            intra_out, inter_out = lin(p + "attn_intra.out_proj"), lin(p + "attn_inter.out_proj")
            n_intra, n_inter, n_cross = norm(p + "norm_intra"), norm(p + "norm_inter"), norm(p + "norm_cross")
            wx, bx = ops.prep_weight(g(p + "attn_inter.in_proj_weight")), g(p + "attn_inter.in_proj_bias")
            self.dec.append({
                # the whole block (in_proj, attention, out_proj, residual, norm) as ONE launch under the f16x3 back-end, else None
                "intra_block": ops.dec_attn_block(wi, bi, intra_out, n_intra, inter=False),
                # up to 128 queries per frame one launch (csrc/dec_attn.hip); up to 352 (GoMatching++: 300) the block's image feeds
                # csrc/dec_inter.hip (in_proj + attention per (group, head)) followed by the out_proj + LayerNorm launch
                # ... with the cross attention's offsets | logits product (N = 384) on its output in the same launch (<= 128 queries)
                "inter_block": ops.dec_attn_block(wx, bx, inter_out, n_inter, inter=True,
                                                  raw=cross["raw"] if self.nq <= ops.DEC_INTER_MAX_FUSED else None)
                if self.nq <= ops.DEC_INTER_MAX_HEADS else None,
                "intra_qk": qlin((wi[:2 * E], bi[:2 * E])), "intra_v": qlin((wi[2 * E:], bi[2 * E:])),
                "intra_out": qlin(intra_out), "norm_intra": n_intra, "intra_out_ln": ops.proj_ln_block(intra_out, n_intra),
                "inter_in": qlin((wx, bx)),
                "inter_out": qlin(inter_out), "norm_inter": n_inter, "inter_out_ln": ops.proj_ln_block(inter_out, n_inter),
                "cross": cross, "norm_cross": n_cross, "cross_out_ln": ops.proj_ln_block(cross["out"], n_cross),
                "lin1": lin(p + "linear1"), "lin2": lin(p + "linear2"), "norm3": norm(p + "norm3"),
                "ffn": ffn(p, "norm3")})
        # all six cross-attention value projections as one [6*256, 256] weight
        vp = [t + "decoder.layers.%d.attn_cross.value_proj" % i for i in range(self.n_dec)]
        self.dec_value = qlin((ops.prep_weight(torch.cat([g(n + ".weight") for n in vp], 0).contiguous()),
                               torch.cat([g(n + ".bias") for n in vp], 0).contiguous()))
        # ... and each layer's [256, 256] row slice of it for the sparse form (ops.DEC_VALUE_SPARSE): the same planes and row scales
        self.dec_value_layers = [ops.K256Linear(self.dec_value.W[i * E:(i + 1) * E], self.dec_value.bias[i * E:(i + 1) * E])
                                 for i in range(self.n_dec)] if isinstance(self.dec_value, ops.K256Linear) else None
        self.dec_value_share = {}                                # decoder layer -> measured share of value rows its sampling loads
        self.dec_value_dense = None                              # None: not decided yet (ops.DEC_VALUE_POLICY); True: the dense launch
        self._dec_value_states = {}                              # (frames, tokens, device) -> ops.DecValueRows
        self.ref_point_head = [qlin(lin(t + "decoder.ref_point_head.layers.%d" % i)) for i in range(2)]

        def mlp2(name, relu_out):                            # two 256 x 256 layers as ONE launch (f16x3 back-end), else None
            return ops.mlp2_block(g(name + ".layers.0.weight"), g(name + ".layers.0.bias"), g(name + ".layers.1.weight"),
                                  g(name + ".layers.1.bias"), relu_out)

        self.ref_point_mlp2 = mlp2(t + "decoder.ref_point_head", False)
        self.ctrl_coord_mlp2 = mlp2("ctrl_point_coord.0", True)
        self.boundary_mlp2 = mlp2("boundary_offset.0", True)
        self.bezier_coord = [lin("bezier_proposal_coord.layers.%d" % i) for i in range(3)]
        self.bezier_class = lin("bezier_proposal_class")
        # enc_output + enc_output_norm + the class logit of every token as ONE launch under the f16x3 back-end (csrc/proj_ln.hip,
        # dot form): the normalised rows never reach HBM, the nq winners' rows are recomputed from their gathered memory rows
        self.enc_output_ln = ops.proj_ln_block(self.enc_output, self.enc_output_norm) if ops.PROPOSAL_DOT else None
        if self.enc_output_ln is not None:
            self._cls_w = self.bezier_class[0].reshape(256).contiguous()
            self._cls_b = float(self.bezier_class[1].reshape(-1)[0])
        self.ctrl_coord = [qlin(lin("ctrl_point_coord.0.layers.%d" % i)) for i in range(3)]      # last layer (N = 2): a pair
        self.ctrl_class = lin("ctrl_point_class.0")
        self.ctrl_text = lin("ctrl_point_text.0")
        self.boundary = [qlin(lin("boundary_offset.0.layers.%d" % i)) for i in range(3)]

        dim_t = torch.arange(128, dtype=_f32)
        dim_t = T.TEMPERATURE ** (2 * torch.div(dim_t, 2, rounding_mode="trunc") / 128)
        self.dim_t = dim_t.to(device)
        # the row-local tail of every decoder layer -- FFN + norm3, ctrl_point_coord + reference refinement, the NEXT layer's
        # ref_point_head over the sine embedding of the refined points -- as ONE launch (csrc/dec_tail.hip), f16x3 back-end
        wb = lambda name: (g(name + ".weight"), g(name + ".bias"))
        for i, L in enumerate(self.dec):
            p = t + "decoder.layers.%d." % i
            L["tail"] = ops.dec_tail_block(
                (g(p + "linear1.weight"), g(p + "linear1.bias"), g(p + "linear2.weight"), g(p + "linear2.bias"),
                 g(p + "norm3.weight"), g(p + "norm3.bias")),
                [wb("ctrl_point_coord.0.layers.%d" % k) for k in range(3)],
                [wb(t + "decoder.ref_point_head.layers.%d" % k) for k in range(2)], self.dim_t,
                # ... and the cross attention's out_proj + norm_cross in front of it: the launch starts from the sampled rows
                proj_w=wb(p + "attn_cross.output_proj") + wb(p + "norm_cross")) if T.DIM_FEEDFORWARD % 32 == 0 else None
        from scipy.special import comb                      # the reference's table (deformable_transformer.py:83-86)
        ts = torch.linspace(0, 1, self.P)
        self.bernstein = torch.tensor([[tt ** k * (1 - tt) ** (3 - k) * comb(3, k) for k in range(4)]
                                       for tt in ts]).to(device)
        self._geom = {}
        self._geom_transient = False        # True: `geometry` builds without keeping (training on motion clips: new sizes every step)
        self._invalid_logit = None

    # --------------------------------------------------------------------------------- tables
    @staticmethod
    def level_shapes(h, w):
        """Spatial sizes of res3/res4/res5 and the extra stride-64 level for an h x w network input."""
        def c(x, k, s, p):
            return (x + 2 * p - k) // s + 1
        h2, w2 = c(c(h, 7, 2, 3), 3, 2, 1), c(c(w, 7, 2, 3), 3, 2, 1)
        shapes = []
        for _ in range(3):
            h2, w2 = c(h2, 3, 2, 1), c(w2, 3, 2, 1)
            shapes.append((h2, w2))
        shapes.append((c(h2, 3, 2, 1), c(w2, 3, 2, 1)))
        return shapes

    @staticmethod
    def valid_shapes(shapes, image_hw, strides=(8, 16, 32)):
        """Valid (unpadded) extent of every level for an image of `image_hw` inside a padded batch: ceil(size / stride)
        for the backbone levels (gom_lstmatcher.py:63-76); the extra level takes the nearest-neighbour resampling of the
        FIRST level's mask (detection_transformer_wobackbone.py:177-178) with torch's float source-index rule."""
        import numpy as np
        v = [(min(-(-image_hw[0] // s), H), min(-(-image_hw[1] // s), W)) for s, (H, W) in zip(strides, shapes[:3])]

        def resample(n_in, n_out, n_valid):
            scale = np.float32(n_in) / np.float32(n_out)
            src = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
            return int((src < n_valid).sum())

        v.append((resample(shapes[0][0], shapes[3][0], v[0][0]), resample(shapes[0][1], shapes[3][1], v[0][1])))
        return v

    @staticmethod
    def valid_shapes_frames(shapes, image_sizes, strides=(8, 16, 32)):
        """`valid_shapes` of every frame of a padded batch: image_sizes = B x (h, w) -> [B][L][2]."""
        return [DeepSolo.valid_shapes(shapes, tuple(hw), strides) for hw in image_sizes]

    def geometry_frames(self, shapes, image_sizes):
        """The tables of a padded batch whose frames have their OWN valid extents (a motion clip made from a still): per-frame
        `lvl_pos`, `enc_ref`, `valid` (one launch, `ops.padded_geometry`), `vshapes` [B,L,2], `vr` [B,L,2] and `vr0` [B,2] on the
        device; `pos_w` is the non-periodic form, a [B*S,384] residual per encoder layer.  A frame that fills the padded size
        takes ratio 1.0 and its full extents through the same kernels.  Never cached: every clip brings new sizes, and
        inference's cache (whose entries captured graphs may point into) is not touched."""
        import numpy as np
        dev, B = self.device, len(image_sizes)
        fv = self.valid_shapes_frames(shapes, image_sizes)
        for vshapes in fv:
            if any(v[0] <= 0 or v[1] <= 0 for v in vshapes):
                raise ValueError("a level has no valid token: image %s too small for the padded batch" % (vshapes,))
        ss = torch.as_tensor(shapes, dtype=torch.long)
        lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        S = int(ss.prod(1).sum())
        ss_d, lsi_d = ss.to(dev), lsi.to(dev)
        vs_d = torch.as_tensor(fv, dtype=torch.long).to(dev)                              # [B, L, 2] (Hv, Wv)
        vr = np.array([[[np.float32(v[1]) / np.float32(s_[1]), np.float32(v[0]) / np.float32(s_[0])]
                        for v, s_ in zip(vshapes, shapes)] for vshapes in fv], np.float32)   # (Wv/W, Hv/H), get_valid_ratio
        vr_d = torch.from_numpy(vr).to(dev)
        lvl_pos, enc_ref, valid = ops.padded_geometry(self.dim_t, self.level_embed, ss_d, lsi_d, vs_d, B, S)
        lvl_pos = lvl_pos.view(B * S, 256)
        return {
            "S": S, "shapes": ss_d, "lsi": lsi_d, "lsi_host": [int(v) for v in lsi],
            "pos_w": [ops.gemm(lvl_pos, L["attn"]["raw"][0]) for L in self.enc], "pos_periodic": False,
            "hw0": tuple(int(v) for hw in shapes[:2] for v in hw),
            "lvl_pos": lvl_pos, "enc_ref": enc_ref.view(B * S, 1, 2), "valid": valid,
            "vshapes": vs_d, "vr": vr_d, "vr0": vr_d[:, 0].contiguous(), "frames": True,
        }

    def geometry(self, shapes, B, vshapes=None):
        """Per-resolution tables.  `vshapes`: valid extents per level for a padded batch (None: nothing is padded)."""
        if vshapes is not None and all(tuple(v) == tuple(s) for v, s in zip(vshapes, shapes)):
            vshapes = None
        key = (tuple(shapes), B, None if vshapes is None else tuple(map(tuple, vshapes)))
        if key in self._geom:
            return self._geom[key]
        dev = self.device
        ss = torch.as_tensor(shapes, dtype=torch.long)
        lsi = torch.cat((ss.new_zeros((1,)), ss.prod(1).cumsum(0)[:-1]))
        S = int(ss.prod(1).sum())
        ss_d, lsi_d = ss.to(dev), lsi.to(dev)
        vs_d = vr_d = None
        if vshapes is not None:
            import numpy as np
            if any(v[0] <= 0 or v[1] <= 0 for v in vshapes):
                raise ValueError("a level has no valid token: image %s too small for the padded batch" % (vshapes,))
            vs_d = torch.as_tensor(vshapes, dtype=torch.long).to(dev)
            vr = np.array([[np.float32(v[1]) / np.float32(s[1]), np.float32(v[0]) / np.float32(s[0])]
                           for v, s in zip(vshapes, shapes)], np.float32)              # (Wv/W, Hv/H), get_valid_ratio
            vr_d = torch.from_numpy(vr).to(dev)
        lvl_pos = torch.empty((S, 256), dtype=_f32, device=dev)
        for l, (H, W) in enumerate(shapes):
            ops.pos_encoding_into(self.dim_t, self.level_embed[l], lvl_pos[int(lsi[l]):], H, W,
                                  None if vshapes is None else vshapes[l])
        # (src + pos) @ W = src @ W + pos @ W, and pos is a per-resolution constant: the position term of every encoder
        # layer's offsets/logits GEMM is a cached residual table instead of a second operand stream
        # (src + pos) W^T = src W^T + (pos W^T): the second term is a [S, 384] table per layer.  The f16x3 kernel reads it
        # periodically (row m -> table row m % S: 57 MB per call instead of a 457 MB broadcast copy at 8 x 37 171 tokens)
        self._pos_periodic = ops.GEMM_MODE == "f16x3" and ops.POS_PERIODIC
        # (the same term as Ty[map row] + Tx[map column] -- the sine embedding puts a function of y alone in channels [0, 128) and of
        # x alone in [128, 256), 1 MB of tables -- removed the projection's surplus traffic and none of its time: the re-reads are
        # Infinity Cache hits; docs/LAB_NOTES.md round 5, profiles/r05_k256_separable_*)
        pos_w = [ops.gemm(lvl_pos, L["attn"]["raw"][0]) for L in self.enc]
        if not self._pos_periodic:
            pos_w = [ops.broadcast_rows(t_, B).view(B * S, 384) for t_ in pos_w]
        geo = {
            "S": S, "shapes": ss_d, "lsi": lsi_d, "lsi_host": [int(v) for v in lsi], "pos_w": pos_w,
            "hw0": tuple(int(v) for hw in shapes[:2] for v in hw),     # (H0, W0[, H1, W1]): the window kernels' tile grids
            "pos_periodic": self._pos_periodic,
            "lvl_pos": ops.broadcast_rows(lvl_pos, B).view(B * S, 256),
            "enc_ref": ops.broadcast_rows(ops.encoder_reference_points(ss_d, lsi_d, S, vs_d), B).view(B * S, 1, 2),
            "valid": ops.proposal_valid(ss_d, lsi_d, S, vs_d),
            "vshapes": vs_d, "vr": vr_d, "vr0": None if vr_d is None else (float(vr[0, 0]), float(vr[0, 1])),
        }
        if not self._geom_transient:        # inference's cache stays as it is: a captured graph may hold pointers into it
            self._geom[key] = geo
        return geo

    def invalid_logit(self):
        """Class logit of a zeroed memory row (what every invalid-proposal token gets in the reference)."""
        if self._invalid_logit is None:
            z = torch.zeros((1, 256), dtype=_f32, device=self.device)
            if self.enc_output_ln is not None:
                self._invalid_logit = ops.proj_ln_dot(z, self.enc_output_ln, self._cls_w, self._cls_b).view(1)
            else:
                om = ops.layernorm(ops.gemm(z, self.enc_output[0], bias=self.enc_output[1]), *self.enc_output_norm)
                self._invalid_logit = ops.gemm(om, self.bezier_class[0], bias=self.bezier_class[1]).view(1)
        return self._invalid_logit

    # --------------------------------------------------------------------------------- pieces
    def input_tokens(self, feats, B, image_hw=None, image_sizes=None):
        """A4 + A5: input_proj (conv + GroupNorm) of the 3 backbone levels + the stride-2 extra level,
        written level by level into the flattened token buffer."""
        shapes = [(f.shape[1], f.shape[2]) for f in feats]
        top = feats[-1]
        if top.shape[3] != self.proj3_cin:               # zero channels up to the padded weight (tiny map: one small copy)
            padded = torch.zeros(top.shape[:3] + (self.proj3_cin,), dtype=_f32, device=self.device)
            padded[..., :top.shape[3]] = top
            top = padded
        x3 = ops.conv2d_nhwc(top, self.proj3[0], shift=self.proj3[1], stride=2, pad=1)
        shapes.append((x3.shape[1], x3.shape[2]))
        if image_sizes is not None:
            geo = self.geometry_frames(shapes, image_sizes)
        else:
            geo = self.geometry(shapes, B, None if image_hw is None else self.valid_shapes(shapes, image_hw))
        S = geo["S"]
        src = torch.empty((B, S, 256), dtype=_f32, device=self.device)
        for l, f in enumerate(feats):
            H, W = shapes[l]
            y = ops.gemm(f.view(B * H * W, f.shape[3]), self.proj[l][0], bias=self.proj[l][1])
            ops.groupnorm32_into(y.view(B, H * W, 256), self.proj[l][2], self.proj[l][3],
                                 src[0, geo["lsi_host"][l]:], S * 256)
        ops.groupnorm32_into(x3.view(B, -1, 256), self.proj3[2], self.proj3[3], src[0, geo["lsi_host"][3]:], S * 256)
        return src.view(B * S, 256), geo

    def encoder(self, src, geo, B):
        S = geo["S"]
        for li, L in enumerate(self.enc):
            rv = ops.linear(src, L["attn"]["raw_value"], R=geo["pos_w"][li], r_cols=384,
                            r_period=S if geo["pos_periodic"] else 0)   # [B*S, 384 | 256]
            frames = geo.get("frames", False)              # a valid extent per frame (`geometry_frames`)
            if frames:
                ops.zero_padded_tokens_frames_(rv, 384, 256, geo["shapes"], geo["lsi"], geo["vshapes"], B, S)
            elif geo["vr"] is not None:                    # padded batch: value.masked_fill(padding_mask, 0)
                ops.zero_padded_tokens_(rv, 384, 256, geo["shapes"], geo["lsi"], geo["vshapes"], B, S)
            # LDS windows for this layer's queries?  Decided once per layer, on its first eager call, from the measured share of octet
            # groups whose samples leave the windows (ops.MSDA_WINDOW_POLICY); undecided calls (a capture in progress) use the windows
            use_win = geo["vr"] is None and L.get("msda_window", True)
            decide = use_win and "msda_window" not in L and ops.MSDA_WINDOW and ops.MSDA_LANES and ops.MSDA_WINDOW_POLICY and \
                not torch.cuda.is_current_stream_capturing()
            if decide and self._msda_counter is None:
                self._msda_counter = torch.zeros((1,), dtype=torch.int32, device=src.device)
            samp = ops.msda_fused(rv, geo["enc_ref"], rv[:, 384:], S * 640, geo["shapes"], geo["lsi"], B, S,
                                  None if frames else geo["vr"], encoder_hw0=geo["hw0"] if use_win else None,
                                  fallback_counter=self._msda_counter if decide else None,
                                  frame_valid_ratios=geo["vr"] if frames else None)
            if decide:
                frac = float(self._msda_counter.item()) / max(1, ops.msda_window_groups(geo["hw0"], B))
                L["msda_window"] = frac <= ops.MSDA_WINDOW_MAX_FALLBACK
                self.msda_window_fallback[li] = frac
            if L["out_ln"] is not None:
                src = ops.proj_ln(samp, L["out_ln"], src)
            else:
                x = ops.gemm(samp, L["attn"]["out"][0], bias=L["attn"]["out"][1], R=src)
                src = ops.layernorm(x, *L["norm1"])
            if L["ffn"] is not None:
                src = ops.ffn_fused_ln(src, L["ffn"])
                continue
            h = ops.gemm(src, L["lin1"][0], bias=L["lin1"][1], relu=True)
            x = ops.gemm(h, L["lin2"][0], bias=L["lin2"][1], R=src)
            src = ops.layernorm(x, *L["norm2"])
        return src

    def proposals(self, memory, geo, B):
        """A8: class logits for every token, top-k, Bezier proposals of the winners -> 25 reference points."""
        S = geo["S"]
        if self.enc_output_ln is not None:
            enc_class = ops.proj_ln_dot(memory, self.enc_output_ln, self._cls_w, self._cls_b).view(-1, 1)   # [B*S, 1]
        else:
            om = ops.layernorm(ops.gemm(memory, self.enc_output[0], bias=self.enc_output[1]), *self.enc_output_norm)
            enc_class = ops.gemm(om, self.bezier_class[0], bias=self.bezier_class[1])          # [B*S, 1]
        frames = geo.get("frames", False)
        topk, rows = ops.topk_tokens(enc_class, B, S, self.nq, invalid_logit=self.invalid_logit(), with_rows=True,
                                     **({"frame_valid": geo["valid"]} if frames else {"valid": geo["valid"]}))
        rows = rows.view(-1)                       # coordinate MLP on the nq winning rows per frame only
        if self.enc_output_ln is not None:
            om_sel = ops.proj_ln(ops.gather_rows(memory, rows), self.enc_output_ln, None)
            h = ops.gemm(om_sel, self.bezier_coord[0][0], bias=self.bezier_coord[0][1], relu=True)
        else:
            h = ops.gemm(om, self.bezier_coord[0][0], bias=self.bezier_coord[0][1], rows=rows, relu=True)
        h = ops.gemm(h, self.bezier_coord[1][0], bias=self.bezier_coord[1][1], relu=True)
        coord_sel = ops.gemm(h, self.bezier_coord[2][0], bias=self.bezier_coord[2][1])          # [B*nq, 8]
        refs = ops.bezier_reference_points(coord_sel, topk, geo["shapes"], geo["lsi"], self.bernstein, B, S, self.nq,
                                           self.P, compact=True, **({"frame_vshapes" if frames else "vshapes": geo["vshapes"]}))
        return refs, topk, enc_class

    def decoder(self, memory, refs, geo, B):
        """A9: six composite decoder layers with iterative reference refinement."""
        nq, P, S = self.nq, self.P, geo["S"]
        Q = B * nq * P
        tgt = ops.broadcast_rows(self.point_embed, B).view(Q, 256)
        vr = geo["vr"]
        # value_proj of the six layers: only the rows each layer's sampling loads (`_dec_value_rows`), or every row in one launch
        sparse = self._dec_value_state(geo, B, memory.device)
        decide = sparse is not None and self.dec_value_dense is None and ops.DEC_VALUE_POLICY and \
            not torch.cuda.is_current_stream_capturing()
        if sparse is not None:
            values = _SparseValues(sparse, memory, decide)
        else:
            values = ops.linear(memory, self.dec_value)                                       # [B*S, 1536]
        if vr is not None:
            zero = ops.zero_padded_tokens_frames_ if geo.get("frames", False) else ops.zero_padded_tokens_
            zero(values, 0, values.shape[1], geo["shapes"], geo["lsi"], geo["vshapes"], B, S)
        refs = refs.view(Q, 2)
        inter_refs = []
        E = 256
        emb = None                   # the layer's point embedding, when the previous layer's refinement launch already made it
        qpos = None                  # ... or the layer's query position itself (the previous layer's tail launch)
        for lid, L in enumerate(self.dec):
            refs, tgt, emb, qpos = self._decoder_layer(lid, L, tgt, refs, values, geo, B, vr, emb, lid + 1 < len(self.dec), qpos)
            inter_refs.append(refs)
        if decide:                   # one layer above the threshold keeps the dense launch, and the launch then serves all six
            self.dec_value_dense = max(self.dec_value_share.values()) > ops.DEC_VALUE_MAX_SHARE
        return tgt, inter_refs

    def _dec_value_state(self, geo, B, device):
        """The sparse value projection's device state for this resolution (ops.DecValueRows, cached: one zero-filled [B*S, 256] buffer
        that all six layers reuse -- layer l's rows are consumed before layer l + 1's are written on the same stream), or None when
        the step runs the dense launch: switched off, another GEMM back-end, a padded batch (its masked value rows are zeroed in the
        dense buffer), or a measured share above ops.DEC_VALUE_MAX_SHARE."""
        if not ops.DEC_VALUE_SPARSE or geo["vr"] is not None or self.dec_value_dense or self.dec_value_layers is None:
            return None
        key = (B, geo["S"], str(device))
        if key not in self._dec_value_states:
            self._dec_value_states[key] = ops.DecValueRows(B * geo["S"], device)
        return self._dec_value_states[key]

    def _dec_value_rows(self, lid, sv, raw, ref, geo, B, Lq):
        """Layer `lid`'s value rows: mark what the gather kernel will load for these offsets | logits, compact, project the listed rows
        (the GEMM clears their marks).  Nothing on the host, unless this call measures the layer's share."""
        st = sv.state
        ops.dec_value_mark(raw, ref, geo["shapes"], geo["lsi"], B, Lq, geo["S"], st)
        ops.dec_value_compact(st)
        if sv.measure:
            self.dec_value_share[lid] = float(st.count.item()) / st.n
        return ops.linear_rows(sv.memory, self.dec_value_layers[lid], st)

    def _decoder_layer(self, lid, L, tgt, refs, values, geo, B, vr, emb=None, more=False, qpos=None):
        nq, P, E = self.nq, self.P, 256
        Q = B * nq * P
        with ops.profile_scope("decoder_layer"):                 # bench.py: the launches that perform a layer's Q-side products
            # reference_points_input = reference_points * valid_ratios; the query position comes from level 0's (:470-473)
            if qpos is None:
                if emb is None:
                    if vr is None:
                        qref = refs
                    elif geo.get("frames", False):
                        qref = ops.scale_xy_frames_(refs.clone(), geo["vr0"])
                    else:
                        qref = ops.scale_xy_(refs.clone(), *geo["vr0"])
                    emb = ops.point_pos_embed(qref, self.dim_t)
                qpos = emb
                if self.ref_point_mlp2 is not None:
                    qpos = ops.mlp2_fused(qpos, self.ref_point_mlp2)
                else:
                    qpos = ops.linear(qpos, self.ref_point_head[0], relu=True)
                    qpos = ops.linear(qpos, self.ref_point_head[1])
            # intra-instance attention over the 25 points of each query (deformable_transformer.py:386-394)
            attn = None
            if L["intra_block"] is not None and P <= 32:
                tgt = ops.dec_attn(tgt, L["intra_block"], B * nq, P, pos=qpos)
            else:
                qk = ops.linear(tgt, L["intra_qk"], A2=qpos)                                   # [Q, 512]
                v = ops.linear(tgt, L["intra_v"])
                attn = torch.empty((Q, E), dtype=_f32, device=self.device)
                qkf = qk.view(-1)
                ops.mha_core(qkf, qkf[E:], v, attn, B * nq, 1, 8, 32, P, P,
                             [P * 2 * E, 0, 2 * E, P * 2 * E, 0, 2 * E, P * E, 0, E, P * E, 0, E])
                tgt = self._out_norm(attn, L, "intra", tgt)
            # inter-instance attention over the nq queries, batched over (frame, point) (:396-404)
            raw = None
            if L["inter_block"] is not None and nq <= ops.DEC_INTER_MAX_FUSED:
                if L["inter_block"].has_raw and vr is None:
                    tgt, raw = ops.dec_attn(tgt, L["inter_block"], B * P, nq, inner=P, raw_pos=qpos)
                else:
                    tgt = ops.dec_attn(tgt, L["inter_block"], B * P, nq, inner=P)
            elif L["inter_block"] is not None and L["inter_out_ln"] is not None:
                tgt = ops.proj_ln(ops.dec_inter_heads(tgt, L["inter_block"], B * P, nq, inner=P), L["inter_out_ln"], tgt)
            else:
                qkv = ops.linear(tgt, L["inter_in"])                                           # [Q, 768]
                if attn is None:
                    attn = torch.empty((Q, E), dtype=_f32, device=self.device)
                f = qkv.view(-1)
                ld = 3 * E
                ops.mha_core(f, f[E:], f[2 * E:], attn, B, P, 8, 32, nq, nq,
                             [nq * P * ld, ld, P * ld] * 3 + [nq * P * E, E, P * E])
                tgt = self._out_norm(attn, L, "inter", tgt)
            # deformable cross attention into the encoder memory (:406-422)
            if isinstance(values, _SparseValues):
                if raw is None:      # (the inter block's launch did not make the offsets | logits: the unfused path)
                    raw = ops.linear(tgt, L["cross"]["raw"], A2=qpos)
                value, ld_value = self._dec_value_rows(lid, values, raw, refs, geo, B, nq * P), E
            else:
                value, ld_value = values[:, lid * E:(lid + 1) * E], values.stride(0)
            samp = self._msda_strided(L["cross"], tgt, qpos, refs.view(Q, 1, 2), value, ld_value, geo, B, nq * P, vr, raw=raw)
            tail = L.get("tail") if vr is None else None
            if tail is not None and tail.proj is not None:
                # out_proj + norm_cross, FFN + norm3, the coordinate MLP + reference refinement (:484-488) and the next layer's query
                # position: one launch from the sampled rows
                tgt, refs, nqpos = ops.dec_tail(samp, tail, refs, want_qpos=more, residual=tgt, frames=B)
                return refs, tgt, None, nqpos
            tgt = self._out_norm(samp, L, "cross", tgt)
            if tail is not None:
                tgt, refs, nqpos = ops.dec_tail(tgt, tail, refs, want_qpos=more, frames=B)
                return refs, tgt, None, nqpos
            if L["ffn"] is not None:
                tgt = ops.ffn_fused_ln(tgt, L["ffn"])
            else:
                h = ops.gemm(tgt, L["lin1"][0], bias=L["lin1"][1], relu=True)
                x = ops.gemm(h, L["lin2"][0], bias=L["lin2"][1], R=tgt)
                tgt = ops.layernorm(x, *L["norm3"])
            # reference refinement (:484-488); with the MLP's hidden layers fused, its N = 2 layer, the sigmoid update and the NEXT
            # layer's point embedding (:470-473) are one launch
            if ops.REF_UPDATE and self.ctrl_coord_mlp2 is not None:
                scale = {} if vr is None else {"frame_scales" if geo.get("frames", False) else "scale": geo["vr0"]}
                refs, emb = ops.ref_update(ops.mlp2_fused(tgt, self.ctrl_coord_mlp2), self.ctrl_coord[2], refs, self.dim_t,
                                           want_pos=more, **scale)
            else:
                d = self._mlp3(tgt, self.ctrl_coord)
                refs, emb = ops.ref_sigmoid(d, refs, 2), None
        return refs, tgt, emb, None

    @staticmethod
    def _out_norm(x, L, name, tgt):
        """norm_<name>(tgt + out_proj(x)) of a decoder attention block: one launch under the f16x3 back-end."""
        blk = L[name + "_out_ln"]
        if blk is not None:
            return ops.proj_ln(x, blk, tgt)
        out = L["cross"]["out"] if name == "cross" else L[name + "_out"]
        return ops.layernorm(ops.linear(x, out, R=tgt), *L["norm_" + name])

    def _msda_strided(self, W, query, query_pos, ref, value_view, ld_value, geo, B, Lq, vr=None, raw=None):
        """Cross-attention sampling straight out of the fused [B*S, 1536] value buffer (no compaction copy); `raw` = the offsets |
        logits when the inter block's launch already made them."""
        if raw is None:
            raw = ops.linear(query, W["raw"], A2=query_pos)
        if geo.get("frames", False):
            return ops.msda_fused(raw, ref, value_view, geo["S"] * ld_value, geo["shapes"], geo["lsi"], B, Lq, frame_valid_ratios=vr)
        return ops.msda_fused(raw, ref, value_view, geo["S"] * ld_value, geo["shapes"], geo["lsi"], B, Lq, vr)

    def _mlp3(self, x, layers):
        blk = self.ctrl_coord_mlp2 if layers is self.ctrl_coord else self.boundary_mlp2 if layers is self.boundary else None
        if blk is not None:
            return ops.linear(ops.mlp2_fused(x, blk), layers[2])
        h = ops.linear(x, layers[0], relu=True)
        h = ops.linear(h, layers[1], relu=True)
        return ops.linear(h, layers[2])

    def heads(self, hs, inter_refs):
        """A10: last-layer heads with inter_references[last-1] (detection_transformer_wobackbone.py:209-253)."""
        ref = inter_refs[self.n_dec - 2]
        cls = ops.gemm(hs, self.ctrl_class[0], bias=self.ctrl_class[1])                       # [Q,1]
        text = ops.gemm(hs, self.ctrl_text[0], bias=self.ctrl_text[1])                        # [Q,voc+1]
        # pred_ctrl_points IS the last layer's refined reference: the same (shared, detection_transformer_wobackbone.py:141-155)
        # MLP on the same hs plus the same inverse_sigmoid(reference), through the same sigmoid (deformable_transformer.py:484-488)
        # -- for DEC_LAYERS >= 2.  With a single layer the reference's base is inter_references[-1], the already refined points
        # (index last_lvl - 1 = -1), so the head output is one more application of the MLP on top of them.
        ctrl = inter_refs[self.n_dec - 1] if self.n_dec >= 2 else ops.ref_sigmoid(self._mlp3(hs, self.ctrl_coord), ref, 2)
        bd = ops.ref_sigmoid(self._mlp3(hs, self.boundary), ref, 4)
        return {"pred_logits": cls, "pred_text_logits": text, "pred_ctrl_points": ctrl, "pred_bd_points": bd,
                "query_features": hs}

    # --------------------------------------------------------------------------------- whole forward
    def forward(self, feats, taps=None, image_hw=None, image_sizes=None):
        """feats: [res3, res4, res5] NHWC tensors of one batch of same-size frames.  Returns the reference's
        output dict with tensors flattened over (B, nq, P): pred_logits [B*nq*P,1], pred_text_logits [.,voc+1],
        pred_ctrl_points [.,2], pred_bd_points [.,4], query_features [.,256].
        image_hw: the (h, w) all frames of a padded batch share; image_sizes: B x (h, w), every frame its own (exclusive)."""
        B = feats[0].shape[0]
        if image_sizes is not None:
            if image_hw is not None:
                raise ValueError("image_hw and image_sizes are exclusive")
            image_sizes = [tuple(int(v) for v in hw) for hw in image_sizes]
            if len(image_sizes) != B:
                raise ValueError("image_sizes has %d entries for a batch of %d frames" % (len(image_sizes), B))
        src, geo = self.input_tokens(feats, B, image_hw, image_sizes)
        memory = self.encoder(src, geo, B)
        refs, topk, enc_class = self.proposals(memory, geo, B)
        hs, inter_refs = self.decoder(memory, refs, geo, B)
        out = self.heads(hs, inter_refs)
        if taps is not None:
            taps.update(src=src, memory=memory, topk=topk, enc_class=enc_class, init_ref=refs, geo=geo)
        return out
