"""Tensor-level wrappers over the C ABI (torch = device memory + stream plumbing only).

Every function launches hand-written HIP kernels from libgomatching_hip.so on torch's current stream;
none has a CPU or torch-op fallback.
"""
import collections
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import lib as _lib_mod
from .lib import check

_f32 = torch.float32


def _L():
    return _lib_mod.load()


def _call(name, *args):
    """Call the status-returning entry point `name`; a non-zero status raises GomError("<name> failed: ...")."""
    rc = getattr(_lib_mod._lib or _L(), name)(*args)         # (the loaded handle read directly: host time per launch matters)
    if rc:
        check(rc, name)


# Optional launch profiler for bench.py's roofline leg: a list that receives one (start_event, end_event, flops, bytes, label,
# scope) per launch of every instrumented kernel (`_timed`); bench.py picks kernels by label prefix and the decoder layers by
# scope (`profile_scope`).  None = no events recorded.
_gemm_profile = None


_profile_scope = ""


@contextlib.contextmanager
def profile_scope(name):
    """Every profile record made inside the block carries `name` as its last element (bench.py: which launches belong to the
    decoder layers)."""
    global _profile_scope
    old, _profile_scope = _profile_scope, name
    try:
        yield
    finally:
        _profile_scope = old


def set_gemm_profile(collector):
    global _gemm_profile
    _gemm_profile = collector


class _Timed:
    """HIP events around the launch(es) of a `with` block; the record is appended when the block ends without an error."""

    def __init__(self, prof, figures):
        self.prof, self.figures = prof, figures

    def __enter__(self):
        self.e0 = torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def __exit__(self, etype, exc, tb):
        if etype is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.prof.append((self.e0, e1) + self.figures() + (_profile_scope,))


_untimed = contextlib.nullcontext()


def _timed(cond, figures):
    """Launch bracket of the profiler: `with _timed(cond, lambda: (flops, bytes, label)): _call(launch)`.  Without a collector or
    with `cond` false it is one shared no-op: no event is created and `figures` is never called."""
    return _Timed(_gemm_profile, figures) if (_gemm_profile is not None and cond) else _untimed


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _ld(t, width=None):
    """Leading dimension of a 2-D row-strided tensor as the kernels take it: stride(0), except that a tensor of one row (or none)
    passes its width -- there stride(0) is whatever the view it was cut from had.  None passes 0.  `width`: the row length of a
    tensor that has no shape[1] of its own (a 1-D vector passed as one row).  The rule looks at the tensor, not at the launch: a
    one-row launch into a taller buffer passes that buffer's real stride, which serves a single row as well as the width does."""
    if t is None:
        return 0
    shape = t.shape                                          # (one .shape and one .stride() cost what a single .stride(0) does)
    if len(shape) > 1 and shape[0] > 1:
        return t.stride()[0]
    return shape[-1] if width is None else width


def _stream():
    # raw hipStream_t of torch's current stream; the private accessor costs ~0.3 us against ~8 us for
    # torch.cuda.current_stream().cuda_stream, which matters on the launch-bound tracker path
    return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or \
    (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if t.dtype != _f32 or not t.is_cuda or not t.is_contiguous():
            raise _lib_mod.GomError("expected a contiguous float32 CUDA tensor, got %s %s contiguous=%s" % (
                t.dtype, t.device, t.is_contiguous()))


def _chk_frame_desc(t, B, tail, dtype, name):
    """A per-frame descriptor of a padded batch (`padded_geometry` and the `frame_*` keywords): [B, *tail], contiguous, on the GPU."""
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.dim() != 1 + len(tail) or t.shape[0] != B or \
            tuple(t.shape[1:]) != tuple(tail):
        raise _lib_mod.GomError("%s: expected a contiguous %s CUDA tensor of shape %s (one entry per frame of the batch), got %s %s" % (
            name, dtype, (B,) + tuple(tail), t.dtype, tuple(t.shape)))


# ------------------------------------------------------------------------------------------ GEMM
# "bf16x6": weights of the big contractions are pre-split into three bf16 planes and multiplied on the bf16
# matrix cores with fp32-level accuracy (csrc/gemm_bf16x6.hip); "fp32": exact-fp32 MFMA everywhere.
GEMM_MODE = "f16x3"


class SplitWeight:
    """Pre-split planes of an fp32 weight [N, K] (row slices keep the plane stride): kind "bf16x6" = [3, N, Kpad] bf16,
    kind "f16x3" = [2, N, Kpad] fp16 of the power-of-two-scaled rows + `inv_scale` [N] fp32."""

    def __init__(self, planes, N, K, conv_shape=None, kind="bf16x6", inv_scale=None):
        self.planes, self.N, self.K, self.conv_shape, self.kind, self.inv_scale = planes, N, K, conv_shape, kind, inv_scale

    @property
    def shape(self):
        return (self.N, self.K)

    def __getitem__(self, sl):
        assert isinstance(sl, slice) and sl.step in (None, 1)
        a, b, _ = sl.indices(self.N)
        return SplitWeight(self.planes[:, a:b], b - a, self.K, kind=self.kind,
                           inv_scale=None if self.inv_scale is None else self.inv_scale[a:b])


def split_weight(w, conv_shape=None, kind=None):
    """w: fp32 [N, K] on the GPU (rows may be strided: a column slice of a wider buffer, as the K / V operands of an
    attention product are) -> SplitWeight of the current GEMM_MODE's kind."""
    assert w.dim() == 2 and w.stride(1) == 1 and w.dtype == _f32 and w.is_cuda
    kind = kind or (GEMM_MODE if GEMM_MODE in ("bf16x6", "f16x3") else "bf16x6")
    N, K = w.shape
    ldw = _ld(w)
    Kpad = (K + 31) // 32 * 32
    if kind == "f16x3":
        planes = torch.empty((2, N, Kpad), dtype=torch.float16, device=w.device)
        inv = torch.empty((N,), dtype=_f32, device=w.device)
        _call("gom_split_f16x2", _p(w), ldw, N, K, _p(planes), Kpad, _p(inv), _stream())
        return SplitWeight(planes, N, K, conv_shape, "f16x3", inv)
    planes = torch.empty((3, N, Kpad), dtype=torch.bfloat16, device=w.device)
    _call("gom_split_bf16x3", _p(w), ldw, N, K, _p(planes), Kpad, _stream())
    return SplitWeight(planes, N, K, conv_shape)


_range_flags = {}


def _switch(name, default=True):
    """Build-time switches of the f16x3 path; the environment (GOM_<NAME>=0/1) overrides the default for same-box A/B runs."""
    import os
    v = os.environ.get("GOM_" + name)
    return default if v is None else v not in ("0", "false", "False", "")


_lib_forms = {}


def _lib_form(setter, on):
    """A library-side kernel-form switch follows its ops.<NAME> value (set again only when that changed)."""
    on = bool(on)
    if _lib_forms.get(setter) is not on:
        getattr(_L(), setter)(1 if on else 0)
        _lib_forms[setter] = on


# Small launches of the detector pass in their lean forms (same results bit for bit; off = the forms before them, for A/B runs):
TOPK_LEAN = _switch("TOPK_LEAN")                 # proposal top-k: k-bounded chunk sort, merge network sized by the candidates
DEC_VALUE_MARK_LEAN = _switch("DEC_VALUE_MARK_LEAN")   # decoder row marking: a flag is read before it is stored
GEMM_NARROW_TILE = _switch("GEMM_NARROW_TILE")   # exact-fp32 GEMM, N <= 32: 128-row tiles while 256-row tiles would leave most CUs empty


def _dev_index(device):
    d = torch.device(device)
    return d.index if d.index is not None else torch.cuda.current_device()


def range_flag(device):
    """Device word the f16x3 kernels set when a result is not finite (an activation beyond fp16's range)."""
    key = _dev_index(device)
    if key not in _range_flags:
        _range_flags[key] = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", key))
    return _range_flags[key]


def check_range_flag(device):
    """Host check at a sync point: raises instead of letting an out-of-range activation pass as a result."""
    key = _dev_index(device)
    words = [f for f in [_range_flags.get(key)] if f is not None]
    up = [f for f in words if int(f.item()) != 0]
    if up:
        for f in up:
            f.zero_()
        raise _lib_mod.GomError("f16x3 GEMM produced a non-finite value: an activation left fp16's range (|x| > 65504) "
                                "or the input was not finite; run with ops.GEMM_MODE = 'bf16x6'")


@contextlib.contextmanager
def gemm_mode(mode):
    """Run a block (model construction and / or a forward pass) under another contraction back-end; the model's precision
    fallback builds and runs its bf16x6 twin of the detector this way (GoMatching._fallback_detect)."""
    global GEMM_MODE
    old, GEMM_MODE = GEMM_MODE, mode
    try:
        yield
    finally:
        GEMM_MODE = old


# Frames of the detector step the model plans (GoMatching.frames_per_step), or None.  Kernel choices that depend on a launch's row
# count (`conv_plan`, `tail_form2_wins`) decide by the planned step's rows instead of the call's, so a frame's bits do not depend on
# how many frames share its step: a clip's short last step and every per-size step of a mixed-resolution clip make the choices of a
# full step.  None (direct op calls): each call decides by its own rows.
STEP_FRAMES = None


@contextlib.contextmanager
def step_plan(frames):
    """Run a block (one detector step, GoMatching._detect_core) under a step plan of `frames` frames."""
    global STEP_FRAMES
    assert frames is None or int(frames) > 0
    old, STEP_FRAMES = STEP_FRAMES, (None if frames is None else int(frames))
    try:
        yield
    finally:
        STEP_FRAMES = old


def plan_rows(frames, rows_per_frame):
    """The row count a row-count-dependent dispatch decides by: the planned step's when a plan is set (also for a step with more
    frames than planned), else the call's own `frames` x `rows_per_frame`."""
    return (STEP_FRAMES or frames) * rows_per_frame


def flag_nonfinite(x, flag):
    """flag |= 1 on the device when x holds an Inf / NaN (result check of the back-ends whose GEMMs carry no range flag)."""
    _chk_f32(x)
    _call("gom_flag_nonfinite_f32", _p(x), x.numel(), _p(flag), _stream())


def prep_weight(w, min_n=33):
    """Weight preparation policy for the detector's nn.Linear weights."""
    if GEMM_MODE in ("bf16x6", "f16x3") and w.shape[0] >= min_n:
        return split_weight(w.contiguous())
    return w


def prep_conv_weight(w_ohwi):
    if GEMM_MODE in ("bf16x6", "f16x3") and w_ohwi.shape[0] >= 33:
        Cout = w_ohwi.shape[0]
        return split_weight(w_ohwi.reshape(Cout, -1).contiguous(), conv_shape=tuple(w_ohwi.shape))
    return w_ohwi


def _gemm_split(A, W, bias, scale, A2, rows, R, relu, out, M, r_cols=None, r_period=0):
    if A2 is not None:                                       # the bf16x6 kernel has one A operand: add first
        assert rows is None
        A = add(A.contiguous(), A2.contiguous())
    K, N = A.shape[1], W.N
    assert W.K == K
    if out is None:
        out = torch.empty((M, N), dtype=_f32, device=A.device)
    lda, ldc, ldr = _ld(A), _ld(out), _ld(R)
    pl = W.planes
    rc = (r_cols if r_cols is not None else N) if R is not None else 0
    if W.kind != "f16x3":
        assert not r_period, "a periodic residual is served by the f16x3 kernel only"
        assert relu in (False, True, 0, 1), "only the f16x3 kernel has a GELU epilogue (use gemm_gelu)"
    with _timed(M > 0, lambda: (2.0 * M * N * K, 4.0 * M * K + 2.0 * pl.shape[0] * N * pl.shape[2] + 4.0 * M * N
                                + (4.0 * (r_period or M) * rc if R is not None else 0.0), "%dx%dx%d" % (M, N, K))):
        if W.kind == "f16x3":
            _call("gom_gemm_f32_f16x3_rp", _p(A), _p(rows), lda, _p(pl), pl.stride(0), pl.stride(1), _p(W.inv_scale), _p(scale),
                  _p(bias), _p(R), ldr, rc, int(r_period), 2 if relu == "gelu" else (1 if relu else 0), _p(out), ldc, M, N, K,
                  _p(range_flag(A.device)), _stream())
        else:
            _call("gom_gemm_f32_bf16x6", _p(A), _p(rows), lda, _p(pl), pl.stride(0), pl.stride(1), _p(scale), _p(bias), _p(R), ldr,
                  rc, 1 if relu else 0, _p(out), ldc, M, N, K, _stream())
    return out


SPLITK_MAX_ROWS = 1024
SMALL_GEMM_OUTPUTS = 1 << 16         # M*N up to which gemm(..., small=True) runs the patch-per-wave VALU kernel (tracker logits)
SMALL_GEMM_ROWS = 64                 # ... and any N up to this many rows (csrc/matcher_rt.cpp `linear` applies the same rule)


def gemm(A, W, bias=None, scale=None, A2=None, rows=None, R=None, relu=False, out=None, M=None, splitk=None,
         r_cols=None, small=False, r_period=0):
    """C = act((A[+A2])[M,K] @ W[N,K]^T * scale + bias + R).  A may be a 2-D row-strided view
    (stride(1) == 1); W likewise (row slices of a weight matrix)."""
    if isinstance(W, SplitWeight):
        assert A.dim() == 2 and A.stride(1) == 1
        if M is None:
            M = A.shape[0] if rows is None else rows.numel()
        if A2 is not None:
            assert A2.shape == A.shape and A2.stride() == A.stride()
        return _gemm_split(A, W, bias, scale, A2, rows, R, relu, out, M, r_cols, r_period)
    assert not r_period, "a periodic residual (r_period) is served by the f16x3 split-weight kernel only"
    assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1
    if R is not None and r_cols is not None and r_cols < W.shape[0]:
        # exact-fp32 kernel has no column-limited residual: run the two column blocks as two launches
        Mrows = A.shape[0] if rows is None else rows.numel()
        if out is None:
            out = torch.empty((Mrows, W.shape[0]), dtype=_f32, device=A.device)
        gemm(A, W[:r_cols], bias=None if bias is None else bias[:r_cols], scale=scale, A2=A2, rows=rows, R=R,
             relu=relu, out=out[:, :r_cols], M=M)
        gemm(A, W[r_cols:], bias=None if bias is None else bias[r_cols:], scale=scale, A2=A2, rows=rows, relu=relu,
             out=out[:, r_cols:], M=M)
        return out
    K = A.shape[1]
    assert W.shape[1] == K
    N = W.shape[0]
    if M is None:
        M = A.shape[0] if rows is None else rows.numel()
    lda, ldw = _ld(A), _ld(W)
    if A2 is not None:
        assert A2.shape == A.shape and A2.stride() == A.stride()
    if out is None:
        out = torch.empty((M, N), dtype=_f32, device=A.device)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] == N
    if R is not None:
        assert R.dim() == 2 and R.stride(1) == 1 and R.shape[1] == N
    ldc, ldr = _ld(out), _ld(R)
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.is_contiguous()
    if M == 0:
        return out                                           # no row, no launch: an empty tensor has no address for the entry's null checks
    # `small` marks the tracker's latency-bound products (kernel choice must never depend on how many frames share a
    # step, so this is an explicit request): up to SMALL_GEMM_OUTPUTS outputs one wave owns a column for 8 rows on the
    # VALU (7-20 us); larger ones take the deterministic split-K (20-50 us) instead of looping the whole K in few
    # workgroups (85-95 us whatever M is; tools/skinny_bench.py)
    if small and A2 is None and M > 0:
        if (M <= SMALL_GEMM_ROWS or M * N <= SMALL_GEMM_OUTPUTS) and K % 4 == 0 and lda % 4 == 0 and ldw % 4 == 0:
            _call("gom_gemm_small_f32", _p(A), _p(rows), lda, _p(W), ldw, _p(scale), _p(bias), _p(R), ldr, 1 if relu else 0,
                  _p(out), ldc, M, N, K, _stream())
            return out
        splitk = M <= SPLITK_MAX_ROWS                        # beyond that the partial sums cost more than they save
    if splitk is None:
        splitk = 0 < M <= 128 and N * K >= (1 << 18) and K >= 256      # skinny, weight-read bound
    if splitk and A2 is None and M > 0:
        nbytes = _L().gom_gemm_splitk_workspace_bytes(M, N, K)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=A.device)
        _call("gom_gemm_f32_splitk", _p(A), _p(rows), lda, _p(W), ldw, _p(scale), _p(bias), _p(R), ldr, 1 if relu else 0, _p(out),
              ldc, M, N, K, _p(ws), nbytes, _stream())
        return out
    with _timed(N > 64 and M > 0 and GEMM_MODE == "fp32", lambda: (
            2.0 * M * N * K, 4.0 * (M * K + N * K + M * N + (M * N if R is not None else 0)), "%dx%dx%d" % (M, N, K))):
        _lib_form("gom_gemm_f32_set_narrow_tile", GEMM_NARROW_TILE)
        _call("gom_gemm_f32", _p(A), _p(A2), _p(rows), lda, _p(W), ldw, _p(scale), _p(bias), _p(R), ldr, 1 if relu else 0, _p(out),
              ldc, M, N, K, _stream())
    return out


# f16x3 back-end: pointwise convolutions with 256 input channels (res4 conv3) on the row-resident K = 256 kernel.  MEASURED in the
# step (bench.py, one box): 157 us per launch against the tile kernel's 150 -- the shortcut's residual reads and 16-byte stores
# cost what the missing A staging saves at 441 one-per-CU tiles.  OFF; GOM_PW_K256=1 for A/B runs.
PW_K256 = _switch("PW_K256", default=False)
PW_K256_MIN_ROWS = 16384
CONV3_PATCH = _switch("CONV3_PATCH")   # f16x3 back-end: 3x3 / stride 1 convolutions on the patch-resident kernel


def conv_plan(rows, Cout, Cin, KH, KW, stride, pad, kind, residual=False):
    """(kernel, splits) of a convolution with `rows` output pixels (B x OH x OW, or `plan_rows`) on back-end `kind` ("f16x3", "bf16x6"
    or "fp32" = an unsplit weight).  kernel: "patch" (csrc/conv3x3_patch.hip), "pw_k256" (csrc/gemm_k256.hip), "tile" (the split-weight
    implicit GEMM of csrc/gemm_f16x3.hip / gemm_bf16x6.hip, K sliced `splits` ways when splits > 1) or "fp32" (csrc/gemm_conv.hip).
    The split count sets the K partition and so the fp32 summation order: it must come from the same rows for every step size."""
    if kind == "fp32":
        return "fp32", 0
    splits = _L().gom_conv_bf16x6_splits(rows, Cout, KH * KW * Cin)    # few tiles x long K (input_proj[3]): slice K
    if (kind == "f16x3" and CONV3_PATCH and KH == 3 and KW == 3 and stride == 1 and pad == 1 and not residual and splits <= 1
            and _L().gom_conv3x3_patch_supported(Cin, Cout)):
        return "patch", 0
    if (kind == "f16x3" and PW_K256 and KH == 1 and KW == 1 and stride == 1 and pad == 0 and Cin == 256 and Cout % 32 == 0
            and Cout >= 512 and rows >= PW_K256_MIN_ROWS and splits <= 1):
        return "pw_k256", 0
    return "tile", splits


def conv2d_nhwc(x, w_ohwi, scale=None, shift=None, R=None, relu=False, stride=1, pad=0):
    """x [B,H,W,Cin] -> [B,OH,OW,Cout]; w [Cout,KH,KW,Cin] fp32, or a SplitWeight made by prep_conv_weight."""
    split = isinstance(w_ohwi, SplitWeight)
    _chk_f32(x, None if split else w_ohwi, scale, shift, R)
    B, H, Wd, Cin = x.shape
    Cout, KH, KW, Cin2 = w_ohwi.conv_shape if split else w_ohwi.shape
    assert Cin == Cin2
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (Wd + 2 * pad - KW) // stride + 1
    y = torch.empty((B, OH, OW, Cout), dtype=_f32, device=x.device)
    if R is not None:
        assert R.shape == y.shape
    if split:
        pl = w_ohwi.planes
        M = B * OH * OW
        kernel, splits = conv_plan(plan_rows(B, OH * OW), Cout, Cin, KH, KW, stride, pad, w_ohwi.kind, residual=R is not None)
        ws, nbytes = None, 0
        if splits > 1:
            nbytes = 4 * splits * M * Cout
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
        if kernel == "patch":
            # the bottlenecks' 3x3 / 1 convolutions: input patch resident in LDS (csrc/conv3x3_patch.hip)
            img = getattr(w_ohwi, "patch_image", None)
            if img is None:                                  # fragment-linear image of the planes, built once per weight
                nb = _L().gom_conv3x3_patch_image_bytes(Cin, Cout)
                img = torch.empty((nb,), dtype=torch.uint8, device=pl.device)
                _call("gom_conv3x3_patch_image", _p(pl), pl.stride(0), pl.stride(1), Cin, Cout, _p(img), nb, _stream())
                w_ohwi.patch_image = img
            with _timed(True, lambda: (2.0 * M * Cout * 9 * Cin, 4.0 * M * (Cin + Cout) + 4.0 * 9 * Cin * Cout,
                                       "conv3:%dx%dx%d" % (M, Cout, 9 * Cin))):
                _call("gom_conv3x3_patch_f32_f16x3", _p(x), _p(img), _p(w_ohwi.inv_scale), _p(scale), _p(shift), 1 if relu else 0,
                      _p(y), B, H, Wd, Cin, Cout, _p(range_flag(x.device)), _stream())
            return y
        if kernel == "pw_k256":
            # conv3 of the res4 bottlenecks (256 -> 1024, + BN + shortcut + ReLU): K = 256 is the row-resident kernel's shape
            # (csrc/gemm_k256.hip: rows as fragments once, weights by LDS-DMA, no A staging) -- FrozenBN's scale folds into the
            # image's inverse row scale, its shift is the bias
            key = (id(scale), id(shift))
            cache = w_ohwi.__dict__.setdefault("k256_images", {})
            img = cache.get(key)
            if img is None:
                inv = w_ohwi.inv_scale if scale is None else (w_ohwi.inv_scale * scale).contiguous()
                nb = _L().gom_gemm_k256_image_bytes(Cout, Cin)
                img = torch.empty((nb,), dtype=torch.uint8, device=pl.device)
                _call("gom_gemm_k256_image", _p(pl), pl.stride(0), pl.stride(1), _p(inv), _p(shift), Cout, Cin, _p(img), nb,
                      _stream())
                cache[key] = img = (img, inv, scale, shift)         # (the vectors stay referenced: ids are the cache key)
            with _timed(True, lambda: (2.0 * M * Cout * Cin, 4.0 * M * Cin + 4.0 * M * Cout * (2 if R is not None else 1) + 4.0 * Cout * Cin,
                                       "pwk256:%dx%dx%d" % (M, Cout, Cin))):
                _call("gom_gemm_k256_rp_f32", _p(x), None, Cin, _p(img[0]), _p(R), Cout if R is not None else 0,
                      Cout if R is not None else 0, 0, 1 if relu else 0, _p(y), Cout, M, Cout, Cin, 1, _p(range_flag(x.device)),
                      _stream())
            return y
        if w_ohwi.kind == "f16x3":
            # a pointwise convolution IS a launch of the GEMM tile kernel (dispatch<0, 0> in csrc/gemm_f16x3.hip): bench.py's
            # roofline sample of that kernel covers these launches too (label "pw:")
            with _timed(KH == 1 and stride == 1 and pad == 0 and splits <= 1 and Cout > 64, lambda: (
                    2.0 * M * Cout * Cin, 4.0 * M * Cin + 4.0 * M * Cout * (2 if R is not None else 1) + 4.0 * Cout * Cin, "pw:%dx%dx%d" % (M, Cout, Cin))):
                _call("gom_conv2d_nhwc_f32_f16x3", _p(x), _p(pl), pl.stride(0), pl.stride(1), _p(w_ohwi.inv_scale), _p(scale),
                      _p(shift), _p(R), 1 if relu else 0, _p(y), B, H, Wd, Cin, Cout, KH, KW, stride, pad, _p(ws), nbytes, splits,
                      _p(range_flag(x.device)), _stream())
            return y
        _call("gom_conv2d_nhwc_f32_bf16x6_splitk", _p(x), _p(pl), pl.stride(0), pl.stride(1), _p(scale), _p(shift), _p(R),
              1 if relu else 0, _p(y), B, H, Wd, Cin, Cout, KH, KW, stride, pad, _p(ws), nbytes, splits, _stream())
        return y
    _lib_form("gom_gemm_f32_set_narrow_tile", GEMM_NARROW_TILE)
    _call("gom_conv2d_nhwc_f32", _p(x), _p(w_ohwi), _p(scale), _p(shift), _p(R), 1 if relu else 0, _p(y), B, H, Wd, Cin, Cout, KH,
          KW, stride, pad, _stream())
    return y


# ------------------------------------------------------------------------------------------ norms
def layernorm(x, gamma, beta, residual=None, eps=1e-5, out=None):
    _chk_f32(x, gamma, beta, residual)
    D = x.shape[-1]
    rows = x.numel() // D
    if out is None:
        out = torch.empty_like(x)
    _call("gom_layernorm_f32", _p(x), _p(residual), _p(gamma), _p(beta), _p(out), rows, D, eps, _stream())
    return out


def groupnorm32_into(x, gamma, beta, out_view, out_batch_stride, eps=1e-5):
    """x [B,HW,256] -> out_view (pointer to out[0, offset, 0] of a [B,S,256] buffer)."""
    _chk_f32(x, gamma, beta)
    B, HW, C = x.shape
    ws = torch.empty((B * 64,), dtype=torch.float64, device=x.device)
    _call("gom_groupnorm32_nhwc_f32", _p(x), _p(gamma), _p(beta), _p(ws), _p(out_view), out_batch_stride, B, HW, C, eps, _stream())


_masked_streams = {}


def masked_stream(mask_words, device):
    """A torch stream (ExternalStream over gom_stream_create_cu_mask) restricted to the CUs of `mask_words` (list of uint32).
    One hardware queue per (device, mask) for the life of the process: a re-reservation with the same split gets the same queue
    back, so repeated reservations do not accumulate queues.  The queues are deliberately never destroyed: torch's caching
    allocator remembers every stream a block was allocated or recorded on and records an event there when the block is freed --
    possibly long after a reservation ended (gom_stream_destroy under it aborts the process in HIPEvent::record)."""
    key = (_dev_index(device), tuple(int(w) & 0xFFFFFFFF for w in mask_words))
    st = _masked_streams.get(key)
    if st is None:
        arr = (ctypes.c_uint32 * len(mask_words))(*key[1])
        out = ctypes.c_void_p()
        with torch.cuda.device(device):
            _call("gom_stream_create_cu_mask", arr, len(mask_words), ctypes.byref(out))
        st = torch.cuda.ExternalStream(out.value, device=device)
        _masked_streams[key] = st
    return st


K256_GEMM = _switch("K256_GEMM")   # f16x3 back-end: K = 256 products on the row-resident kernel where it measures faster (below)
K256_MAX_ROWS = 1 << 16  # "short" problems (the decoder's Q side: M = frames x queries x points)
K256_LONG = _switch("K256_LONG")   # long problems: N >= 512 on the kernel's whole-line-store form (off: N >= 1024, 16-byte stores)


def k256_wins(M, N, has_a2):
    """Kernel choice from tools/gemm_k256_bench.py (interleaved A/B on MI355X).  Both kernels return the same
    bits, so this is a pure speed rule.  Short problems: N = 256 (21 vs 24 us at M = 20 000) and everything with a second
    addend (the tile kernel needs an `add` launch first: 23-54 vs 32-56 us); long problems (whole-line-store form of the kernel):
    N >= 512 (at M = 297 368: N = 640 with the periodic position table 354 vs 449 us, N = 1536 747 vs 944 us; the tile kernel
    keeps N = 256: 170 vs 175 us)."""
    if M <= K256_MAX_ROWS:
        return N == 256 or has_a2
    return N >= (512 if K256_LONG else 1024)


class K256Linear:
    """An nn.Linear with in_features 256 prepared for gom_gemm_k256_f32: fragment-linear image of the f16x3 planes + inverse
    row scales + bias (csrc/gemm_k256.hip).  `W` (SplitWeight, possibly a row slice) and `bias` stay available for the tile
    kernel, which serves long problems."""

    def __init__(self, W, bias=None):
        assert isinstance(W, SplitWeight) and W.kind == "f16x3"
        nbytes = _L().gom_gemm_k256_image_bytes(W.N, W.K)
        if nbytes < 0:
            raise _lib_mod.GomError("row-resident GEMM kernel does not serve N %d / K %d" % (W.N, W.K))
        pl = W.planes
        self.image = torch.empty((nbytes,), dtype=torch.uint8, device=pl.device)
        _call("gom_gemm_k256_image", _p(pl), pl.stride(0), pl.stride(1), _p(W.inv_scale), _p(bias), W.N, W.K, _p(self.image),
              nbytes, _stream())
        self.W, self.bias, self.N, self.K = W, bias, W.N, W.K


def k256_linear(w, bias=None):
    """(weight, bias) of a K = 256 layer -> K256Linear when the back-end and shape allow, else the pair for ops.gemm."""
    if K256_GEMM and GEMM_MODE == "f16x3" and isinstance(w, SplitWeight) and w.kind == "f16x3" and w.K == 256 and w.N % 32 == 0:
        return K256Linear(w, bias)
    return (w, bias)


def linear(x, lin, A2=None, R=None, relu=False, r_cols=None, out=None, groups=0, r_period=0):
    """act((x [+ A2]) @ W^T + b [+ R]) for `lin` = K256Linear or a (weight, bias) pair; r_period > 0: row m adds
    R[m % r_period] (ops.gemm).  `groups`: column groups of the row-resident kernel's launch; the product always launches ONE
    (every workgroup splits its rows once and walks all columns): splitting the columns over more workgroups re-splits the
    rows per group and measured slower in the step (the decoder's 30 launches: 689 -> 878 us, bench.py same box)."""
    if not isinstance(lin, K256Linear):
        return gemm(x, lin[0], bias=lin[1], A2=A2, R=R, relu=relu, r_cols=r_cols, out=out, r_period=r_period)
    M = x.shape[0]
    # an explicit `groups` forces the kernel (tests, tools)
    if M == 0 or not (groups or k256_wins(M, lin.N, A2 is not None)):
        return gemm(x, lin.W, bias=lin.bias, A2=A2, R=R, relu=relu, r_cols=r_cols, out=out, r_period=r_period)
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == lin.K and x.dtype == _f32
    if A2 is not None:
        assert A2.shape == x.shape and A2.stride() == x.stride() and A2.dtype == _f32
    N = lin.N
    if out is None:
        out = torch.empty((M, N), dtype=_f32, device=x.device)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] == N
    rc = 0
    if R is not None:
        assert R.dim() == 2 and R.stride(1) == 1 and R.dtype == _f32
        rc = r_cols if r_cols is not None else N
    if not K256_LONG:
        _L().gom_gemm_k256_set_lines(0)                      # (A/B switch only: the round-2 mid-state of the kernel)
    with _timed(True, lambda: (2.0 * M * N * lin.K, 4.0 * M * lin.K * (2 if A2 is not None else 1) + lin.image.numel() + 4.0 * M * N
                               + 4.0 * (r_period or M) * rc, "k256:%dx%dx%d" % (M, N, lin.K))):
        _call("gom_gemm_k256_rp_f32", _p(x), _p(A2), _ld(x), _p(lin.image), _p(R), _ld(R), rc, int(r_period), 1 if relu else 0,
              _p(out), _ld(out), M, N, lin.K, groups or 1, _p(range_flag(x.device)), _stream())
    return out


HOIST_MATCH_PROJECTIONS = _switch("HOIST_MATCH_PROJECTIONS")   # native tracker: per-row matcher projections computed once per detection
PROJ_LN = _switch("PROJ_LN")         # f16x3 back-end: out_proj + residual + LayerNorm of every attention block as one launch
POS_PERIODIC = _switch("POS_PERIODIC")   # f16x3 back-end: the encoder's position table read as row m % S (no broadcast copy)


class ProjLN:
    """`LayerNorm(x W^T + b + R)` prepared for gom_proj_ln_f32 (csrc/proj_ln.hip): k-major fragment image of the f16x3 planes of
    W [256, 256] + inverse row scales + bias + the norm's gain / bias.  `pair` / `norm` stay available for the two-launch path."""

    def __init__(self, W, bias, gamma, beta, eps=1e-5):
        assert isinstance(W, SplitWeight) and W.kind == "f16x3"
        nbytes = _L().gom_proj_ln_image_bytes(W.N, W.K)
        if nbytes < 0:
            raise _lib_mod.GomError("projection + LayerNorm kernel does not serve N %d / K %d" % (W.N, W.K))
        _chk_f32(bias, gamma, beta)
        pl = W.planes
        self.image = torch.empty((nbytes,), dtype=torch.uint8, device=pl.device)
        _call("gom_proj_ln_image", _p(pl), pl.stride(0), pl.stride(1), W.N, W.K, _p(self.image), nbytes, _stream())
        self.W, self.bias, self.gamma, self.beta, self.eps = W, bias, gamma, beta, eps


def proj_ln_block(pair, norm):
    """(weight, bias) of an attention block's out_proj + (gamma, beta) of the norm behind it -> ProjLN when the back-end and
    shape allow, else None (callers keep the two-launch path)."""
    w, b = pair if not isinstance(pair, K256Linear) else (pair.W, pair.bias)
    if PROJ_LN and GEMM_MODE == "f16x3" and isinstance(w, SplitWeight) and w.kind == "f16x3" and w.N == 256 and w.K == 256:
        return ProjLN(w, b, norm[0], norm[1])
    return None


def proj_ln(x, blk, R, out=None):
    """LayerNorm(x @ W^T + b [+ R]) * gamma + beta in one launch; x, R [M, 256] row-strided (R may be None)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32
    assert R is None or (R.shape == x.shape and R.stride(1) == 1 and R.dtype == _f32)
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, 256), dtype=_f32, device=x.device)
    with _timed(M > 0, lambda: (2.0 * M * 256 * 256, (12.0 if R is not None else 8.0) * M * 256 + blk.image.numel(),
                                "projln:%dx256x256" % M)):
        _call("gom_proj_ln_f32", _p(x), _ld(x), _p(blk.image), _p(blk.W.inv_scale), _p(blk.bias), _p(R), _ld(R), _p(blk.gamma),
              _p(blk.beta), blk.eps, _p(out), _ld(out), M, _p(range_flag(x.device)), _stream())
    return out


PROPOSAL_DOT = _switch("PROPOSAL_DOT")   # f16x3 back-end: enc_output + norm + class logit of every token as one launch


def proj_ln_dot(x, blk, w, b):
    """[M] = <LayerNorm(x @ W^T + b) * gamma + beta, w> + b in one launch (the normalised rows are not stored); w [256] fp32
    device tensor, b a Python float."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32
    _chk_f32(w)
    assert w.numel() == 256
    M = x.shape[0]
    out = torch.empty((M,), dtype=_f32, device=x.device)
    with _timed(M > 0, lambda: (2.0 * M * 256 * 257, 4.0 * M * 257 + blk.image.numel(), "projdot:%dx256x257" % M)):
        _call("gom_proj_ln_dot_f32", _p(x), _ld(x), _p(blk.image), _p(blk.W.inv_scale), _p(blk.bias), _p(blk.gamma), _p(blk.beta),
              blk.eps, _p(w), float(b), _p(out), M, _p(range_flag(x.device)), _stream())
    return out


BNECK_FUSED = _switch("BNECK_FUSED")   # f16x3 back-end: a bottleneck block's conv3 + residual + ReLU fused with the next block's conv1


BNECK2 = _switch("BNECK2")           # res4's bottleneck tails + next heads (256 -> 1024 -> 256) fused on csrc/bneck2.hip (two workgroups per CU)
# a stage's first block: its 1x1 projection shortcut computed inside the fused launch from the block's input (res2.0); off: the
# shortcut is a launch of its own whose [M, c4] output the fused launch reads back
BNECK_SHORTCUT = _switch("BNECK_SHORTCUT")


class BneckFused:
    """conv3 (1x1, [c4, k1]) + folded BatchNorm + residual + ReLU of one ResNet bottleneck block and conv1 (1x1, [mp, c4]) +
    folded BatchNorm + ReLU of the NEXT block prepared for gom_bneck_f32 (csrc/bneck_fused.hip): the block's output is written once
    and never read back."""

    def __init__(self, w3, scale3, shift3, w1, scale1, shift1, shortcut=None):
        """shortcut = (SplitWeight [c4, ks], scale, shift, stride) of the block's 1x1 projection shortcut: the launch then computes
        the residual from the block's input (`serves_shortcut` says whether the shapes are built)."""
        assert isinstance(w3, SplitWeight) and isinstance(w1, SplitWeight) and w3.kind == "f16x3" and w1.kind == "f16x3"
        self.k1, self.c4, self.mp = w3.K, w3.N, w1.N
        assert w1.K == self.c4
        _chk_f32(scale3, shift3, scale1, shift1)
        p3, p1 = w3.planes, w1.planes
        self.ks, self.stride = 0, 1
        if shortcut is not None:
            ws, scale_s, shift_s, stride = shortcut
            assert BneckFused.serves_shortcut(w3, w1, ws, stride), "fused bottleneck kernel does not serve this shortcut"
            _chk_f32(scale_s, shift_s)
            self.v2, self.ks, self.stride = False, ws.K, int(stride)
            ps = ws.planes
            nbytes = _L().gom_bneck_sc_image_bytes(self.k1, self.c4, self.mp, self.ks, self.stride)
            self.image = torch.empty((nbytes,), dtype=torch.uint8, device=p3.device)
            _call("gom_bneck_sc_image", _p(p3), p3.stride(0), p3.stride(1), _p(w3.inv_scale), _p(scale3), _p(shift3), _p(p1),
                  p1.stride(0), p1.stride(1), _p(ps), ps.stride(0), ps.stride(1), _p(ws.inv_scale), _p(scale_s), _p(shift_s),
                  self.k1, self.c4, self.mp, self.ks, self.stride, _p(self.image), nbytes, _stream())
            self.sc1 = (scale1 * w1.inv_scale).contiguous()
            self.sh1 = shift1.contiguous()
            return
        self.v2 = BneckFused._wide(self.k1, self.c4, self.mp)
        if self.v2:
            # res4 (256 -> 1024 -> 256) and the res3 -> res4 transition (128 -> 512 -> 256): csrc/bneck2.hip, 16-pixel waves, eight per
            # workgroup sharing one weight ring
            nbytes = _L().gom_bneck2_image_bytes(self.k1, self.c4, self.mp)
            self.image = torch.empty((nbytes,), dtype=torch.uint8, device=p3.device)
            _call("gom_bneck2_image", _p(p3), p3.stride(0), p3.stride(1), _p(w3.inv_scale), _p(scale3), _p(shift3), _p(p1),
                  p1.stride(0), p1.stride(1), self.k1, self.c4, self.mp, _p(self.image), nbytes, _stream())
            self.sc1 = (scale1 * w1.inv_scale).contiguous()
            self.sh1 = shift1.contiguous()
            return
        nbytes = _L().gom_bneck_image_bytes(self.k1, self.c4, self.mp)
        if nbytes < 0:
            raise _lib_mod.GomError("fused bottleneck kernel does not serve %d -> %d -> %d" % (self.k1, self.c4, self.mp))
        self.image = torch.empty((nbytes,), dtype=torch.uint8, device=p3.device)
        _call("gom_bneck_image", _p(p3), p3.stride(0), p3.stride(1), _p(w3.inv_scale), _p(scale3), _p(shift3), _p(p1), p1.stride(0),
              p1.stride(1), self.k1, self.c4, self.mp, _p(self.image), nbytes, _stream())
        self.sc1 = (scale1 * w1.inv_scale).contiguous()          # exact: the row scale is a power of two (the tile kernel's product)
        self.sh1 = shift1.contiguous()

    @staticmethod
    def _wide(k1, c4, mp):
        return bool(BNECK2) and _L().gom_bneck2_image_bytes(k1, c4, mp) > 0

    @staticmethod
    def serves(w3, w1):
        return (BNECK_FUSED and GEMM_MODE == "f16x3" and isinstance(w3, SplitWeight) and isinstance(w1, SplitWeight)
                and w3.kind == "f16x3" and w1.kind == "f16x3" and w1.K == w3.N
                and (BneckFused._wide(w3.K, w3.N, w1.N) or _L().gom_bneck_image_bytes(w3.K, w3.N, w1.N) > 0))


    @staticmethod
    def serves_shortcut(w3, w1, ws, stride):
        """By shapes only (never by row count: a frame's bits must not depend on what shares its step)."""
        return (bool(BNECK_SHORTCUT) and BneckFused.serves(w3, w1) and isinstance(ws, SplitWeight) and ws.kind == "f16x3"
                and ws.N == w3.N and _L().gom_bneck_sc_image_bytes(w3.K, w3.N, w1.N, ws.K, int(stride)) > 0)


def _bneck_fused_sc(a, blk, S):
    _chk_f32(a, S)
    B, H, W, k1 = a.shape
    Bs, Hs, Ws, ks = S.shape
    st = blk.stride
    assert k1 == blk.k1 and ks == blk.ks and Bs == B and (H, W) == ((Hs - 1) // st + 1, (Ws - 1) // st + 1)
    assert a.is_contiguous() and S.is_contiguous()
    M = B * H * W
    X = torch.empty((B, H, W, blk.c4), dtype=_f32, device=a.device)
    Y1 = torch.empty((B, H, W, blk.mp), dtype=_f32, device=a.device)
    # profile bytes: A and the sampled rows of S in, X and Y1 out: no residual stream
    with _timed(M > 0, lambda: (2.0 * M * blk.c4 * (blk.k1 + blk.ks + blk.mp), 4.0 * M * (blk.k1 + blk.ks + blk.c4 + blk.mp) + blk.image.numel(),
                                "bneck:%dx%dx%dx%d+sc%d/%d" % (M, blk.k1, blk.c4, blk.mp, blk.ks, st))):
        _call("gom_bneck_sc_f32", _p(a), k1, _p(blk.image), _p(S), ks, B, Hs, Ws, st, _p(blk.sc1), _p(blk.sh1), _p(X), blk.c4,
              _p(Y1), blk.mp, blk.k1, blk.c4, blk.mp, blk.ks, _p(range_flag(a.device)), _stream())
    return X, Y1


def bneck_fused(a, blk, R):
    """(X, Y1) = (relu(bn3(conv3(a)) + R), relu(bn1'(conv1'(X)))) in one launch; a [B, H, W, k1], R [B, H, W, c4] NHWC.  A block
    prepared with its projection shortcut takes the block's INPUT [B, Hs, Ws, ks] in R's place and computes the residual itself."""
    if blk.ks:
        return _bneck_fused_sc(a, blk, R)
    _chk_f32(a, R)
    B, H, W, k1 = a.shape
    assert k1 == blk.k1 and tuple(R.shape) == (B, H, W, blk.c4) and a.is_contiguous() and R.is_contiguous()
    M = B * H * W
    X = torch.empty((B, H, W, blk.c4), dtype=_f32, device=a.device)
    Y1 = torch.empty((B, H, W, blk.mp), dtype=_f32, device=a.device)
    with _timed(M > 0, lambda: (2.0 * M * blk.c4 * (blk.k1 + blk.mp), 4.0 * M * (blk.k1 + 2 * blk.c4 + blk.mp) + blk.image.numel(),
                                "bneck:%dx%dx%dx%d" % (M, blk.k1, blk.c4, blk.mp))):
        _call("gom_bneck2_f32" if blk.v2 else "gom_bneck_f32", _p(a), k1, _p(blk.image), _p(R), blk.c4, _p(blk.sc1), _p(blk.sh1),
              _p(X), blk.c4, _p(Y1), blk.mp, M, blk.k1, blk.c4, blk.mp, _p(range_flag(a.device)), _stream())
    return X, Y1


DEC_ATTN = _switch("DEC_ATTN")       # f16x3 back-end: the decoder's intra / inter self-attention blocks as one launch each
DEC_ATTN_INTRA = _switch("DEC_ATTN_INTRA")
DEC_ATTN_INTER = _switch("DEC_ATTN_INTER")


class DecAttnBlock:
    """One self-attention block of a composite decoder layer -- in_proj (q | k | v), 8 x 32 attention, out_proj, residual,
    LayerNorm -- prepared for gom_dec_attn_f32 (csrc/dec_attn.hip): the fragment-linear image of in_proj_weight [768, 256] and
    out_proj.weight [256, 256] in the kernel's stage order + what its epilogue needs.  `inter`: attention over the queries of a
    (frame, point) (deformable_transformer.py:396-404) instead of over the points of a query (:386-394)."""

    def __init__(self, in_w, in_b, out_w, out_b, gamma, beta, inter, eps=1e-5, raw=None, form=None):
        """raw = (weight [384, 256] as a SplitWeight or fp32 tensor, bias [384]) of the cross attention's sampling_offsets |
        attention_weights layers: an inter block then also serves `dec_attn(..., raw_pos=query_pos)`.  form 2 (default, `DEC_ATTN2`):
        16-token waves, two per SIMD (csrc/dec_attn2.hip); the form-1 image is kept beside it (dec_inter_heads reads its stages)."""
        self.form = form if form is not None else (2 if DEC_ATTN2 else 1)
        assert tuple(in_w.shape) == (768, 256) and tuple(out_w.shape) == (256, 256)
        nbytes = _L().gom_dec_attn_image_bytes(256, 8)
        if nbytes < 0:
            raise _lib_mod.GomError("decoder attention kernel serves d_model 256 / 8 heads only")
        if raw is not None:
            assert inter and tuple(raw[0].shape) == (384, 256)
            nbytes = _L().gom_dec_attn_raw_image_bytes()
        si = in_w if isinstance(in_w, SplitWeight) else split_weight(in_w.contiguous(), kind="f16x3")
        so = out_w if isinstance(out_w, SplitWeight) else split_weight(out_w.contiguous(), kind="f16x3")
        assert si.kind == "f16x3" and so.kind == "f16x3"
        _chk_f32(in_b, out_b, gamma, beta)
        self.image = torch.empty((nbytes,), dtype=torch.uint8, device=si.planes.device)
        pi, po = si.planes, so.planes
        _call("gom_dec_attn_image", _p(pi), pi.stride(0), pi.stride(1), _p(si.inv_scale), _p(in_b), _p(po), po.stride(0),
              po.stride(1), _p(so.inv_scale), _p(out_b), _p(gamma), _p(beta), 1 if inter else 0, _p(self.image), nbytes, _stream())
        self.eps, self.inter, self.has_raw = eps, bool(inter), raw is not None
        if raw is not None:
            sr = raw[0] if isinstance(raw[0], SplitWeight) else split_weight(raw[0].contiguous(), kind="f16x3")
            assert sr.kind == "f16x3"
            _chk_f32(raw[1])
            _call("gom_dec_attn_raw_image", _p(sr.planes), sr.planes.stride(0), sr.planes.stride(1), _p(sr.inv_scale), _p(raw[1]),
                  _p(self.image), nbytes, _stream())
        if self.form == 2:
            n2 = _L().gom_dec_attn2_raw_image_bytes() if raw is not None else _L().gom_dec_attn2_image_bytes(256, 8)
            self.image2 = torch.empty((n2,), dtype=torch.uint8, device=si.planes.device)
            _call("gom_dec_attn2_image", _p(pi), pi.stride(0), pi.stride(1), _p(si.inv_scale), _p(in_b), _p(po), po.stride(0),
                  po.stride(1), _p(so.inv_scale), _p(out_b), _p(gamma), _p(beta), 1 if inter else 0, _p(self.image2), n2, _stream())
            if raw is not None:
                _call("gom_dec_attn2_raw_image", _p(sr.planes), sr.planes.stride(0), sr.planes.stride(1), _p(sr.inv_scale),
                      _p(raw[1]), _p(self.image2), n2, _stream())


DEC_ATTN_RAW = _switch("DEC_ATTN_RAW")      # the inter block's launch also makes the cross attention's offsets | logits
DEC_ATTN2 = _switch("DEC_ATTN2")            # the two blocks on 16-token waves, two per SIMD (csrc/dec_attn2.hip, round 6)


def dec_attn_block(in_w, in_b, out_pair, norm, inter, raw=None):
    """DecAttnBlock when the back-end allows, else None (callers keep the five-launch path)."""
    w, b = out_pair if not isinstance(out_pair, K256Linear) else (out_pair.W, out_pair.bias)
    on = DEC_ATTN and (DEC_ATTN_INTER if inter else DEC_ATTN_INTRA)
    if on and GEMM_MODE == "f16x3" and isinstance(in_w, SplitWeight) and in_w.kind == "f16x3" and tuple(in_w.shape) == (768, 256) \
            and isinstance(w, SplitWeight) and w.kind == "f16x3" and tuple(w.shape) == (256, 256):
        if raw is not None:
            rw, rb = raw if not isinstance(raw, K256Linear) else (raw.W, raw.bias)
            raw = (rw, rb) if (DEC_ATTN_RAW and inter and isinstance(rw, SplitWeight) and rw.kind == "f16x3" and tuple(rw.shape) == (384, 256)) else None
        return DecAttnBlock(in_w, in_b, w, b, norm[0], norm[1], inter, raw=raw)
    return None


def _dec_attn_figures(blk, groups, group_tokens, with_raw, with_pos):
    """Profile record of a `dec_attn` launch: the block's nn.Linear products (in_proj 768 + out_proj 256 [+ raw 384] columns) +
    QK^T and PV of every head; rows in (x [, pos | raw_pos]) and out (out [, raw 384 wide]) + the image."""
    rows = groups * group_tokens
    flops = 2.0 * rows * 256 * (1024 + (384 if with_raw else 0)) + 4.0 * rows * group_tokens * 256
    nbytes = (4.0 * rows * (256 * 3 + 384) if with_raw else 4.0 * rows * 256 * (3 if with_pos else 2)) + blk.image.numel()
    return flops, nbytes, "decattn:%s:%dx%d" % ("inter+raw" if with_raw else "inter" if blk.inter else "intra", groups, group_tokens)


def dec_attn(x, blk, groups, group_tokens, inner=1, pos=None, out=None, raw_pos=None):
    """LayerNorm(x + out_proj(MHA(...))) of one decoder self-attention block in one launch.  x [rows, 256]; intra (blk.inter
    False): `groups` runs of `group_tokens` <= 32 consecutive rows, q = k = x + pos, v = x; inter: token t of group g is row
    ((g // inner) * group_tokens + t) * inner + g % inner, q = k = v = x.  raw_pos (inter blocks built with `raw`): returns
    (out, raw [rows, 384]) with raw = (out + raw_pos) Wraw^T + braw, the cross attention's sampling offsets | attention logits."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32
    assert (pos is None) == blk.inter
    rows = groups * group_tokens
    with_raw = raw_pos is not None
    if with_raw:
        assert blk.inter and blk.has_raw and raw_pos.shape == x.shape and raw_pos.stride(1) == 1 and raw_pos.dtype == _f32
        assert x.shape[0] == rows
    if pos is not None:
        assert pos.shape == x.shape and pos.stride(1) == 1 and pos.dtype == _f32
    assert x.shape[0] >= rows
    if out is None:
        out = torch.empty((x.shape[0], 256), dtype=_f32, device=x.device)
    raw = torch.empty((rows, 384), dtype=_f32, device=x.device) if with_raw else None
    form2 = blk.form == 2
    img = blk.image2 if form2 else blk.image
    with _timed(rows > 0, lambda: _dec_attn_figures(blk, groups, group_tokens, with_raw, pos is not None)):
        if with_raw:
            _call("gom_dec_attn2_raw_f32" if form2 else "gom_dec_attn_raw_f32", _p(x), _ld(x), _p(img), blk.eps, _p(out), _ld(out),
                  _p(raw_pos), _ld(raw_pos), _p(raw), 384, groups, group_tokens, inner, _p(range_flag(x.device)), _stream())
        else:
            _call("gom_dec_attn2_f32" if form2 else "gom_dec_attn_f32", _p(x), _ld(x), _p(pos), _ld(pos), _p(img), blk.eps, _p(out),
                  _ld(out), groups, group_tokens, inner, 1 if blk.inter else 0, _p(range_flag(x.device)), _stream())
    return (out, raw) if with_raw else out


def dec_inter_heads(x, blk, groups, group_tokens, inner, out=None):
    """in_proj + attention core of the inter-instance block for 128 < group_tokens <= 352 (csrc/dec_inter.hip): returns the
    concatenated head outputs [rows, 256] (out_proj + residual + LayerNorm: `proj_ln`).  Row mapping as `dec_attn` (inter)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32 and blk.inter
    rows = groups * group_tokens
    assert x.shape[0] >= rows
    if out is None:
        out = torch.empty((x.shape[0], 256), dtype=_f32, device=x.device)
    # profile flops: in_proj + QK^T and PV of every head
    with _timed(rows > 0, lambda: (2.0 * rows * 256 * 768 + 4.0 * rows * group_tokens * 256, 4.0 * rows * 256 * 2 + 24 * 36864,
                                   "decattn:inter-heads:%dx%d" % (groups, group_tokens))):
        _call("gom_dec_inter_heads_f32", _p(x), _ld(x), _p(blk.image), _p(out), _ld(out), groups, group_tokens, inner,
              _p(range_flag(x.device)), _stream())
    return out


DEC_INTER_MAX_FUSED = 128            # tokens per group the one-launch block (csrc/dec_attn.hip) serves; up to 352: csrc/dec_inter.hip
DEC_INTER_MAX_HEADS = 352
FUSED_FFN = _switch("FUSED_FFN")     # f16x3 back-end: FFN blocks as one fused launch (False: GEMM, GEMM, LayerNorm)


def _ffn_image(w1, b1, w2, refusal=None, acc_order=False, into=None, off=0):
    """Fragment-linear image of a `linear1 [F, D] -> ReLU -> linear2 [D, F]` pair (csrc/ffn_fused.hip; acc_order: linear1 in
    accumulator order, the form a block behind another block of one launch takes) -> (inv_scale1, inv_scale2, image).  The image is
    a new buffer, or the gom_ffn_fused_image_bytes(D, F) bytes of `into` from `off`.  `refusal`: the error's text for shapes the
    kernel does not serve (None: the caller has checked them)."""
    F_, D_ = w1.shape
    assert tuple(w2.shape) == (D_, F_)
    nbytes = _L().gom_ffn_fused_image_bytes(D_, F_)
    if nbytes < 0 and refusal is not None:
        raise _lib_mod.GomError(refusal)
    assert nbytes >= 0
    s1, s2 = split_weight(w1.contiguous(), kind="f16x3"), split_weight(w2.contiguous(), kind="f16x3")
    if into is None:
        into = torch.empty((nbytes,), dtype=torch.uint8, device=w1.device)
    assert off + nbytes <= into.numel()
    p1, p2 = s1.planes, s2.planes
    _call("gom_ffn_fused_image_acc_order" if acc_order else "gom_ffn_fused_image", _p(p1), p1.stride(0), p1.stride(1),
          _p(s1.inv_scale), _p(b1), _p(p2), p2.stride(0), p2.stride(1), D_, F_, ctypes.c_void_p(into.data_ptr() + off), nbytes, _stream())
    return s1.inv_scale, s2.inv_scale, into


class FusedFFN:
    """Weights of one `linear1 -> ReLU -> linear2 -> + residual -> LayerNorm` block prepared for gom_ffn_fused_ln_f32: the
    fragment-linear image of both weight matrices + what the epilogue needs.  Built once per layer (f16x3 mode only)."""

    def __init__(self, w1, b1, w2, b2, gamma, beta, eps=1e-5):
        self.F, self.D = w1.shape
        _, self.inv2, self.image = _ffn_image(w1, b1, w2, "fused FFN kernel does not serve d_model %d / d_hidden %d" % (self.D, self.F))
        self.b2, self.gamma, self.beta, self.eps = b2, gamma, beta, eps


FUSED_MLP2 = _switch("FUSED_MLP2")   # f16x3 back-end: the decoder's two-layer 256 -> 256 -> 256 perceptrons as one launch


class FusedMLP2:
    """linear -> ReLU -> linear [-> ReLU] with 256 inputs and outputs prepared for gom_mlp2_fused_f32 (the fused FFN kernel's
    pipeline without residual / LayerNorm)."""

    def __init__(self, w1, b1, w2, b2, relu_out):
        self.F, self.D = w1.shape
        assert self.D == 256
        _, self.inv2, self.image = _ffn_image(w1, b1, w2, "fused two-layer perceptron does not serve %d -> %d -> %d" % (self.D, self.F, self.D))
        self.b2, self.relu_out = b2.contiguous(), bool(relu_out)


def mlp2_block(w1, b1, w2, b2, relu_out):
    """FusedMLP2 when the back-end and shapes allow (fp32 weights [256, 256] twice), else None."""
    if FUSED_MLP2 and FUSED_FFN and GEMM_MODE == "f16x3" and tuple(w1.shape) == (256, 256) and tuple(w2.shape) == (256, 256):
        return FusedMLP2(w1, b1, w2, b2, relu_out)
    return None


def mlp2_fused(x, blk):
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32
    M = x.shape[0]
    out = torch.empty((M, 256), dtype=_f32, device=x.device)
    with _timed(M > 0, lambda: (4.0 * M * blk.D * blk.F, 8.0 * M * blk.D + blk.image.numel(), "ffn-mlp2:%dx%dx%d" % (M, blk.D, blk.F))):
        _call("gom_mlp2_fused_f32", _p(x), _ld(x), _p(blk.image), _p(blk.inv2), _p(blk.b2), 1 if blk.relu_out else 0, _p(out), 256,
              M, blk.D, blk.F, _p(range_flag(x.device)), _stream())
    return out


def ffn_fused_ln(x, ffn, out=None):
    """LayerNorm(x + FFN(x)) in one launch (csrc/ffn_fused.hip); x [M, 256] row-strided."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == ffn.D and x.dtype == _f32
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, ffn.D), dtype=_f32, device=x.device)
    with _timed(M > 0, lambda: (4.0 * M * ffn.D * ffn.F, 8.0 * M * ffn.D + ffn.image.numel(), "ffn%dx%dx%d" % (M, ffn.D, ffn.F))):
        _call("gom_ffn_fused_ln_f32", _p(x), _ld(x), _p(ffn.image), _p(ffn.inv2), _p(ffn.b2), _p(ffn.gamma), _p(ffn.beta), ffn.eps,
              _p(out), _ld(out), M, ffn.D, ffn.F, _p(range_flag(x.device)), _stream())
    return out


DEC_TAIL = _switch("DEC_TAIL")       # f16x3 back-end: FFN + ctrl_point_coord + reference refinement + the next ref_point_head, one launch


class DecTail:
    """The row-local tail of a composite decoder layer prepared for gom_dec_tail_f32 (csrc/dec_tail.hip): the concatenated
    fragment-linear image of the FFN block, ctrl_point_coord's two hidden layers and ref_point_head (the latter two with their
    first weight in accumulator order), plus the vectors the three epilogues need."""

    def __init__(self, ffn_w, coord_w, qpos_w, dim_t, eps=1e-5, proj_w=None, form=None, waves=None):
        """proj_w = (out_proj weight [256, 256], bias, norm gain, norm bias) of the cross-attention block: the launch then starts from
        the sampled rows (`dec_tail(..., residual=tgt)`).  form 2 (default where the shapes allow, `DEC_TAIL2`): the CU-cooperative
        kernel of csrc/dec_tail2.hip (80 rows per workgroup, the waves split the output columns; `waves` = 4, or 8 = two per SIMD:
        `DEC_TAIL2_WAVES`); form 1: csrc/dec_tail.hip."""
        w1, b1, w2, b2, gamma, beta = ffn_w
        (c1, cb1), (c2, cb2), (W3, b3) = coord_w
        (q1, qb1), (q2, qb2) = qpos_w
        F_, D_ = w1.shape
        if form is None:
            form = 2 if (DEC_TAIL2 and F_ % 128 == 0) else 1
        self.form = form
        self.waves = int(waves) if waves is not None else DEC_TAIL2_WAVES
        assert D_ == 256 and tuple(w2.shape) == (D_, F_) and tuple(W3.shape) == (2, 256) and (form != 2 or F_ % 128 == 0)
        for w in (c1, c2, q1, q2):
            assert tuple(w.shape) == (256, 256)
        self.D, self.F = D_, F_
        L = _L()
        if form == 2:
            self.wave_bytes = {q: L.gom_dec_tail2_wave_bytes(D_, F_, 1 if proj_w is not None else 0, q, self.waves) for q in (0, 1)}
            served = self.wave_bytes[1] >= 0
        else:
            served = L.gom_dec_tail_image_bytes(D_, F_, 1) >= 0
        if not served:
            raise _lib_mod.GomError("decoder tail kernel%s does not serve d_model %d / d_hidden %d" % (" (form 2)" if form == 2 else "", D_, F_))
        so, self.proj = None, None
        if proj_w is not None:
            wo, bo, pg, pb = proj_w
            assert tuple(wo.shape) == (256, 256)
            so = split_weight(wo.contiguous(), kind="f16x3")
            self.proj = (so.inv_scale, bo.contiguous(), pg.contiguous(), pb.contiguous())
        mlps = ((w1, b1, w2), (c1, cb1, c2), (q1, qb1, q2))       # FFN | ctrl_point_coord | ref_point_head
        invs = (self._image2 if form == 2 else self._image1)(mlps, so)
        (self.inv1, self.inv2), (self.c_inv1, self.c_inv2), (self.q_inv1, self.q_inv2) = invs
        self.b1, self.b2, self.gamma, self.beta = b1.contiguous(), b2.contiguous(), gamma.contiguous(), beta.contiguous()
        self.c_b1, self.c_b2, self.q_b1, self.q_b2 = cb1.contiguous(), cb2.contiguous(), qb1.contiguous(), qb2.contiguous()
        self.W3, self.b3, self.dim_t, self.eps = W3.contiguous(), b3.contiguous(), dim_t, eps

    def _image1(self, mlps, so):
        """csrc/dec_tail.hip: the images of [out_proj] | FFN | ctrl_point_coord | ref_point_head back to back, every block behind
        another one with its first weight in accumulator order.  Returns the blocks' (inv_scale1, inv_scale2)."""
        L = _L()
        lin_bytes = L.gom_dec_tail_lin_image_bytes() if so is not None else 0
        nbytes = L.gom_dec_tail_image_bytes(self.D, self.F, 1) + lin_bytes
        self.image = torch.empty((nbytes,), dtype=torch.uint8, device=mlps[0][0].device)
        if so is not None:
            _call("gom_dec_tail_lin_image", _p(so.planes), so.planes.stride(0), so.planes.stride(1), _p(self.image), lin_bytes,
                  _stream())
        off, invs = lin_bytes, []
        for i, (wa, ba, wb) in enumerate(mlps):
            invs.append(_ffn_image(wa, ba, wb, acc_order=i > 0 or so is not None, into=self.image, off=off)[:2])
            off += L.gom_ffn_fused_image_bytes(self.D, wa.shape[0])
        assert off == nbytes
        return invs

    def _image2(self, mlps, so):
        """One linear weight stream per wave (csrc/dec_tail2.hip): [out_proj] | FFN | ctrl_point_coord | ref_point_head; an image
        WITHOUT ref_point_head's part serves the last layer (want_qpos=False): the streams of the two differ only in length.
        Returns the blocks' (inv_scale1, inv_scale2)."""
        nw, wb = self.waves, self.wave_bytes[1]
        self.image = torch.empty((nw * wb,), dtype=torch.uint8, device=mlps[0][0].device)
        blk_bytes = (256 // nw) * 1024                            # a wave's share of a 256 -> 256 layer or of a chunk of 128 hidden units
        off, invs = 0, []
        if so is not None:
            _call("gom_dec_tail2_image_lin", _p(so.planes), so.planes.stride(0), so.planes.stride(1), _p(self.image), wb, off, nw,
                  _stream())
            off += blk_bytes
        for wa, _, wb_ in mlps:
            sa, sb = split_weight(wa.contiguous(), kind="f16x3"), split_weight(wb_.contiguous(), kind="f16x3")
            _call("gom_dec_tail2_image_mlp", _p(sa.planes), sa.planes.stride(0), sa.planes.stride(1), _p(sb.planes),
                  sb.planes.stride(0), sb.planes.stride(1), wa.shape[0], _p(self.image), wb, off, nw, _stream())
            off += (wa.shape[0] // 128) * blk_bytes
            invs.append((sa.inv_scale, sb.inv_scale))
        assert off == wb
        # the last layer's image: the same streams without ref_point_head's part, packed at the shorter stride
        self.image_last = self.image.view(nw, wb)[:, :self.wave_bytes[0]].contiguous().view(-1)
        return invs


DEC_TAIL2 = _switch("DEC_TAIL2")            # ... as the CU-cooperative split-N kernel (csrc/dec_tail2.hip, round 6)
DEC_TAIL2_WAVES = 8 if _switch("DEC_TAIL2_WAVES8") else 4   # ... with eight waves per workgroup (two per SIMD) or four
DEC_TAIL_PROJ = _switch("DEC_TAIL_PROJ")    # ... with the cross-attention's out_proj + norm_cross in front of it


def tail_form2_wins(M, cus=256):
    """Which form of the tail launch is faster at M rows.  A form-2 workgroup (80 rows) takes ~108 us, a form-1 workgroup (128 rows)
    ~148 us -- 0.74 against 0.86 rows per us and CU: form 2 wins by OCCUPANCY where whole rounds of one-per-CU workgroups decide
    (8 x 100 x 25 rows: 250 workgroups in one round against 157 in one), form 1 by throughput where they do not (8 x 300 x 25 rows:
    three rounds of 108 us against two of 148)."""
    def t(rows, us):
        rounds = -(-M // rows) / float(cus)
        return (math.ceil(rounds) if rounds <= 4 else rounds) * us
    return t(80, 108.0) <= t(128, 148.0)


def dec_tail_block(ffn_w, coord_w, qpos_w, dim_t, proj_w=None):
    """DecTail when the back-end and shapes allow, else None (callers keep the four-launch path).  Under `DEC_TAIL2` the block is the
    CU-cooperative form with the round-5 form beside it (`.alt`): `dec_tail` takes the faster one for the planned step's row count
    (`tail_form2_wins`, `plan_rows`): the two forms do not return the same bits."""
    ok = DEC_TAIL and FUSED_FFN and FUSED_MLP2 and REF_UPDATE and GEMM_MODE == "f16x3" and ffn_w[0].shape[1] == 256 and \
        ffn_w[0].shape[0] % 32 == 0 and all(tuple(w.shape) == (256, 256) for w in (coord_w[0][0], coord_w[1][0], qpos_w[0][0], qpos_w[1][0]))
    if proj_w is not None and not (DEC_TAIL_PROJ and tuple(proj_w[0].shape) == (256, 256)):
        proj_w = None
    if not ok:
        return None
    blk = DecTail(ffn_w, coord_w, qpos_w, dim_t, proj_w=proj_w)
    blk.alt = DecTail(ffn_w, coord_w, qpos_w, dim_t, proj_w=proj_w, form=1) if blk.form == 2 else None
    return blk


def _dec_tail_figures(blk, M, want_qpos):
    """Profile record of a `dec_tail` launch: FFN + ctrl_point_coord [+ ref_point_head] + the N = 2 layer [+ out_proj]."""
    flops = 4.0 * M * 256 * blk.F + 4.0 * M * 256 * 256 * (2 if want_qpos else 1) + 4.0 * M * 256 + \
        (2.0 * M * 256 * 256 if blk.proj is not None else 0.0)
    return flops, 4.0 * M * 256 * (3 if want_qpos else 2) + blk.image.numel(), "dectail:%dx%d%s" % (M, blk.F, "+qpos" if want_qpos else "")


def dec_tail(x, blk, ref, want_qpos=True, residual=None, frames=None):
    """(tgt [M,256], new_ref [M,2], qpos [M,256] | None) of one launch: LayerNorm(x + FFN(x)), the refined reference points and the
    NEXT layer's query position (deformable_transformer.py:352-369, :484-488, :470-473).  A block built with `proj_w` takes
    x = the rows sampled by the cross attention and residual = tgt in front of that block: out_proj + norm_cross run first.
    `frames`: how many frames the M rows hold; with it, a block that carries both forms picks by the step plan's rows
    (`plan_rows`) rather than M."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == 256 and x.dtype == _f32
    assert (residual is not None) == (blk.proj is not None)
    _chk_f32(ref)
    M = x.shape[0]
    assert ref.numel() == 2 * M
    assert frames is None or (frames > 0 and M % frames == 0)
    rows = M if frames is None else plan_rows(frames, M // frames)
    if blk.form == 2 and getattr(blk, "alt", None) is not None and not tail_form2_wins(rows):
        blk = blk.alt                                            # many rounds of workgroups: the 128-row form's throughput wins
    out = torch.empty((M, 256), dtype=_f32, device=x.device)
    new_ref = torch.empty_like(ref)
    qpos = torch.empty((M, 256), dtype=_f32, device=x.device) if want_qpos else None
    r = residual
    assert r is None or (r.dim() == 2 and r.stride(1) == 1 and r.shape == x.shape and r.dtype == _f32)
    pi, pb, pg, pbe = blk.proj if blk.proj is not None else (None, None, None, None)
    with _timed(M > 0, lambda: _dec_tail_figures(blk, M, want_qpos)):
        if blk.form == 2:
            _call("gom_dec_tail2_f32", _p(x), _ld(x), _p(r), _ld(r), _p(blk.image if want_qpos else blk.image_last),
                  blk.wave_bytes[1 if want_qpos else 0], blk.F, _p(pi), _p(pb), _p(pg), _p(pbe), blk.eps, _p(blk.inv1), _p(blk.b1),
                  _p(blk.inv2), _p(blk.b2), _p(blk.gamma), _p(blk.beta), blk.eps, _p(blk.c_inv1), _p(blk.c_b1), _p(blk.c_inv2),
                  _p(blk.c_b2), _p(blk.W3), _p(blk.b3), _p(ref), _p(blk.dim_t), _p(blk.q_inv1), _p(blk.q_b1), _p(blk.q_inv2),
                  _p(blk.q_b2), _p(out), 256, _p(new_ref), _p(qpos), 256, M, blk.waves, _p(range_flag(x.device)), _stream())
        elif blk.proj is None:
            _call("gom_dec_tail_f32", _p(x), _ld(x), _p(blk.image), blk.F, _p(blk.inv2), _p(blk.b2), _p(blk.gamma), _p(blk.beta),
                  blk.eps, _p(blk.c_inv2), _p(blk.c_b2), _p(blk.W3), _p(blk.b3), _p(ref), _p(blk.dim_t), _p(blk.q_inv2),
                  _p(blk.q_b2), _p(out), 256, _p(new_ref), _p(qpos), 256, M, _p(range_flag(x.device)), _stream())
        else:
            _call("gom_dec_tail_proj_f32", _p(x), _ld(x), _p(r), _ld(r), _p(blk.image), blk.F, _p(pi), _p(pb), _p(pg), _p(pbe),
                  blk.eps, _p(blk.inv2), _p(blk.b2), _p(blk.gamma), _p(blk.beta), blk.eps, _p(blk.c_inv2), _p(blk.c_b2), _p(blk.W3),
                  _p(blk.b3), _p(ref), _p(blk.dim_t), _p(blk.q_inv2), _p(blk.q_b2), _p(out), 256, _p(new_ref), _p(qpos), 256, M,
                  _p(range_flag(x.device)), _stream())
    return out, new_ref, qpos


# ------------------------------------------------------------------------------------------ MSDA
def _msda_args(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, *more):
    """Preconditions of the native op (ms_deform_attn_cuda.cu:28-52) + the dtype code of its dispatch (:64)."""
    ts = (value, sampling_loc, attn_weight) + more
    if value.dtype not in (_f32, torch.float64):
        raise _lib_mod.GomError("ms_deform_attn: float32 or float64 tensors only (got %s)" % value.dtype)
    for t in ts:
        if t.dtype != value.dtype or not t.is_cuda or not t.is_contiguous():
            raise _lib_mod.GomError("expected a contiguous %s CUDA tensor, got %s %s contiguous=%s" % (
                value.dtype, t.dtype, t.device, t.is_contiguous()))
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise _lib_mod.GomError("spatial_shapes / level_start_index must be int64")
    if not (spatial_shapes.is_cuda and level_start_index.is_cuda and spatial_shapes.is_contiguous()
            and level_start_index.is_contiguous()):
        raise _lib_mod.GomError("spatial_shapes / level_start_index must be contiguous CUDA tensors")
    B, S, M, D = value.shape
    _, Lq, M2, Lv, Pn, two = sampling_loc.shape
    if (sampling_loc.shape[0] != B or M2 != M or two != 2 or tuple(attn_weight.shape) != (B, Lq, M, Lv, Pn)
            or spatial_shapes.shape[0] != Lv or level_start_index.shape[0] != Lv):
        raise _lib_mod.GomError("ms_deform_attn: value [B,S,M,D], sampling_loc [B,Lq,M,L,P,2], attn_weight [B,Lq,M,L,P], "
                                "spatial_shapes [L,2], level_start_index [L] disagree")
    return 0 if value.dtype == _f32 else 1, (B, S, M, D, Lv, Lq, Pn)


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=64):
    """Same signature as the reference's adet._C.ms_deform_attn_forward (im2col_step accepted, unused): any heads / channels /
    levels / points, float32 or float64 (third_party/adet/layers/csrc/DeformAttn/ms_deform_attn_cuda.cu:20-80)."""
    code, dims = _msda_args(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    B, S, M, D, Lv, Lq, Pn = dims
    out = torch.empty((B, Lq, M * D), dtype=value.dtype, device=value.device)
    if code == 0:           # the 1:1 entry: the shipped shape on the wave-per-query kernel, anything else on the general one
        _call("gom_ms_deform_attn_forward", _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc), _p(attn_weight),
              _p(out), B, S, M, D, Lv, Lq, Pn, _stream())
    else:
        _call("gom_ms_deform_attn_forward_any", code, _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc),
              _p(attn_weight), _p(out), B, S, M, D, Lv, Lq, Pn, _stream())
    return out


def ms_deform_attn_forward_any(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    """The general kernel whatever the shape (tests compare it with the wave-per-query kernel on the shipped shape)."""
    code, dims = _msda_args(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    B, S, M, D, Lv, Lq, Pn = dims
    out = torch.empty((B, Lq, M * D), dtype=value.dtype, device=value.device)
    _call("gom_ms_deform_attn_forward_any", code, _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc),
          _p(attn_weight), _p(out), B, S, M, D, Lv, Lq, Pn, _stream())
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step=64):
    """adet._C.ms_deform_attn_backward (ms_deform_attn_cuda.cu:83-156): (grad_value, grad_sampling_loc, grad_attn_weight)."""
    code, dims = _msda_args(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output)
    B, S, M, D, Lv, Lq, Pn = dims
    if grad_output.numel() != B * Lq * M * D:
        raise _lib_mod.GomError("ms_deform_attn_backward: grad_output must hold [B, Lq, M*D] elements")
    gv, gl, gw = torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
    _call("gom_ms_deform_attn_backward", code, _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc),
          _p(attn_weight), _p(grad_output), _p(gv), _p(gl), _p(gw), B, S, M, D, Lv, Lq, Pn, _stream())
    return gv, gl, gw


def ms_deform_attn_forward_strided(value2d, batch_stride, shapes, lsi, loc, w, B, Lq):
    """value2d: [B*S, 256] column slice (stride(1)==1) of a wider buffer; reads it in place."""
    assert value2d.stride(1) == 1
    out = torch.empty((B * Lq, 256), dtype=_f32, device=value2d.device)
    _call("gom_ms_deform_attn_forward_strided", _p(value2d), batch_stride, value2d.stride(0), _p(shapes), _p(lsi), _p(loc), _p(w),
          _p(out), B, Lq, _stream())
    return out


MSDA_LANES = _switch("MSDA_LANES")   # fused MSDA: per-sample arithmetic distributed over a head's lanes (same bits, 3x fewer VALU)
_msda_lanes_set = [None]


MSDA_WINDOW = _switch("MSDA_WINDOW")   # encoder calls: level-0 queries served from LDS windows of the value map (same bits)
# ... and the level-1 queries (round 6): 8 x 16 tiles whose level-0 samples are gathered from global memory (their level-0 window
# would be 1 161 lines) and whose level-1 .. 3 samples come from windows: bit-identical, encoder call 830 -> 808 us.  (4 x 8 tiles with
# all four levels from windows were slower: 958 vs 865 us; profiles/r06_msda_level1_windows_and_offset_scale.log)
MSDA_WINDOW_L1 = _switch("MSDA_WINDOW_L1")
# ... with the window kernel's overlapped fill schedule: the first window is requested in front of the owner part, the others in
# pairs that share the buffer (same windows on the shipped pyramids, same bits; off = one fill at a time, barriers on both sides)
MSDA_WINDOW_OVERLAP = _switch("MSDA_WINDOW_OVERLAP")
# ... and the window kernel's four-lane layout: 4 lanes per (query, head) pair with 8 channels each, the owner's values broadcast by
# DPP inside the quad (same bits, same fallback octets; off = 8 lanes of 4 channels, broadcasts through the LDS crossbar)
MSDA_WINDOW_LANES4 = _switch("MSDA_WINDOW_LANES4")
_msda_window_set = [None]


# Encoder layers decide ONCE, on their first eager call, whether their level-0 queries are worth the LDS windows: the window kernel
# assumes sampling offsets within its 5-pixel halo; an octet group (8 (query, head) pairs) with one sample outside takes the gather
# path after paying for the windows.  Measured at the bench shape (profiles/r06_msda_level1_windows_and_offset_scale.log): 872 us per
# call with no group falling back against 973 us for the gather kernel alone, 1131 us with 87 % falling back (the synthetic weights'
# offsets x 2) -- break-even near 34 %.  A trained checkpoint's offsets are not known here (none ships); the policy makes the
# choice a measurement instead of an assumption.  GOM_MSDA_WINDOW_POLICY=0: always the windows (round 4-5 behaviour).
MSDA_WINDOW_POLICY = _switch("MSDA_WINDOW_POLICY")
MSDA_WINDOW_MAX_FALLBACK = 0.30


def msda_window_groups(encoder_hw0, B):
    """Octet groups of one encoder call's window launches (8 heads x 8-query groups of every tile, padded tiles included)."""
    h0, w0 = int(encoder_hw0[0]), int(encoder_hw0[1])
    n = -(-h0 // 8) * -(-w0 // 16) * 16
    if MSDA_WINDOW_L1 and len(encoder_hw0) >= 4:
        n += -(-int(encoder_hw0[2]) // 8) * -(-int(encoder_hw0[3]) // 16) * 16
    return B * 8 * n


def msda_fused(raw, ref, value2d, batch_stride, shapes, lsi, B, Lq, valid_ratios=None, encoder_hw0=None, fallback_counter=None,
               frame_valid_ratios=None):
    """raw [B*Lq, >=384] (offsets | logits, stride(1)==1), ref [B*Lq, 2], value2d [B*S, 256] column slice;
    valid_ratios [4,2] fp32 (Wv/W, Hv/H) for padded batches.  encoder_hw0 = (H0, W0[, H1, W1]): an ENCODER call (query q = token
    q, reference points = the tokens' own positions) -- the level-0 (and level-1) queries then run on the LDS-window kernel
    (csrc/msda.hip).  fallback_counter: a one-word int32 device tensor the window launches of THIS call add their fallback octet
    groups to (zeroed here).  frame_valid_ratios [B,4,2]: a table per frame (exclusive with valid_ratios)."""
    assert raw.stride(1) == 1 and value2d.stride(1) == 1
    _chk_f32(ref, valid_ratios)
    if frame_valid_ratios is not None:
        assert valid_ratios is None, "valid_ratios and frame_valid_ratios are exclusive"
        _chk_frame_desc(frame_valid_ratios, B, (shapes.shape[0], 2), _f32, "frame_valid_ratios")
    if _msda_lanes_set[0] != MSDA_LANES:                     # library-side switch follows ops.MSDA_LANES
        _L().gom_msda_set_lane_distributed(1 if MSDA_LANES else 0)
        _msda_lanes_set[0] = MSDA_LANES
    out = torch.empty((B * Lq, 256), dtype=_f32, device=raw.device)
    S_rows = value2d.shape[0]
    # profile figures: 2 * Lq * 8 heads * 16 samples * 4 corners * 32; the value map once + raw offsets | logits +
    # output (fp32)
    with _timed(True, lambda: (2.0 * B * Lq * 8 * 16 * 4 * 32, 4.0 * (S_rows * 256 + B * Lq * (384 + 256)), "msda:%dx%d" % (B, Lq))):
        if frame_valid_ratios is not None:
            _call("gom_msda_fused_forward_vr_frames", _p(raw), raw.stride(0), _p(ref), _p(value2d), batch_stride, value2d.stride(0),
                  _p(shapes), _p(lsi), _p(frame_valid_ratios), _p(out), B, Lq, _stream())
        elif valid_ratios is not None:
            _call("gom_msda_fused_forward_vr", _p(raw), raw.stride(0), _p(ref), _p(value2d), batch_stride, value2d.stride(0),
                  _p(shapes), _p(lsi), _p(valid_ratios), _p(out), B, Lq, _stream())
        elif encoder_hw0 is not None and MSDA_WINDOW and MSDA_LANES:
            mask = (3 if MSDA_WINDOW_L1 else 1) | (4 if MSDA_WINDOW_OVERLAP else 0) | (8 if MSDA_WINDOW_LANES4 else 0)
            if _msda_window_set[0] != mask:
                _L().gom_msda_set_window(mask)
                _msda_window_set[0] = mask
            h1, w1 = (int(encoder_hw0[2]), int(encoder_hw0[3])) if len(encoder_hw0) >= 4 else (0, 0)
            if fallback_counter is not None:
                fallback_counter.zero_()
                _L().gom_msda_window_count_fallbacks(_p(fallback_counter))
            try:
                _call("gom_msda_fused_forward_encoder", _p(raw), raw.stride(0), _p(ref), _p(value2d), batch_stride,
                      value2d.stride(0), _p(shapes), _p(lsi), _p(out), B, Lq, int(encoder_hw0[0]), int(encoder_hw0[1]), h1, w1,
                      _stream())
            finally:
                if fallback_counter is not None:
                    _L().gom_msda_window_count_fallbacks(None)
        else:
            _call("gom_msda_fused_forward", _p(raw), raw.stride(0), _p(ref), _p(value2d), batch_stride, value2d.stride(0),
                  _p(shapes), _p(lsi), _p(out), B, Lq, _stream())
    return out


# The decoder's cross-attention value projection on the rows its sampling reads (csrc/dec_value_rows.hip): per layer mark -> compact ->
# the row-list form of the K = 256 kernel, into one [frames x tokens, 256] buffer, instead of one dense N = 1536 launch for the six
# layers.  Every value the sampling reads keeps its bits (value projection is row-local).  GOM_DEC_VALUE_SPARSE=0: the dense launch.
DEC_VALUE_SPARSE = _switch("DEC_VALUE_SPARSE")
# Each decoder layer measures its share of marked rows on its first eager call; a layer above DEC_VALUE_MAX_SHARE makes the model keep
# the dense launch (tools/dec_value_bench.py: the three sparse launches of a layer cost a sixth of the dense launch at a share of
# 48 %; the threshold keeps a margin below that; docs/LAB_NOTES.md).  GOM_DEC_VALUE_POLICY=0: sparse whatever the share.
DEC_VALUE_POLICY = _switch("DEC_VALUE_POLICY")
DEC_VALUE_MAX_SHARE = 0.35


class DecValueRows:
    """Device state of the sparse value projection at one (frames x tokens): the byte flags (zero between layers), the row list and
    its count, and the [n, 256] value buffer -- zero-filled once, so that a row never listed holds finite values; a row listed by
    an earlier layer or step keeps that stale projection, and no sampling reads it."""

    def __init__(self, n, device):
        self.n = n
        self.flags = torch.zeros((_L().gom_dec_value_flag_bytes(n),), dtype=torch.uint8, device=device)
        self.rows = torch.zeros((n,), dtype=torch.int32, device=device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=device)
        self.value = torch.zeros((n, 256), dtype=_f32, device=device)


def dec_value_mark(raw, ref, shapes, lsi, B, Lq, S, state):
    """Flag the rows that `msda_fused(raw, ref, ...)` (the gather kernel: no windows, no valid ratios) loads, in state.flags."""
    assert raw.stride(1) == 1 and state.n == B * S
    _chk_f32(ref)
    _lib_form("gom_dec_value_set_lean_mark", DEC_VALUE_MARK_LEAN)
    _call("gom_dec_value_mark", _p(raw), raw.stride(0), _p(ref), _p(shapes), _p(lsi), B, Lq, S, _p(state.flags), _stream())


def dec_value_compact(state):
    """state.flags -> state.rows[:state.count], ascending."""
    _call("gom_dec_value_compact", _p(state.flags), state.n, _p(state.rows), _p(state.count), _stream())


def linear_rows(x, lin, state, out=None, clear=True):
    """out[r] = x[r] @ W^T + b for the rows r listed in `state` (K256Linear, N = lin.N; `out` defaults to state.value), with the bits
    `linear` gives those rows; other rows of `out` stay.  clear: the listed rows' flags go back to zero."""
    if not isinstance(lin, K256Linear):
        raise _lib_mod.GomError("the row-list GEMM runs on the row-resident K = 256 kernel only (f16x3 back-end)")
    out = state.value if out is None else out
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape == (state.n, lin.K) and x.dtype == _f32
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == state.n and out.shape[1] >= lin.N and out.dtype == _f32
    _call("gom_gemm_k256_rows_f32", _p(x), _ld(x), _p(lin.image), _p(state.rows), _p(state.count), _p(state.flags) if clear else None,
          _p(out), _ld(out), state.n, lin.N, lin.K, _p(range_flag(x.device)), _stream())
    return out


def msda_prepare(raw, ref, spatial_shapes, ref_levels=1):
    """raw [Q, >=384] (offsets | logits), ref [Q, ref_levels, 2] -> loc [Q,8,4,4,2], w [Q,8,4,4]."""
    _chk_f32(ref)
    Q = raw.shape[0]
    loc = torch.empty((Q, 8, 4, 4, 2), dtype=_f32, device=raw.device)
    w = torch.empty((Q, 8, 4, 4), dtype=_f32, device=raw.device)
    _call("gom_msda_prepare", _p(raw), raw.stride(0), _p(ref), ref_levels, _p(spatial_shapes), _p(loc), _p(w), Q, _stream())
    return loc, w


# ------------------------------------------------------------------------------------------ attention
def mha_core(q, k, v, out, outer, inner, heads, head_dim, Lq, Lk, strides):
    arr = (ctypes.c_long * 12)(*[int(s) for s in strides])
    _call("gom_mha_core_f32", _p(q), _p(k), _p(v), _p(out), outer, inner, heads, head_dim, Lq, Lk, arr, _stream())
    return out


def mha_core_segments(q, k, v, out, segments, num_segments, heads, head_dim, ld_q, ld_k, ld_v, ld_o, max_Lq, max_Lk):
    """Ragged batch: segments int32 [S,4] (device) = (first query row, Lq, first key row, Lk) over shared matrices."""
    _call("gom_mha_core_segments_f32", _p(q), _p(k), _p(v), _p(out), _p(segments), num_segments, heads, head_dim, ld_q, ld_k, ld_v,
          ld_o, max_Lq, max_Lk, _stream())
    return out


# ------------------------------------------------------------------------------------------ glue
def preprocess(images, mean, std):
    _chk_f32(images)
    B, C, H, W = images.shape
    assert C == 3
    out = torch.empty((B, H, W, 4), dtype=_f32, device=images.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("gom_preprocess_nchw_to_nhwc4", _p(images), m, s, _p(out), B, H, W, _stream())
    return out


_resample_tables = {}


def _build_resample_tables(in_size, out_size, device):
    ks = _L().gom_resample_ksize_bilinear(in_size, out_size)
    if ks <= 0:
        raise ValueError("bad resample sizes %d -> %d" % (in_size, out_size))
    bounds = torch.empty((out_size, 2), dtype=torch.int32)
    kk = torch.empty((out_size, ks), dtype=torch.int32)
    _call("gom_resample_coeffs_bilinear", in_size, out_size, _p(bounds), _p(kk), ks)
    return (bounds.to(device), kk.to(device), ks)


def resample_tables(in_size, out_size, device):
    """Pillow-bilinear coefficient tables of one axis on `device` (cached): (bounds i32 [out,2], kk i32 [out,ks], ks)."""
    key = (in_size, out_size, str(device))
    hit = _resample_tables.get(key)
    if hit is None:
        hit = _build_resample_tables(in_size, out_size, device)
        _resample_tables[key] = hit
    return hit


def _chk_frames(frames):
    if frames.dtype != torch.uint8 or not frames.is_cuda or not frames.is_contiguous() or frames.dim() != 4 \
            or frames.shape[3] != 3:
        raise ValueError("frames must be a contiguous CUDA uint8 [B,H,W,3] tensor")


def resize_u8(frames, out_h, out_w, flip=False):
    """[B,H,W,3] u8 -> [B,out_h,out_w,3] u8, bit-exact with PIL.Image.resize(BILINEAR)."""
    _chk_frames(frames)
    B, H, W, _ = frames.shape
    xb, xk, xks = resample_tables(W, out_w, frames.device)
    yb, yk, yks = resample_tables(H, out_h, frames.device)
    out = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=frames.device)
    _call("gom_resize_bilinear_u8_hwc3", _p(frames), B, H, W, _p(xb), _p(xk), xks, _p(yb), _p(yk), yks, _p(out), out_h, out_w,
          int(flip), _stream())
    return out


def ingest(frames, out_h, out_w, mean, std, flip):
    """[B,H,W,3] u8 frames -> normalised [B,out_h,out_w,4] f32 backbone input (resize + flip + (x-mean)/std)."""
    _chk_frames(frames)
    B, H, W, _ = frames.shape
    xb, xk, xks = resample_tables(W, out_w, frames.device)
    yb, yk, yks = resample_tables(H, out_h, frames.device)
    out = torch.empty((B, out_h, out_w, 4), dtype=_f32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("gom_ingest_u8_hwc3_to_nhwc4", _p(frames), B, H, W, _p(xb), _p(xk), xks, _p(yb), _p(yk), yks, m, s, _p(out), out_h, out_w,
          int(flip), _stream())
    return out


CROP_TABLES_MAX = 16               # per-axis tables the crop ops keep: random scales give a new size almost every clip
_crop_tables = collections.OrderedDict()


def _crop_resample_tables(in_size, out_size, device):
    """`resample_tables` behind a small LRU of its own (the unbounded cache above serves inference's few fixed sizes, and is
    read but never filled from here).  An evicted table may still be read by a queued launch: its memory goes back to torch's
    allocator, which hands it out again in the order of the stream it was allocated on.  That is safe only while every table is
    built and every crop launch is issued on ONE stream (no `record_stream` is called) -- true of `forward_losses`, the only
    caller; a caller that launches crops on several streams must keep its tables alive itself."""
    key = (in_size, out_size, str(device))
    hit = _crop_tables.pop(key, None)
    if hit is None:
        hit = _resample_tables.get(key)
    if hit is None:
        hit = _build_resample_tables(in_size, out_size, device)
    _crop_tables[key] = hit
    while len(_crop_tables) > CROP_TABLES_MAX:
        _crop_tables.popitem(last=False)
    return hit


def _chk_window(scaled_hw, window):
    SH, SW = (int(v) for v in scaled_hw)
    y0, x0, OH, OW = (int(v) for v in window)
    if min(SH, SW, OH, OW) <= 0 or y0 < 0 or x0 < 0 or y0 + OH > SH or x0 + OW > SW:
        raise ValueError("window (y0=%d, x0=%d, %dx%d) is not inside the %dx%d resized image" % (y0, x0, OH, OW, SH, SW))
    return SH, SW, y0, x0, OH, OW


def resize_crop_u8(frames, scaled_hw, window, flip=False):
    """[B,H,W,3] u8 -> [B,OH,OW,3] u8: `PIL.Image.resize((SW,SH), BILINEAR)` then `[y0:y0+OH, x0:x0+OW]`, bit-exact, one
    launch, no SH x SW intermediate.  scaled_hw = (SH, SW), window = (y0, x0, OH, OW)."""
    SH, SW, y0, x0, OH, OW = _chk_window(scaled_hw, window)
    _chk_frames(frames)
    B, H, W, _ = frames.shape
    xb, xk, xks = _crop_resample_tables(W, SW, frames.device)
    yb, yk, yks = _crop_resample_tables(H, SH, frames.device)
    out = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device=frames.device)
    _call("gom_resize_crop_bilinear_u8_hwc3", _p(frames), B, H, W, _p(xb), _p(xk), xks, _p(yb), _p(yk), yks, _p(out), SH, SW, y0,
          x0, OH, OW, int(flip), _stream())
    return out


def ingest_crop(frames, scaled_hw, window, mean, std, flip):
    """[B,H,W,3] u8 frames -> normalised [B,OH,OW,4] f32 backbone input of the training augmentation: resize to scaled_hw,
    keep `window`, flip, (x-mean)/std (custom_transform.py:46-59 + gom_lstmatcher.py:159-170), one launch."""
    SH, SW, y0, x0, OH, OW = _chk_window(scaled_hw, window)
    _chk_frames(frames)
    B, H, W, _ = frames.shape
    xb, xk, xks = _crop_resample_tables(W, SW, frames.device)
    yb, yk, yks = _crop_resample_tables(H, SH, frames.device)
    out = torch.empty((B, OH, OW, 4), dtype=_f32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("gom_ingest_crop_u8_hwc3_to_nhwc4", _p(frames), B, H, W, _p(xb), _p(xk), xks, _p(yb), _p(yk), yks, m, s, _p(out), SH, SW,
          y0, x0, OH, OW, int(flip), _stream())
    return out


INGEST_MOTION_MAX_FRAMES = _lib_mod.CONSTANTS["GOM_INGEST_MOTION_MAX_FRAMES"]


def motion_tables(H, W, frames):
    """Host half of `ingest_motion`: the coefficient tables of every frame of a motion clip in ONE int32 buffer, and the
    descriptors that point into it.  frames: per frame ((SH, SW), (y0, x0, OH, OW)).  -> (tables int32 [words] (CPU),
    descriptors int32 [T, 12] (CPU; layout in include/gomatching_hip.h), (PH, PW)).  Frames that share a resized size along
    an axis share that axis' table."""
    if not 1 <= len(frames) <= INGEST_MOTION_MAX_FRAMES:
        raise ValueError("a motion clip has 1..%d frames, got %d" % (INGEST_MOTION_MAX_FRAMES, len(frames)))
    L = _L()
    parts, where, words = [], {}, 0

    def table(in_size, out_size):
        nonlocal words
        hit = where.get((in_size, out_size))
        if hit is None:
            ks = L.gom_resample_ksize_bilinear(in_size, out_size)
            if ks <= 0:
                raise ValueError("bad resample sizes %d -> %d" % (in_size, out_size))
            bounds = torch.empty((out_size, 2), dtype=torch.int32)
            kk = torch.empty((out_size, ks), dtype=torch.int32)
            _call("gom_resample_coeffs_bilinear", in_size, out_size, _p(bounds), _p(kk), ks)
            hit = (ks, words, words + bounds.numel())
            words += bounds.numel() + kk.numel()
            parts.extend((bounds.view(-1), kk.view(-1)))
            where[(in_size, out_size)] = hit
        return hit

    desc = []
    for scaled_hw, window in frames:
        SH, SW, y0, x0, OH, OW = _chk_window(scaled_hw, window)
        xks, xb, xk = table(W, SW)
        yks, yb, yk = table(H, SH)
        desc.append([SH, SW, y0, x0, OH, OW, xks, yks, xb, xk, yb, yk])
    return torch.cat(parts), torch.tensor(desc, dtype=torch.int32), (max(d[4] for d in desc), max(d[5] for d in desc))


def ingest_motion(src, frames, mean, std, flip, out=None):
    """ONE u8 image [H,W,3] (or [1,H,W,3]) resident on the GPU -> the normalised, zero-padded batch [T,PH,PW,4] f32 of a
    GEN_IMAGE_MOTION clip in one launch: frame t is the window frames[t] = ((SH, SW), (y0, x0, OH, OW)) of its own Pillow
    bilinear resize, `ingest_crop`'s bits, at the top-left; PH, PW = the largest OH, OW; everything else is written as 0.0
    (`ImageList.from_tensors` of the normalised frames, gom_lstmatcher.py:168-169).  The tables of all frames go up in one
    transfer.  `out`: a contiguous [T,PH,PW,4] f32 tensor to fill (it needs no clearing)."""
    if src.dim() == 4 and src.shape[0] == 1:
        src = src[0]
    if src.dtype != torch.uint8 or not src.is_cuda or not src.is_contiguous() or src.dim() != 3 or src.shape[2] != 3:
        raise ValueError("src must be a contiguous CUDA uint8 [H,W,3] tensor")
    H, W, _ = src.shape
    tables, desc, (PH, PW) = motion_tables(H, W, frames)
    T = desc.shape[0]
    if out is None:
        out = torch.empty((T, PH, PW, 4), dtype=_f32, device=src.device)
    elif out.dtype != _f32 or out.device != src.device or not out.is_contiguous() or tuple(out.shape) != (T, PH, PW, 4):
        raise ValueError("out must be a contiguous float32 [%d,%d,%d,4] tensor on src's device" % (T, PH, PW))
    tab = tables.to(src.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _call("gom_ingest_motion_u8_hwc3_to_nhwc4", _p(src), H, W, _p(tab), tab.numel(), _p(desc), T, m, s, _p(out), PH, PW, int(flip),
          _stream())
    return out


RESULT_ROWS_WORDS = _lib_mod.CONSTANTS["GOM_RESULT_ROWS_WORDS"]


def result_rows(bd, recs, voc_size, track_ids=None):
    """bd [n,25,4] f32, recs [n,25] int64 (CUDA) -> int32 [n, RESULT_ROWS_WORDS]: integer polygon, its fp32 bits, recs,
    CTC emit mask, convex-hull membership and the minimum-area-rectangle edge of every instance, one launch
    (csrc/result_rows.hip; layout in include/gomatching_hip.h)."""
    if not bd.is_cuda or bd.dtype != _f32 or bd.dim() != 3 or tuple(bd.shape[1:]) != (25, 4):
        raise ValueError("bd must be a CUDA float32 [n,25,4] tensor")
    n = bd.shape[0]
    if recs.dtype != torch.int64 or tuple(recs.shape) != (n, 25) or recs.device != bd.device:
        raise ValueError("recs must be an int64 [n,25] tensor on bd's device")
    if track_ids is not None and (track_ids.dtype != torch.int64 or tuple(track_ids.shape) != (n,)
                                  or track_ids.device != bd.device):
        raise ValueError("track_ids must be an int64 [n] tensor on bd's device")
    bd, recs = bd.contiguous(), recs.contiguous()
    track_ids = None if track_ids is None else track_ids.contiguous()
    out = torch.empty((n, RESULT_ROWS_WORDS), dtype=torch.int32, device=bd.device)
    with torch.cuda.device(bd.device):
        _call("gom_result_rows_i32", _p(bd), _p(recs), _p(track_ids), n, int(voc_size), _p(out), RESULT_ROWS_WORDS, _stream())
    return out


RESULT_ROWS_DESC_WORDS = _lib_mod.CONSTANTS["GOM_RR_DESC_WORDS"]


def result_rows_desc(rows, track_ids, sx, sy):
    """The descriptor `result_rows_gather` takes, int32 [n, 6]: ring row, track id low / high word, the fp32 bit patterns of the
    row's scale pair (rounded to fp32 as `scale_xy_` rounds its arguments), 0.  All arguments are arrays of n (or scalars)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n = rows.shape[0]
    if n and (rows.min() < -2 ** 31 or rows.max() >= 2 ** 31):
        raise ValueError("ring rows must fit 32 bits")
    desc = np.zeros((n, RESULT_ROWS_DESC_WORDS), dtype=np.int32)
    desc[:, 0] = rows
    desc[:, 1:3] = np.ascontiguousarray(np.broadcast_to(np.asarray(track_ids, dtype=np.int64), (n,))).view(np.int32).reshape(n, 2)
    desc[:, 3] = np.ascontiguousarray(np.broadcast_to(np.asarray(sx, dtype=np.float32), (n,))).view(np.int32)
    desc[:, 4] = np.ascontiguousarray(np.broadcast_to(np.asarray(sy, dtype=np.float32), (n,))).view(np.int32)
    return desc


def result_rows_gather(bd, recs, desc, voc_size, upload=None):
    """`result_rows` of the instances a host descriptor picks out of a ring: bd [cap,25,4] f32 and recs [cap,25] int64 (CUDA, the
    unscaled fields of every pending frame), desc int32 numpy [n, 6] (`result_rows_desc`) -> int32 [n, RESULT_ROWS_WORDS], row k
    being the row `result_rows` gives for ring row desc[k, 0] after `scale_xy_` with that row's scale pair, carrying that row's
    track id.  One upload (through `upload`, a model's pinned staging `_h2d`, when given), one launch.  A ring row outside
    [0, cap) is refused here, before anything is uploaded."""
    if not bd.is_cuda or bd.dtype != _f32 or bd.dim() != 3 or tuple(bd.shape[1:]) != (25, 4) or not bd.is_contiguous():
        raise ValueError("bd must be a contiguous CUDA float32 [cap,25,4] tensor")
    cap = bd.shape[0]
    if recs.dtype != torch.int64 or tuple(recs.shape) != (cap, 25) or recs.device != bd.device or not recs.is_contiguous():
        raise ValueError("recs must be a contiguous int64 [cap,25] tensor on bd's device")
    if not isinstance(desc, np.ndarray) or desc.dtype != np.int32 or desc.ndim != 2 or desc.shape[1] != RESULT_ROWS_DESC_WORDS:
        raise ValueError("desc must be an int32 numpy array of shape [n, %d]" % RESULT_ROWS_DESC_WORDS)
    n = desc.shape[0]
    if n and (int(desc[:, 0].min()) < 0 or int(desc[:, 0].max()) >= cap):
        raise ValueError("desc names a ring row outside [0, %d)" % cap)
    out = torch.empty((n, RESULT_ROWS_WORDS), dtype=torch.int32, device=bd.device)
    if n == 0:
        return out
    with torch.cuda.device(bd.device):
        desc = np.ascontiguousarray(desc)
        desc_d = upload(desc) if upload is not None else torch.from_numpy(desc).to(bd.device)
        _call("gom_result_rows_gather_i32", _p(bd), _p(recs), cap, _p(desc_d), n, int(voc_size), _p(out), RESULT_ROWS_WORDS,
              _stream())
    return out


RESULT_TEXT_ENTRY_BYTES = _lib_mod.CONSTANTS["GOM_RT_ENTRY_BYTES"]
RESULT_TEXT_SCAN_BLOCK = _lib_mod.CONSTANTS["GOM_RT_SCAN_BLOCK"]


def _chk_display(dev, name, table, W):
    """A display table of `lexicon.DeviceLexicon`: (bytes uint8 [>= 1] CUDA, offsets int32 [W + 1] CUDA, the bytes in use)."""
    data, off, nbytes = table
    _chk_i(dev, (name + " display bytes", data, torch.uint8, (None,)), (name + " display offsets", off, torch.int32, (W + 1,)))
    if data.shape[0] < 1 or not 0 <= int(nbytes) <= data.shape[0]:
        raise ValueError("%s display table: %d bytes in use of %d (at least one is allocated)" % (name, nbytes, data.shape[0]))
    return _p(data), _p(off), int(nbytes)


def result_text(words, pts, keep, frame_rows, first_frame, tables, ov=None, read_with=None):
    """The JSON and XML text of the frames of one call, formatted on the GPU (csrc/result_text.hip; THE RULE is in
    include/gomatching_hip.h, `gom_result_text_*`): words int32 [n, >= RESULT_ROWS_WORDS] as `result_rows` /
    `result_rows_gather` left them, pts int64 [n, 8] and keep uint8 [n] (`results.finish_points`), all CUDA; frame_rows: host
    int32 [F + 1], the CSR offsets of the rows over the call's frames; first_frame: the absolute 0-based index of the call's first
    frame; tables: the (json, xml) pair of uint8 [voc_size - 1, 8] CUDA tensors (`results.text_tables`).
    -> (json u8 tensor, xml u8 tensor, json_frame_off, xml_frame_off): the bytes between the files' header and footer, and int64
    [F + 1] offsets of every frame in each.  Three launches (count and scan, then emit) around ONE synchronising read, the two
    totals, from which the buffers are allocated.  F == 0 gives empty tensors and n == 0 frames without rows, both without a
    launch.  An emitted character id outside the tables raises GomError: nothing was read through it.
    ov = (ov int32 [n], keep_out uint8 [n], json display table, xml display table): the `_ov` entries (the rule of
    `gom_lexicon_rows_*`) -- a row with ov[r] >= 0 takes its transcription from that entry of the display tables
    (`lexicon.DeviceLexicon`), a row writes iff keep[r] and keep_out[r].
    read_with = an int64 CUDA vector that comes back in the SAME copy as the totals (the apply step's counts: no second
    synchronising read); its values are then a fifth element of the result, a list."""
    if not words.is_cuda or words.dtype != torch.int32 or words.dim() != 2 or words.shape[1] < RESULT_ROWS_WORDS or \
            words.stride(1) != 1 and words.shape[0] > 0:
        raise ValueError("words must be a CUDA int32 [n, >= %d] tensor with unit column stride" % RESULT_ROWS_WORDS)
    dev, n = words.device, words.shape[0]
    _chk_i(dev, ("pts", pts, torch.int64, (n, 8)), ("keep", keep, torch.uint8, (n,)))
    json_tab, xml_tab = tables
    ntab = json_tab.shape[0]
    _chk_i(dev, ("json table", json_tab, torch.uint8, (ntab, RESULT_TEXT_ENTRY_BYTES)),
           ("xml table", xml_tab, torch.uint8, (ntab, RESULT_TEXT_ENTRY_BYTES)))
    frame_rows = np.ascontiguousarray(frame_rows, dtype=np.int32).reshape(-1)
    F = frame_rows.shape[0] - 1
    first_frame = int(first_frame)
    if F < 0 or frame_rows[0] != 0 or frame_rows[-1] != n or (np.diff(frame_rows) < 0).any():
        raise ValueError("frame_rows must be non-decreasing offsets from 0 to n = %d" % n)
    if first_frame < 0 or first_frame + F > 2 ** 31 - 2:
        raise ValueError("first_frame + F must fit 31 bits")
    if ov is not None:
        ov_t, keep_out, json_disp, xml_disp = ov
        W = json_disp[1].shape[0] - 1
        _chk_i(dev, ("ov", ov_t, torch.int32, (n,)), ("keep_out", keep_out, torch.uint8, (n,)))
        ov_args = (_p(ov_t), _p(keep_out)) + _chk_display(dev, "json", json_disp, W) + _chk_display(dev, "xml", xml_disp, W) + (W,)
    if F == 0 or n == 0:
        from . import results as _results
        js, xs = _results.host_text_of_empty_frames(first_frame, F)
        joff = np.cumsum([0] + [len(_results.host_text_of_empty_frames(f, 1)[0]) for f in range(first_frame, first_frame + F)])
        xoff = np.cumsum([0] + [len(_results.host_text_of_empty_frames(f, 1)[1]) for f in range(first_frame, first_frame + F)])
        u8 = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
        out = (u8(js), u8(xs), torch.from_numpy(joff.astype(np.int64)).to(dev), torch.from_numpy(xoff.astype(np.int64)).to(dev))
        return out if read_with is None else out + (read_with.tolist(),)
    if ntab < 1:
        raise ValueError("empty tables")
    ld = words.stride(0) if n > 1 else words.shape[1]
    with torch.cuda.device(dev):
        frame_rows_d = torch.from_numpy(frame_rows).to(dev)
        row_len = torch.empty((2, n), dtype=torch.int32, device=dev)
        row_off = torch.empty((2, n + 1), dtype=torch.int64, device=dev)
        row_kept = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        frame_off = torch.empty((2, F + 1), dtype=torch.int64, device=dev)
        totals = torch.empty((_lib_mod.CONSTANTS["GOM_RT_TOTALS"],), dtype=torch.int64, device=dev)
        common = (_p(words), ld, _p(pts), _p(keep), n, _p(frame_rows_d), F, first_frame, _p(json_tab), _p(xml_tab), ntab)
        sfx = ""
        if ov is not None:
            common, sfx = common + ov_args, "_ov"
        _call("gom_result_text_count_scan" + sfx, *common, _p(row_len), _p(row_off), _p(row_kept), _p(frame_off), _p(totals),
              _stream())
        if read_with is not None:
            _chk_i(dev, ("read_with", read_with, torch.int64, (None,)))
            both = torch.cat((totals, read_with)).tolist()   # the one synchronising read, the caller's counts riding along
            (jt, xt, status, _), rode = both[:4], both[4:]
        else:
            jt, xt, status, _ = totals.tolist()              # the one synchronising read
        if status:
            raise _lib_mod.GomError("result_text: an emitted character id lies outside the %d-entry tables (status %d)"
                                    % (ntab, status))
        js = torch.empty((jt,), dtype=torch.uint8, device=dev)
        xs = torch.empty((xt,), dtype=torch.uint8, device=dev)
        _call("gom_result_text_emit" + sfx, *common, _p(row_len), _p(row_off), _p(row_kept), _p(frame_off), _p(js), jt, _p(xs), xt,
              _stream())
    if read_with is not None:
        return js, xs, frame_off[0], frame_off[1], rode
    return js, xs, frame_off[0], frame_off[1]


RESULT_PARSE_MAX_SIZE = _lib_mod.CONSTANTS["GOM_RP_MAX_SIZE"]
RESULT_PARSE_BAD_SIZE = _lib_mod.CONSTANTS["GOM_RP_BAD_SIZE"]


def result_parse(data):
    """The rows of a result file, read from its bytes on the GPU (csrc/result_parse.hip; THE RULE is in
    include/gomatching_hip.h, `gom_result_parse_*`): data uint8 [size] CUDA, the bytes of jsons/<video>.json.
    -> (status, rows): status 0 and a dict of CUDA tensors -- frame_rows int32 [F+1], ids int64 [N], pts int32 [N,8], has_seg
    uint8 [N], t_off int64 [N], t_len int32 [N] (the transcriptions' byte spans in `data`, still escaped), poly_off int32 [N+1],
    poly_xy int32 [P,2] -- with the counts "L", "F", "N", "P"; or a nonzero set of GOM_RP_BAD_* bits and None: the file is not
    the canonical text, which is no error.  Three calls around three synchronising reads of the totals (L; F and N; P and the
    status), because each sizes the next call's buffers; a refusal ends the sequence at the stage that found it.  A size the
    calls do not take (0 bytes, 2^31 - 1 or more) is refused here, without a launch."""
    if not data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("data must be a contiguous CUDA uint8 vector")
    C = _lib_mod.CONSTANTS
    dev, size = data.device, data.shape[0]
    if size < 1 or size > RESULT_PARSE_MAX_SIZE - 1:
        return RESULT_PARSE_BAD_SIZE, None
    i32, i64 = torch.int32, torch.int64
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        nblk = -(-size // C["GOM_RP_BLOCK_BYTES"])
        blk = new((nblk,), i32)
        totals = torch.zeros((C["GOM_RP_TOTALS"],), dtype=i64, device=dev)
        _call("gom_result_parse_lines", _p(data), size, _p(blk), nblk, _p(totals), _stream())
        t = totals.tolist()
        L, status = t[C["GOM_RP_L"]], t[C["GOM_RP_STATUS_LINES"]]
        if status:
            return status, None
        if L == 1:                                            # the two bytes {}
            rows = dict(L=1, F=0, N=0, P=0, frame_rows=torch.zeros((1,), dtype=i32, device=dev), ids=new((0,), i64),
                        pts=new((0, 8), i32), has_seg=new((0,), torch.uint8), t_off=new((0,), i64), t_len=new((0,), i32),
                        poly_off=torch.zeros((1,), dtype=i32, device=dev), poly_xy=new((0, 2), i32))
            return 0, rows
        nmblk = -(-L // C["GOM_RP_BLOCK"])
        line_start, mblk, sblk = new((L + 1,), i32), new((2, nmblk), i32), new((nmblk,), i32)
        _call("gom_result_parse_marks", _p(data), size, _p(blk), nblk, L, _p(line_start), _p(mblk), _p(sblk), nmblk, _p(totals),
              _stream())
        t = totals.tolist()
        F, N, status = t[C["GOM_RP_F"]], t[C["GOM_RP_N"]], t[C["GOM_RP_STATUS_MARKS"]]
        if status:
            return status, None
        cap_p = L // 4
        n1 = max(N, 1)                                        # (an empty tensor has no address to pass)
        rows = dict(frame_rows=new((F + 1,), i32), ids=new((n1,), i64), pts=new((n1, 8), i32), has_seg=new((n1,), torch.uint8),
                    t_off=new((n1,), i64), t_len=new((n1,), i32), poly_off=new((N + 1,), i32))
        poly_xy = new((max(cap_p, 1), 2), i32)
        mark_line, obj_mark, frame_mark = new((N + F + 1,), i32), new((n1,), i32), new((F,), i32)
        unit_status = new((N + F,), i32)
        _call("gom_result_parse_emit", _p(data), size, _p(line_start), L, _p(mblk), nmblk, F, N, _p(mark_line), _p(obj_mark),
              _p(frame_mark), _p(rows["frame_rows"]), _p(rows["poly_off"]), _p(rows["ids"]), _p(rows["pts"]),
              _p(rows["has_seg"]), _p(rows["t_off"]), _p(rows["t_len"]), _p(poly_xy), cap_p, _p(unit_status), _p(totals),
              _stream())
        t = totals.tolist()
        P, status = t[C["GOM_RP_P"]], t[C["GOM_RP_STATUS"]]
        if status:
            return status, None
        for k in ("ids", "pts", "has_seg", "t_off", "t_len"):
            rows[k] = rows[k][:N]
        rows.update(L=L, F=F, N=N, P=P, poly_xy=poly_xy[:P])
    return 0, rows


SCENE_PALETTE = _lib_mod.CONSTANTS["GOM_SP_PALETTE"]
SCENE_BAD_COORD = _lib_mod.CONSTANTS["GOM_SP_BAD_COORD"]


def scene_polygons(frame_rows, ids, poly_off, poly_xy, f0, f1, n_inst, n_cont, p0, p1, H, W, palette, bgr):
    """The polygon side of a drawing scene for frames f0 .. f1 - 1, from the rows `result_parse` left on the GPU
    (csrc/scene_polygons.hip; the rule is in include/gomatching_hip.h, `gom_scene_polygons_i32`): frame_rows int32 [F+1], ids
    int64 [N], poly_off int32 [N+1], poly_xy int32 [P,2], palette uint8 [SCENE_PALETTE,3], all CUDA.  The caller counts, from
    its host copy of frame_rows and poly_off, the chunk's instances `n_inst`, those of them with at least one point `n_cont`,
    and its points p0 = poly_off[frame_rows[f0]] .. p1 = poly_off[frame_rows[f1]].
    -> (points, coff, mcoff, boxes, woff, inst_off, inst_rgb, status): the arrays of `show.device_arrays` (points is the view
    poly_xy[p0:p1]) and an int32 [1] status the caller reads with its next copy back.  Two launches, no
    synchronisation; a chunk without instances launches nothing."""
    dev = frame_rows.device
    i32 = torch.int32
    _chk_i(dev, ("frame_rows", frame_rows, i32, (None,)), ("ids", ids, torch.int64, (None,)), ("poly_off", poly_off, i32, (None,)),
           ("poly_xy", poly_xy, i32, (None, 2)), ("palette", palette, torch.uint8, (SCENE_PALETTE, 3)))
    F, N, P = frame_rows.shape[0] - 1, ids.shape[0], poly_xy.shape[0]
    f0, f1, n_inst, n_cont, p0, p1 = int(f0), int(f1), int(n_inst), int(n_cont), int(p0), int(p1)
    if poly_off.shape[0] != N + 1 or not 0 <= f0 < f1 <= F or not 0 <= n_cont <= n_inst <= N or not 0 <= p0 <= p1 <= P:
        raise ValueError("poly_off must be [N+1], 0 <= f0 < f1 <= F, n_cont <= n_inst <= N and p0 <= p1 point offsets")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > 2 ** 31 - 1:
        raise ValueError("H x W must lie in [1, 2^31 - 1]")
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        if n_inst == 0:
            return (poly_xy[p0:p0], zeros((1,), i32), zeros((1,), i32), zeros((0, 4), i32), zeros((1,), torch.int64),
                    zeros((f1 - f0 + 1,), i32), zeros((0, 3), torch.uint8), zeros((1,), i32))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        coff, mcoff, boxes = new((n_cont + 1,), i32), new((n_inst + 1,), i32), new((n_inst, 4), i32)
        woff, inst_off, inst_rgb = new((n_inst + 1,), torch.int64), new((f1 - f0 + 1,), i32), new((n_inst, 3), torch.uint8)
        inst_status, status = new((n_inst,), i32), new((1,), i32)
        some_xy = poly_xy if P else new((1, 2), i32)         # (an empty tensor has no address to pass; P = 0 reads nothing)
        _call("gom_scene_polygons_i32", _p(frame_rows), F, _p(ids), _p(poly_off), N, _p(some_xy), P, f0, f1, int(H), int(W),
              _p(palette), 1 if bgr else 0, _p(coff), n_cont, _p(mcoff), _p(boxes), _p(woff), _p(inst_off), _p(inst_rgb),
              _p(inst_status), n_inst, _p(status), _stream())
    return poly_xy[p0:p1], coff, mcoff, boxes, woff, inst_off, inst_rgb, status


TRACK_VOTE_RECORD_WORDS = _lib_mod.CONSTANTS["GOM_TV_RECORD_WORDS"]
TRACK_VOTE_ENTRY_MAX = _lib_mod.CONSTANTS["GOM_TV_ENTRY_MAX"]
TRACK_VOTE_BLOCK = _lib_mod.CONSTANTS["GOM_TV_BLOCK"]


def track_vote_records(words, keep, table, ov=None):
    """One record per row of a call (csrc/track_vote.hip; THE RULE is in include/gomatching_hip.h, `gom_track_vote_*`): words
    int32 [n, >= RESULT_ROWS_WORDS] as `result_rows` / `result_rows_gather` left them, keep uint8 [n], table uint8
    [voc_size - 1, 8] (`results.txt_table`), all CUDA -> int32 [n, TRACK_VOTE_RECORD_WORDS]: track id low / high, the text's byte
    length (-1: the row does not vote, -2: an emitted id outside the table), 25 words of text bytes.  One launch, no read back.
    ov = (ov int32 [n], keep_out uint8 [n], txt display table): `gom_track_vote_records_ov_i32` -- a row with ov[r] >= 0 takes
    its text from that entry of the display table, a row votes iff keep[r] and keep_out[r]."""
    if not words.is_cuda or words.dtype != torch.int32 or words.dim() != 2 or words.shape[1] < RESULT_ROWS_WORDS or \
            words.stride(1) != 1 and words.shape[0] > 0:
        raise ValueError("words must be a CUDA int32 [n, >= %d] tensor with unit column stride" % RESULT_ROWS_WORDS)
    dev, n = words.device, words.shape[0]
    ntab = table.shape[0]
    _chk_i(dev, ("keep", keep, torch.uint8, (n,)), ("txt table", table, torch.uint8, (ntab, RESULT_TEXT_ENTRY_BYTES)))
    records = torch.empty((n, TRACK_VOTE_RECORD_WORDS), dtype=torch.int32, device=dev)
    if n == 0:
        return records
    if ntab < 1:
        raise ValueError("an empty table")
    ld = words.stride(0) if n > 1 else words.shape[1]
    with torch.cuda.device(dev):
        if ov is not None:
            ov_t, keep_out, disp = ov
            W = disp[1].shape[0] - 1
            _chk_i(dev, ("ov", ov_t, torch.int32, (n,)), ("keep_out", keep_out, torch.uint8, (n,)))
            _call("gom_track_vote_records_ov_i32", _p(words), ld, _p(keep), n, _p(table), ntab, _p(ov_t), _p(keep_out),
                  *(_chk_display(dev, "txt", disp, W) + (W, _p(records), _stream())))
        else:
            _call("gom_track_vote_records_i32", _p(words), ld, _p(keep), n, _p(table), ntab, _p(records), _stream())
    return records


def track_vote(records):
    """The vote over a video's log: records int32 [m, TRACK_VOTE_RECORD_WORDS] (CUDA, contiguous; `track_vote_records` of every
    call, in file order) -> (text u8 tensor, track ids int64 [T], winner int32 [T], count int32 [T]): the bytes of
    preds/res_<video>.txt, and per line the track's id, the log position of the winning row and how many of the track's rows
    have its text.  The log is ordered by (track id, log position) with a stable sort and cut into tracks here (plumbing); the
    vote, the line lengths and their scan are two launches, the lines a third, around ONE read of {bytes, status}.  A log
    without a voting row gives empty tensors without a launch.  A record flagged for a character id outside the table raises
    GomError."""
    if not records.is_cuda or records.dtype != torch.int32 or records.dim() != 2 or \
            records.shape[1] != TRACK_VOTE_RECORD_WORDS or not records.is_contiguous():
        raise ValueError("records must be a contiguous CUDA int32 [m, %d] tensor" % TRACK_VOTE_RECORD_WORDS)
    dev, m = records.device, records.shape[0]
    if m > 2 ** 31 - 1:
        raise ValueError("a log of more than 2^31 - 1 records")
    C = _lib_mod.CONSTANTS
    with torch.cuda.device(dev):
        ids = records[:, :2].contiguous().view(torch.int64).reshape(m)
        voters = torch.nonzero(records[:, C["GOM_TV_LEN"]] != C["GOM_TV_LEN_DROPPED"]).reshape(-1)
        nv = voters.shape[0]
        if nv == 0:
            return (torch.empty((0,), dtype=torch.uint8, device=dev), torch.empty((0,), dtype=torch.int64, device=dev),
                    torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
        sorted_ids, perm = torch.sort(ids[voters], stable=True)
        order = voters[perm].to(torch.int32)
        track_ids, sizes = torch.unique_consecutive(sorted_ids, return_counts=True)
        T = track_ids.shape[0]
        seg = torch.zeros((T + 1,), dtype=torch.int32, device=dev)
        seg[1:] = torch.cumsum(sizes, 0)
        winner = torch.empty((T, C["GOM_TV_WINNER_WORDS"]), dtype=torch.int32, device=dev)
        line_off = torch.empty((T + 1,), dtype=torch.int64, device=dev)
        totals = torch.empty((C["GOM_TV_TOTALS"],), dtype=torch.int64, device=dev)
        _call("gom_track_vote_count_scan", _p(records), m, _p(order), nv, _p(seg), T, _p(winner), _p(line_off), _p(totals),
              _stream())
        total, status = totals.tolist()                      # the one synchronising read of the vote
        if status:
            raise _lib_mod.GomError("track_vote: %s (status %d)" % (
                "an emitted character id lies outside the table" if status & C["GOM_TV_BAD_ID"] else
                "the ordering of the log is not a cut into tracks", status))
        out = torch.empty((total,), dtype=torch.uint8, device=dev)
        _call("gom_track_vote_emit", _p(records), m, _p(winner), _p(line_off), T, _p(out), total, _stream())
    return out, track_ids, winner[:, 0], winner[:, 1]


def quad_bezier(quads, hw):
    """quads int32 [n,8] (x1,y1,..,x4,y4), hw int32 [n,2] (each quad's image H, W), both CUDA -> int32 [n,16]: the control points
    of the two Bezier curves of every quad, one launch (csrc/prepare.hip; the rule is in include/gomatching_hip.h)."""
    dev = quads.device
    _chk_i(dev, ("quads", quads, torch.int32, (None, 8)), ("hw", hw, torch.int32, (None, 2)))
    n = quads.shape[0]
    if hw.shape[0] != n:
        raise ValueError("hw must be [n,2] for quads [n,8]")
    out = torch.empty((n, 16), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _call("gom_quad_bezier_i32", _p(quads), _p(hw), n, _p(out), _stream())
    return out


def quad_pairs(gt_quads, det_quads, gt_off, det_off, gt_key, det_key, measure, threshold, pairs=None):
    """The (ground truth, detection) pairs of one video whose measure is above `threshold` (csrc/score.hip; contract in
    include/gomatching_hip.h).  gt_quads [G,8] / det_quads [D,8] int32, gt_off / det_off [F+1] int32 (first object of each
    frame), gt_key [G] / det_key [D] int32 (only equal keys pair), all CUDA; measure 0 = IoU, 1 = intersection over the
    detection's area.  -> (counts int32 [G], det int32 [K], value fp64 [K]): kept detections per ground-truth object, then
    per kept pair the detection's index within its frame and the value, ordered by ground truth, then detection.  Two
    launches (count, emit) around the prefix sum of the counts; `pairs` = the per-frame G x D total, if the caller has it."""
    dev = gt_quads.device
    for name, t, shape in (("gt_quads", gt_quads, (None, 8)), ("det_quads", det_quads, (None, 8)), ("gt_off", gt_off, (None,)),
                           ("det_off", det_off, (None,)), ("gt_key", gt_key, (None,)), ("det_key", det_key, (None,))):
        if not t.is_cuda or t.device != dev or t.dtype != torch.int32 or t.dim() != len(shape) or \
                any(s is not None and t.shape[i] != s for i, s in enumerate(shape)) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous CUDA int32 tensor of shape %s" % (name, list(shape)))
    G, D, F = gt_quads.shape[0], det_quads.shape[0], gt_off.shape[0] - 1
    if F < 0 or det_off.shape[0] != F + 1 or gt_key.shape[0] != G or det_key.shape[0] != D:
        raise ValueError("offsets must be [F+1] and keys [G] / [D]")
    if pairs is None:
        pairs = 0 if F == 0 else int(((gt_off[1:] - gt_off[:-1]).to(torch.int64) * (det_off[1:] - det_off[:-1]).to(torch.int64)).sum())
    counts = torch.empty((G,), dtype=torch.int32, device=dev)
    args = (_p(gt_quads), _p(det_quads), _p(gt_off), _p(det_off), _p(gt_key), _p(det_key), G, D, F, int(pairs), int(measure),
            float(threshold))
    with torch.cuda.device(dev):
        _call("gom_quad_pairs_count_f64", *args, _p(counts), _stream())
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(ends[-1]) if G else 0
        scan = ends - counts
        det = torch.empty((total,), dtype=torch.int32, device=dev)
        val = torch.empty((total,), dtype=torch.float64, device=dev)
        _call("gom_quad_pairs_emit_f64", *args, _p(scan), total, _p(det), _p(val), _stream())
    return counts, det, val


QUAD_DET_MATCH_MAX_DET = 4096        # DM_MAX_DET of csrc/score_det.hip: a frame's detections that take part in the matching


def quad_det_match(gt_quads, det_quads, gt_off, det_off, gt_care, iou_thr=0.5, area_thr=0.5, max_det=None):
    """The detection protocol's per-frame greedy matching of one video, one launch (csrc/score_det.hip; the rule is in
    include/gomatching_hip.h).  gt_quads [G,8] / det_quads [D,8] int32, gt_off / det_off [F+1] int32 (first object of each
    frame), gt_care [G] int32 (0 = don't care), all CUDA.  -> (det_care int32 [D], match int32 [G], frame_stats int32 [F,3]):
    whether each detection stays (no don't-care object covers more than `area_thr` of it), per object the matched
    detection's index within its frame or -1, per frame (matched, care objects, care detections).  `max_det` = the largest
    number of detections in a frame, if the caller has it: above 4096 is refused."""
    dev = gt_quads.device
    _chk_i(dev, ("gt_quads", gt_quads, torch.int32, (None, 8)), ("det_quads", det_quads, torch.int32, (None, 8)),
           ("gt_off", gt_off, torch.int32, (None,)), ("det_off", det_off, torch.int32, (None,)),
           ("gt_care", gt_care, torch.int32, (None,)))
    G, D, F = gt_quads.shape[0], det_quads.shape[0], gt_off.shape[0] - 1
    if F < 0 or det_off.shape[0] != F + 1 or gt_care.shape[0] != G:
        raise ValueError("offsets must be [F+1] and gt_care [G]")
    if max_det is None:
        max_det = 0 if F == 0 else int((det_off[1:] - det_off[:-1]).max())
    if max_det > QUAD_DET_MATCH_MAX_DET:
        raise ValueError("a frame with %d detections: at most %d are matched" % (max_det, QUAD_DET_MATCH_MAX_DET))
    det_care = torch.empty((D,), dtype=torch.int32, device=dev)
    match = torch.empty((G,), dtype=torch.int32, device=dev)
    stats = torch.empty((F, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _call("gom_quad_det_match_f64", _p(gt_quads), _p(det_quads), _p(gt_off), _p(det_off), _p(gt_care), G, D, F, float(iou_thr),
              float(area_thr), _p(det_care), _p(match), _p(stats), _stream())
    return det_care, match, stats


def _chk_i(dev, *named):
    for name, t, dtype, shape in named:
        if not t.is_cuda or t.device != dev or t.dtype != dtype or t.dim() != len(shape) or \
                any(s is not None and t.shape[i] != s for i, s in enumerate(shape)) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous CUDA %s tensor of shape %s" % (name, dtype, list(shape)))


def _mask_fill_common(boxes, word_off, H, W, words, area, sel):
    """Checks shared by the two fill calls -> (N, nwords, M): masks, words of the buffer, masks to fill."""
    dev = boxes.device
    _chk_i(dev, ("boxes", boxes, torch.int32, (None, 4)), ("word_off", word_off, torch.int64, (None,)),
           ("words", words, torch.int32, (None,)), ("area", area, torch.int32, (None,)))
    N = boxes.shape[0]
    if word_off.shape[0] != N + 1 or area.shape[0] != N:
        raise ValueError("word_off must be [N+1] and area [N]")
    if sel is not None:
        _chk_i(dev, ("sel", sel, torch.int32, (None,)))
        if sel.shape[0] > N:
            raise ValueError("sel names more masks than there are")
    if boxes.data_ptr() % 16:
        raise ValueError("boxes must be 16-byte aligned")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > 2 ** 31 - 1:
        raise ValueError("H x W must lie in [1, 2^31 - 1]")
    return N, words.shape[0], (N if sel is None else sel.shape[0])


def mask_fill_polygons(points, contour_off, mask_coff, boxes, word_off, H, W, words, area, sel=None):
    """Rasterise polygon masks into their bit rows (csrc/mask_pairs.hip; the rule and the representation are in
    include/gomatching_hip.h).  points int32 [P,2], contour_off int32 [C+1], mask_coff int32 [N+1], boxes int32 [N,4] =
    (y0, y1, wx0, wx1), word_off int64 [N+1], all CUDA; fills `words` (int32 [nwords], the uint32 bit rows) and `area`
    (int32 [N], the popcounts) in place for every mask, or for the masks `sel` (int32 [M]) names.  -> (words, area)."""
    N, nwords, M = _mask_fill_common(boxes, word_off, H, W, words, area, sel)
    _chk_i(boxes.device, ("points", points, torch.int32, (None, 2)), ("contour_off", contour_off, torch.int32, (None,)),
           ("mask_coff", mask_coff, torch.int32, (None,)))
    P, C = points.shape[0], contour_off.shape[0] - 1
    if C < 0 or mask_coff.shape[0] != N + 1:
        raise ValueError("contour_off must be [C+1] and mask_coff [N+1]")
    with torch.cuda.device(boxes.device):
        _call("gom_mask_fill_polygons_u32", _p(points), P, _p(contour_off), C, _p(mask_coff), _p(boxes), _p(word_off), N, nwords,
              _p(sel), M, int(H), int(W), _p(words), _p(area), _stream())
    return words, area


def mask_fill_rle(ends, run_off, boxes, word_off, H, W, words, area, sel=None):
    """Expand COCO run-length masks into their bit rows (csrc/mask_pairs.hip): ends int32 [R] the cumulative run ends (runs
    alternate 0 / 1 from 0, column-major), run_off int32 [N+1]; the other arguments and the result as `mask_fill_polygons`."""
    N, nwords, M = _mask_fill_common(boxes, word_off, H, W, words, area, sel)
    _chk_i(boxes.device, ("ends", ends, torch.int32, (None,)), ("run_off", run_off, torch.int32, (None,)))
    if run_off.shape[0] != N + 1:
        raise ValueError("run_off must be [N+1]")
    with torch.cuda.device(boxes.device):
        _call("gom_mask_fill_rle_u32", _p(ends), ends.shape[0], _p(run_off), _p(boxes), _p(word_off), N, nwords, _p(sel), M, int(H),
              int(W), _p(words), _p(area), _stream())
    return words, area


def mask_pairs(gt_words, gt_boxes, gt_woff, gt_area, det_words, det_boxes, det_woff, det_area, gt_off, det_off, gt_key, det_key,
               threshold, pairs=None):
    """The (ground truth, detection) pairs of one video whose mask IoU is above `threshold` (csrc/mask_pairs.hip; contract
    in include/gomatching_hip.h): two filled mask sets (words, boxes, word offsets, areas as the fill calls leave them),
    gt_off / det_off int32 [F+1], gt_key [G] / det_key [D] int32.  -> the triple of `quad_pairs`: (counts int32 [G], det
    int32 [K], value fp64 [K]), ordered by ground truth, then detection."""
    dev = gt_boxes.device
    i32, i64 = torch.int32, torch.int64
    _chk_i(dev, ("gt_words", gt_words, i32, (None,)), ("gt_boxes", gt_boxes, i32, (None, 4)), ("gt_woff", gt_woff, i64, (None,)),
           ("gt_area", gt_area, i32, (None,)), ("det_words", det_words, i32, (None,)), ("det_boxes", det_boxes, i32, (None, 4)),
           ("det_woff", det_woff, i64, (None,)), ("det_area", det_area, i32, (None,)), ("gt_off", gt_off, i32, (None,)),
           ("det_off", det_off, i32, (None,)), ("gt_key", gt_key, i32, (None,)), ("det_key", det_key, i32, (None,)))
    G, D, F = gt_boxes.shape[0], det_boxes.shape[0], gt_off.shape[0] - 1
    if F < 0 or det_off.shape[0] != F + 1 or gt_key.shape[0] != G or det_key.shape[0] != D or gt_woff.shape[0] != G + 1 or \
            det_woff.shape[0] != D + 1 or gt_area.shape[0] != G or det_area.shape[0] != D:
        raise ValueError("offsets must be [F+1], word offsets [G+1] / [D+1], keys and areas [G] / [D]")
    if gt_boxes.data_ptr() % 16 or det_boxes.data_ptr() % 16:
        raise ValueError("gt_boxes and det_boxes must be 16-byte aligned")
    if pairs is None:
        pairs = 0 if F == 0 else int(((gt_off[1:] - gt_off[:-1]).to(i64) * (det_off[1:] - det_off[:-1]).to(i64)).sum())
    counts = torch.empty((G,), dtype=i32, device=dev)
    args = (_p(gt_words), _p(gt_boxes), _p(gt_woff), _p(gt_area), gt_words.shape[0], _p(det_words), _p(det_boxes), _p(det_woff),
            _p(det_area), det_words.shape[0], _p(gt_off), _p(det_off), _p(gt_key), _p(det_key), G, D, F, int(pairs), float(threshold))
    with torch.cuda.device(dev):
        _call("gom_mask_pairs_count_f64", *args, _p(counts), _stream())
        ends = torch.cumsum(counts, 0, dtype=i64)
        total = int(ends[-1]) if G else 0
        scan = ends - counts
        det = torch.empty((total,), dtype=i32, device=dev)
        val = torch.empty((total,), dtype=torch.float64, device=dev)
        _call("gom_mask_pairs_emit_f64", *args, _p(scan), total, _p(det), _p(val), _stream())
    return counts, det, val


LEXICON_MAX_LEN = _lib_mod.CONSTANTS["GOM_LEXICON_MAX_LEN"]


def lexicon_match(q_chars, q_off, q_seg, w_chars, w_off, seg_off, max_len=None, out=None):
    """The nearest word of its lexicon segment for every query, by Levenshtein distance, lowest index on ties, one launch
    (csrc/lexicon.hip; the rule is in include/gomatching_hip.h).  q_chars int32 [q_nchars] / w_chars int32 [w_nchars] (the
    uint32 code points), q_off [S+1], q_seg [S], w_off [W+1], seg_off [n_seg+1] int32, all CUDA.  -> (index int32 [S], the
    word's index within the query's segment, or -1 for an empty segment; dist int32 [S], 100 beside a -1).  `max_len` = the largest length of a query or a word, if
    the caller has it: above 64 is refused.  `out` = an int32 [2, S] buffer to hold both results (the two returned tensors
    are its rows, so one copy brings both back)."""
    dev = q_off.device
    i32 = torch.int32
    _chk_i(dev, ("q_chars", q_chars, i32, (None,)), ("q_off", q_off, i32, (None,)), ("q_seg", q_seg, i32, (None,)),
           ("w_chars", w_chars, i32, (None,)), ("w_off", w_off, i32, (None,)), ("seg_off", seg_off, i32, (None,)))
    S, W, n_seg = q_seg.shape[0], w_off.shape[0] - 1, seg_off.shape[0] - 1
    if q_off.shape[0] != S + 1 or W < 0 or n_seg < 0:
        raise ValueError("q_off must be [S+1] for q_seg [S], w_off [W+1] and seg_off [n_seg+1]")
    if S > 0 and n_seg == 0:
        raise ValueError("queries without a lexicon segment")
    if max_len is None:
        max_len = max(int((q_off[1:] - q_off[:-1]).max()) if S else 0, int((w_off[1:] - w_off[:-1]).max()) if W else 0)
    if max_len > LEXICON_MAX_LEN:
        raise ValueError("a query or a word of %d code points: at most %d are matched" % (max_len, LEXICON_MAX_LEN))
    if out is None:
        out = torch.empty((2, S), dtype=i32, device=dev)
    else:
        _chk_i(dev, ("out", out, i32, (2, S)))
    with torch.cuda.device(dev):
        _call("gom_lexicon_match_u32", _p(q_chars), q_chars.shape[0], _p(q_off), _p(q_seg), S, _p(w_chars), w_chars.shape[0],
              _p(w_off), W, _p(seg_off), n_seg, int(max_len), _p(out[0]), _p(out[1]), _stream())
    return out[0], out[1]


LEXICON_ROWS_NORM_WORDS = _lib_mod.CONSTANTS["GOM_LR_NORM_WORDS"]
LEXICON_ROWS_TOTALS = _lib_mod.CONSTANTS["GOM_LR_TOTALS"]


def lexicon_rows_queries(words, keep, norm_tab):
    """The lexicon queries of a call's rows (csrc/lexicon_rows.hip; THE RULE is in include/gomatching_hip.h, `gom_lexicon_rows_*`):
    words int32 [n, >= RESULT_ROWS_WORDS], keep uint8 [n], norm_tab int32 [voc_size - 1, 4] (`lexicon.norm_table`: a count and the
    code points of label.upper()), all CUDA -> (q_chars int32 [64 n], q_off int32 [n + 1], q_len int32 [n], q_status int32 [2]):
    the code points of every row's query as `lexicon_match` takes them (CSR; the buffer is sized by the limit, so nothing is read
    back), the lengths (-1: above the limit) and {status, first row above the limit}.  Three launches, no read back."""
    if not words.is_cuda or words.dtype != torch.int32 or words.dim() != 2 or words.shape[1] < RESULT_ROWS_WORDS or \
            words.stride(1) != 1 and words.shape[0] > 0:
        raise ValueError("words must be a CUDA int32 [n, >= %d] tensor with unit column stride" % RESULT_ROWS_WORDS)
    dev, n = words.device, words.shape[0]
    ntab = norm_tab.shape[0]
    _chk_i(dev, ("keep", keep, torch.uint8, (n,)), ("norm table", norm_tab, torch.int32, (ntab, LEXICON_ROWS_NORM_WORDS)))
    if ntab < 1:
        raise ValueError("an empty norm table")
    if n > _lib_mod.CONSTANTS["GOM_LR_MAX_ROWS"]:
        raise ValueError("more than %d rows in one call" % _lib_mod.CONSTANTS["GOM_LR_MAX_ROWS"])
    q_cap = n * LEXICON_MAX_LEN
    q_chars = torch.empty((q_cap,), dtype=torch.int32, device=dev)
    q_off = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
    q_len = torch.empty((n,), dtype=torch.int32, device=dev)
    q_status = torch.zeros((2,), dtype=torch.int32, device=dev)
    ld = words.stride(0) if n > 1 else words.shape[1]
    with torch.cuda.device(dev):
        _call("gom_lexicon_rows_queries_u32", _p(words), ld, _p(keep), n, _p(norm_tab), ntab, _p(q_len), _p(q_off), _p(q_status),
              _p(q_chars), q_cap, _stream())
    return q_chars, q_off, q_len, q_status


def lexicon_rows_apply(keep, q_len, q_status, best_index, best_dist, W, max_dist=1, drop=False):
    """The apply step of `gom_lexicon_rows_*`: keep uint8 [n], q_len int32 [n], q_status int32 [2] (`lexicon_rows_queries`),
    best_index / best_dist int32 [n] (`lexicon_match`), all CUDA; W = the lexicon's words -> (ov int32 [n]: the accepted word's
    index or -1, keep_out uint8 [n], totals int64 [5] = {kept rows in, accepted, dropped, status, first row above the limit}),
    on the device.  One launch, no read back."""
    dev, n = keep.device, keep.shape[0]
    _chk_i(dev, ("keep", keep, torch.uint8, (n,)), ("q_len", q_len, torch.int32, (n,)), ("q_status", q_status, torch.int32, (2,)),
           ("best_index", best_index, torch.int32, (n,)), ("best_dist", best_dist, torch.int32, (n,)))
    if W < 0 or max_dist < 0:
        raise ValueError("W and max_dist must not be negative")
    ov = torch.empty((n,), dtype=torch.int32, device=dev)
    keep_out = torch.empty((n,), dtype=torch.uint8, device=dev)
    totals = torch.zeros((LEXICON_ROWS_TOTALS,), dtype=torch.int64, device=dev)
    if n == 0:
        totals[_lib_mod.CONSTANTS["GOM_LR_FIRST_LONG"]] = -1
    with torch.cuda.device(dev):
        _call("gom_lexicon_rows_apply_i32", _p(keep), _p(q_len), _p(q_status), _p(best_index), _p(best_dist), n, int(W),
              int(max_dist), 1 if drop else 0, _p(ov), _p(keep_out), _p(totals), _stream())
    return ov, keep_out, totals


JPEG_MAX_WIDTH, JPEG_MAX_HEIGHT = _lib_mod.CONSTANTS["GOM_JPEG_MAX_WIDTH"], _lib_mod.CONSTANTS["GOM_JPEG_MAX_HEIGHT"]


def jpeg_encode(frames, quality=95, bgr=True):
    """Baseline JPEG entropy-coded data of u8 frames [F,H,W,3] (CUDA), four launches (csrc/jpeg.hip; the integer rule is in
    include/gomatching_hip.h; `jpeg.header` makes the rest of a file).  -> (payload u8 [offsets[F]] on the device, offsets
    int64 [F+1] on the host): frame f's data is payload[offsets[f]:offsets[f+1]].  One small copy brings the offsets back
    (the payload's size is a result); the caller copies the payload.  Wider than 4096 or higher than 65535 is refused here,
    before any launch."""
    _chk_frames(frames)
    dev = frames.device
    F, H, W, _ = frames.shape
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must lie in 1 .. 100, not %d" % quality)
    if F == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev), torch.zeros((1,), dtype=torch.int64)
    nbytes = _L().gom_jpeg_workspace_bytes(F, H, W)
    if W > JPEG_MAX_WIDTH or H > JPEG_MAX_HEIGHT or nbytes < 0:
        raise _lib_mod.GomError("gom_jpeg_encode_scan_u8 refused: GOM_ERR_UNSUPPORTED (%d x %d frames; at most %d wide and "
                                "%d high are encoded)" % (W, H, JPEG_MAX_WIDTH, JPEG_MAX_HEIGHT))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    off_dev = torch.empty((F + 1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _call("gom_jpeg_encode_scan_u8", _p(frames), F, H, W, 1 if bgr else 0, quality, _p(ws), nbytes, _p(off_dev), _stream())
        offsets = off_dev.cpu()
        total = int(offsets[F])
        payload = torch.empty(((total + 3) // 4 * 4,), dtype=torch.uint8, device=dev)
        _call("gom_jpeg_encode_pack_u8", _p(ws), nbytes, F, H, W, total, _p(payload), payload.shape[0], _stream())
    return payload[:total], offsets


JPEG_DECODE_CHUNK_BYTES = _lib_mod.CONSTANTS["GOM_JPEG_DECODE_CHUNK_BYTES"]
JPEG_DECODE_WALKS = ("segments", "chunks")


def jpeg_decode(plan, bgr=True, device=None, walk="segments", chunk_bytes=None, return_info=False):
    """Baseline JPEG files -> u8 [F,H,W,3] on the device, four launches (csrc/jpeg_decode.hip; the integer rule is in
    include/gomatching_hip.h).  `plan` = `jpeg.plan(files)`: the packed entropy bytes, the segment descriptors and the distinct
    table sets, three uploads.  -> (pixels, status int32 [F] on the device): a frame whose status word is not 0 holds no
    picture and its file goes through Pillow.  A geometry the decoder refuses raises before any launch.
    walk="segments": a wavefront per restart segment (`gom_jpeg_decode_entropy_i16`).  walk="chunks": a lane per `chunk_bytes`
    (a power of two in 16 .. 4096; None: the measured default) of a segment, for files without restart markers
    (`gom_jpeg_decode_entropy_chunks_i16`); the same pixels and status words.  return_info (chunks only) appends seg_info int32
    [nseg, 2] on the device: per segment the route (0 = the chunk walk, 1 = marked and walked serially) and the most settling
    passes of one of its spans."""
    if walk not in JPEG_DECODE_WALKS:
        raise ValueError("walk must be one of %s, not %r" % (", ".join(JPEG_DECODE_WALKS), walk))
    if walk == "segments" and (chunk_bytes is not None or return_info):
        raise ValueError("chunk_bytes and return_info belong to walk=\"chunks\"")
    if walk == "chunks":
        chunk_bytes = JPEG_DECODE_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
        if not (16 <= chunk_bytes <= 4096 and chunk_bytes & (chunk_bytes - 1) == 0):
            raise ValueError("chunk_bytes must be a power of two in 16 .. 4096, not %d" % chunk_bytes)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    F, nseg = int(plan.F), int(plan.desc.shape[0])
    if F == 0:
        raise ValueError("no files")
    geo = (F, int(plan.H), int(plan.W), int(plan.ncomp), int(plan.hs), int(plan.vs))
    nbytes = _L().gom_jpeg_decode_workspace_bytes(*geo)
    if nbytes < 0:
        raise _lib_mod.GomError("gom_jpeg_decode_entropy_i16 refused: GOM_ERR_UNSUPPORTED (%d x %d frames of %d components, "
                                "sampling %dx%d; at most %d wide and %d high, one component or 4:4:4 / 4:2:2 / 4:2:0, are decoded)"
                                % (geo[2], geo[1], geo[3], geo[4], geo[5], JPEG_MAX_WIDTH, JPEG_MAX_HEIGHT))
    if plan.desc.shape != (nseg, _lib_mod.CONSTANTS["GOM_JPEG_DECODE_DESC_WORDS"]) or plan.seg_off.shape != (F + 1,) or \
            plan.frame_set.shape != (F,) or plan.sets.ndim != 2 or plan.sets.shape[1] != _lib_mod.CONSTANTS["GOM_JPEG_DECODE_SET_WORDS"]:
        raise ValueError("a plan whose arrays do not fit its frame count")
    data = np.zeros(((len(plan.data) + 3) // 4 * 4 or 4,), dtype=np.uint8)          # whole words, and never empty
    data[:len(plan.data)] = plan.data
    small = np.concatenate([plan.seg_off.astype(np.int32), plan.frame_set.astype(np.int32),
                            np.ascontiguousarray(plan.sets, dtype=np.int32).reshape(-1)])
    data_d = torch.from_numpy(data).to(dev)
    desc_d = torch.from_numpy(np.ascontiguousarray(plan.desc, dtype=np.int64)).to(dev)
    small_d = torch.from_numpy(small).to(dev)
    seg_off, frame_set, sets = small_d[:F + 1], small_d[F + 1:2 * F + 1], small_d[2 * F + 1:]
    nsets = int(plan.sets.shape[0])
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    status = torch.empty((nseg + F,), dtype=torch.int32, device=dev)
    out = torch.empty((F, geo[1], geo[2], 3), dtype=torch.uint8, device=dev)
    info = torch.empty((nseg, 2), dtype=torch.int32, device=dev) if walk == "chunks" else None
    with torch.cuda.device(dev):
        if walk == "chunks":
            _call("gom_jpeg_decode_entropy_chunks_i16", _p(data_d), len(plan.data), _p(desc_d), nseg, _p(seg_off), _p(sets), nsets,
                  *geo, _p(ws), nbytes, _p(status[:nseg]), _p(status[nseg:]), chunk_bytes, _p(info), _stream())
        else:
            _call("gom_jpeg_decode_entropy_i16", _p(data_d), len(plan.data), _p(desc_d), nseg, _p(seg_off), _p(sets), nsets, *geo,
                  _p(ws), nbytes, _p(status[:nseg]), _p(status[nseg:]), _stream())
        _call("gom_jpeg_decode_pixels_u8", _p(sets), nsets, _p(frame_set), *geo, 1 if bgr else 0, _p(ws), nbytes, _p(out), _stream())
    return (out, status[nseg:], info) if return_info else (out, status[nseg:])


def mask_outline_polygons(points, contour_off, mask_coff, boxes, word_off, H, W, words, sel=None):
    """`mask_fill_polygons` for the outlines alone (csrc/overlay.hip): writes Boundary of the rasterisation rule, without
    Fill and without areas, into `words` (int32 [nwords]) for every mask, or for the masks `sel` names.  -> words."""
    dev = boxes.device
    _chk_i(dev, ("boxes", boxes, torch.int32, (None, 4)), ("word_off", word_off, torch.int64, (None,)),
           ("words", words, torch.int32, (None,)), ("points", points, torch.int32, (None, 2)),
           ("contour_off", contour_off, torch.int32, (None,)), ("mask_coff", mask_coff, torch.int32, (None,)))
    N, P, C = boxes.shape[0], points.shape[0], contour_off.shape[0] - 1
    if word_off.shape[0] != N + 1 or C < 0 or mask_coff.shape[0] != N + 1:
        raise ValueError("word_off and mask_coff must be [N+1] and contour_off [C+1]")
    if sel is not None:
        _chk_i(dev, ("sel", sel, torch.int32, (None,)))
        if sel.shape[0] > N:
            raise ValueError("sel names more masks than there are")
    if boxes.data_ptr() % 16:
        raise ValueError("boxes must be 16-byte aligned")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) > 2 ** 31 - 1:
        raise ValueError("H x W must lie in [1, 2^31 - 1]")
    with torch.cuda.device(dev):
        _call("gom_mask_outline_polygons_u32", _p(points), P, _p(contour_off), C, _p(mask_coff), _p(boxes), _p(word_off), N,
              words.shape[0], _p(sel), N if sel is None else sel.shape[0], int(H), int(W), _p(words), _stream())
    return words


def overlay_compose(frames, face_words, outline_words, boxes, word_off, inst_off, inst_rgb, label_off, label_pos, label_glyph,
                    label_rgb, glyph_wh, glyph_woff, glyph_words, a_face, a_box, out=None, slots=None):
    """Draw instances and labels over u8 frames [F,H,W,3] (csrc/overlay.hip; the integer rule is in
    include/gomatching_hip.h): two mask sets over one set of boxes and word offsets (what `mask_fill_polygons` and
    `mask_outline_polygons` leave), inst_off int32 [F+1], inst_rgb u8 [N,3], the labels (label_off int32 [F+1], label_pos int32
    [L,2], label_glyph int32 [L], label_rgb u8 [L,3]) and the atlas (glyph_wh int32 [G,2], glyph_woff int64 [G+1], glyph_words
    int32, the uint32 bitmap rows), all CUDA.  `out` may be `frames` (in place); default a new tensor.  -> out.
    With `slots` (int32 [F], CUDA) `frames` is a ring u8 [cap,H,W,3] that is only read, frame f is drawn from
    frames[slots[f]] into a dense `out` [F,H,W,3] (default a new tensor; it must not share memory with the ring) by ONE
    `gom_overlay_compose_gather_u8` launch: what the dense call gives for frames[slots].  A slot outside [0, cap) raises."""
    _chk_frames(frames)
    dev = frames.device
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    _chk_i(dev, ("face_words", face_words, i32, (None,)), ("outline_words", outline_words, i32, (None,)),
           ("boxes", boxes, i32, (None, 4)), ("word_off", word_off, i64, (None,)), ("inst_off", inst_off, i32, (None,)),
           ("inst_rgb", inst_rgb, u8, (None, 3)), ("label_off", label_off, i32, (None,)), ("label_pos", label_pos, i32, (None, 2)),
           ("label_glyph", label_glyph, i32, (None,)), ("label_rgb", label_rgb, u8, (None, 3)), ("glyph_wh", glyph_wh, i32, (None, 2)),
           ("glyph_woff", glyph_woff, i64, (None,)), ("glyph_words", glyph_words, i32, (None,)))
    F, H, W, _ = frames.shape
    cap = F
    if slots is not None:
        _chk_i(dev, ("slots", slots, i32, (None,)))
        F = slots.shape[0]
        if cap < 1:
            raise ValueError("a ring of no frames")
        if F and (int(slots.min()) < 0 or int(slots.max()) >= cap):
            raise ValueError("slots must lie in [0, %d), the ring's frames" % cap)
    N, L, G = boxes.shape[0], label_pos.shape[0], glyph_wh.shape[0]
    if inst_off.shape[0] != F + 1 or label_off.shape[0] != F + 1 or word_off.shape[0] != N + 1 or inst_rgb.shape[0] != N or \
            outline_words.shape[0] != face_words.shape[0] or label_glyph.shape[0] != L or label_rgb.shape[0] != L or \
            glyph_woff.shape[0] != G + 1:
        raise ValueError("offsets must be [F+1], word_off [N+1], inst_rgb [N,3], the two word buffers of one size, "
                         "label arrays [L] and glyph_woff [G+1]")
    if boxes.data_ptr() % 16:
        raise ValueError("boxes must be 16-byte aligned")
    if slots is not None:
        if out is None:
            out = torch.empty((F, H, W, 3), dtype=u8, device=dev)
        else:
            _chk_frames(out)
            if tuple(out.shape) != (F, H, W, 3) or out.device != dev:
                raise ValueError("out must be [len(slots),H,W,3] on the device of the ring")
            if out.data_ptr() < frames.data_ptr() + frames.numel() and frames.data_ptr() < out.data_ptr() + out.numel():
                raise ValueError("out must not share memory with the ring: the ring is only read")
        with torch.cuda.device(dev):
            _call("gom_overlay_compose_gather_u8", _p(frames), cap, _p(slots), _p(out), F, H, W, _p(face_words), _p(outline_words),
                  _p(boxes), _p(word_off), N, face_words.shape[0], _p(inst_off), _p(inst_rgb), _p(label_off), _p(label_pos),
                  _p(label_glyph), _p(label_rgb), L, _p(glyph_wh), _p(glyph_woff), _p(glyph_words), G, glyph_words.shape[0],
                  int(a_face), int(a_box), _stream())
        return out
    if out is None:
        out = torch.empty_like(frames)
    elif out is not frames:
        _chk_frames(out)
        if out.shape != frames.shape or out.device != dev:
            raise ValueError("out must have the shape and the device of frames")
    with torch.cuda.device(dev):
        _call("gom_overlay_compose_u8", _p(frames), _p(out), F, H, W, _p(face_words), _p(outline_words), _p(boxes), _p(word_off), N,
              face_words.shape[0], _p(inst_off), _p(inst_rgb), _p(label_off), _p(label_pos), _p(label_glyph), _p(label_rgb), L,
              _p(glyph_wh), _p(glyph_woff), _p(glyph_words), G, glyph_words.shape[0], int(a_face), int(a_box), _stream())
    return out


STEM_POOL = _switch("STEM_POOL")   # f16x3 back-end: the ResNet stem (conv 7x7 / 2 + BN + ReLU + max-pool 3x3 / 2) as one launch


def stem_conv_pool(x, w, scale=None, shift=None):
    """relu(conv7x7 / stride 2 / pad 3 (x) * scale + shift) followed by max_pool2d(3, 2, 1), one launch (csrc/stem_pool.hip):
    x [B, H, W, 4] fp32, w = prep_conv_weight of the [64, 7, 7, 4] stem weight under the f16x3 back-end.  Equal bit for bit to
    conv2d_nhwc(..., relu=True, stride=2, pad=3) + maxpool3x3s2."""
    assert isinstance(w, SplitWeight) and w.kind == "f16x3" and tuple(w.conv_shape) == (64, 7, 7, 4)
    _chk_f32(x, scale, shift)
    B, H, Wd, Cin = x.shape
    assert Cin == 4 and x.is_contiguous()
    OH, OW = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
    PH, PW = (OH + 2 - 3) // 2 + 1, (OW + 2 - 3) // 2 + 1
    y = torch.empty((B, PH, PW, 64), dtype=_f32, device=x.device)
    pl = w.planes
    _call("gom_stem_conv_pool_f32", _p(x), _p(pl), pl.stride(0), pl.stride(1), _p(w.inv_scale), _p(scale), _p(shift), _p(y), B, H,
          Wd, _p(range_flag(x.device)), _stream())
    return y


def stem_pool_serves(w):
    return bool(STEM_POOL and GEMM_MODE == "f16x3" and isinstance(w, SplitWeight) and w.kind == "f16x3"
                and tuple(getattr(w, "conv_shape", ())) == (64, 7, 7, 4))


def maxpool3x3s2(x):
    _chk_f32(x)
    B, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, OH, OW, C), dtype=_f32, device=x.device)
    _call("gom_maxpool3x3s2_nhwc_f32", _p(x), _p(y), B, H, W, C, _stream())
    return y


def pos_encoding_into(dim_t, level_embed_row, out_view, H, W, valid_hw=None):
    if valid_hw is not None:
        _call("gom_pos_encoding_2d_valid_f32", _p(dim_t), _p(level_embed_row), _p(out_view), H, W, int(valid_hw[0]),
              int(valid_hw[1]), _stream())
        return
    _call("gom_pos_encoding_2d_f32", _p(dim_t), _p(level_embed_row), _p(out_view), H, W, _stream())


def point_pos_embed(pts, dim_t):
    _chk_f32(pts, dim_t)
    Q = pts.numel() // 2
    out = torch.empty((Q, 256), dtype=_f32, device=pts.device)
    _call("gom_point_pos_embed_f32", _p(pts), _p(dim_t), _p(out), Q, _stream())
    return out


def ref_sigmoid(delta, ref, C):
    _chk_f32(ref)
    Q = ref.numel() // 2
    out = torch.empty((Q, C), dtype=_f32, device=ref.device)
    _call("gom_ref_sigmoid_f32", _p(delta), delta.stride(0), _p(ref), _p(out), Q, C, _stream())
    return out


REF_UPDATE = _switch("REF_UPDATE")   # decoder: last MLP layer (N = 2) + reference refinement + next layer's point embedding, one launch


def ref_update(h, last, ref, dim_t, scale=None, want_pos=True, frame_scales=None):
    """(new_ref [Q,2], pos [Q,256] | None): sigmoid(h @ W3^T + b3 + inverse_sigmoid(ref)) and the sine embedding of the new
    reference points (times `scale` = the level-0 valid ratios of a padded batch); `last` = the (weight [2,256], bias) pair.
    frame_scales [B,2]: a scale pair per frame of Q / B points each (exclusive with `scale`)."""
    W3, b3 = last
    _chk_f32(ref, W3, b3, dim_t)
    assert h.dim() == 2 and h.stride(1) == 1 and h.shape[1] == 256 and h.dtype == _f32 and tuple(W3.shape) == (2, 256)
    Q = ref.numel() // 2
    assert h.shape[0] == Q
    new_ref = torch.empty_like(ref)
    pos = torch.empty((Q, 256), dtype=_f32, device=ref.device) if want_pos else None
    if frame_scales is not None:
        assert scale is None, "scale and frame_scales are exclusive"
        B = frame_scales.shape[0] if frame_scales.dim() else 0
        if B <= 0 or Q % B:
            raise _lib_mod.GomError("frame_scales: %d points do not divide into %s frames" % (Q, B))
        _chk_frame_desc(frame_scales, B, (2,), _f32, "frame_scales")
        _call("gom_ref_update_frames_f32", _p(h), _ld(h), _p(W3), _p(b3), _p(ref), _p(dim_t), _p(frame_scales), Q // B, _p(new_ref),
              _p(pos), Q, _stream())
        return new_ref, pos
    sx, sy = scale if scale is not None else (1.0, 1.0)
    _call("gom_ref_update_f32", _p(h), _ld(h), _p(W3), _p(b3), _p(ref), _p(dim_t), float(sx), float(sy), _p(new_ref), _p(pos), Q,
          _stream())
    return new_ref, pos


def proposal_valid(shapes, lsi, S, vshapes=None):
    out = torch.empty((S,), dtype=torch.uint8, device=shapes.device)
    if vshapes is not None:
        _call("gom_proposal_valid_masked", _p(shapes), _p(lsi), shapes.shape[0], _p(vshapes), _p(out), S, _stream())
        return out
    _call("gom_proposal_valid", _p(shapes), _p(lsi), shapes.shape[0], _p(out), S, _stream())
    return out


def zero_padded_tokens_(buf, col0, ncols, shapes, lsi, vshapes, B, S):
    """buf [B*S, ld]: zero columns [col0, col0+ncols) of the tokens outside their level's valid region."""
    _chk_f32(buf)
    _call("gom_zero_padded_tokens_f32", _p(buf), buf.stride(0), col0, ncols, _p(shapes), _p(lsi), _p(vshapes), shapes.shape[0], B,
          S, _stream())
    return buf


def zero_padded_tokens_frames_(buf, col0, ncols, shapes, lsi, frame_vshapes, B, S):
    """`zero_padded_tokens_` with frame tok // S's valid extents: frame_vshapes [B,L,2] int64."""
    _chk_f32(buf)
    _chk_frame_desc(frame_vshapes, B, (shapes.shape[0], 2), torch.int64, "frame_vshapes")
    _call("gom_zero_padded_tokens_frames_f32", _p(buf), buf.stride(0), col0, ncols, _p(shapes), _p(lsi), _p(frame_vshapes),
          shapes.shape[0], B, S, _stream())
    return buf


def padded_geometry(dim_t, level_embed, shapes, lsi, frame_vshapes, B, S):
    """The geometry tables of a padded batch whose frames have their own valid extents (frame_vshapes [B,L,2] int64), ONE launch:
    (lvl_pos [B,S,256], enc_ref [B,S,2], valid [B,S] uint8) -- per frame what `pos_encoding_into(..., valid_hw)` + level embed,
    `encoder_reference_points(..., vshapes)` and `proposal_valid(..., vshapes)` give for that frame's extents."""
    L = shapes.shape[0]
    _chk_f32(dim_t, level_embed)
    assert tuple(level_embed.shape) == (L, 256) and dim_t.numel() == 128
    _chk_frame_desc(frame_vshapes, B, (L, 2), torch.int64, "frame_vshapes")
    dev = shapes.device
    lvl_pos = torch.empty((B, S, 256), dtype=_f32, device=dev)
    ref = torch.empty((B, S, 2), dtype=_f32, device=dev)
    valid = torch.empty((B, S), dtype=torch.uint8, device=dev)
    _call("gom_padded_geometry_f32", _p(dim_t), _p(level_embed), _p(shapes), _p(lsi), _p(frame_vshapes), L, B, S, _p(lvl_pos),
          _p(ref), _p(valid), _stream())
    return lvl_pos, ref, valid


def encoder_reference_points(shapes, lsi, S, vshapes=None):
    out = torch.empty((S, 2), dtype=_f32, device=shapes.device)
    if vshapes is not None:
        _call("gom_encoder_reference_points_masked", _p(shapes), _p(lsi), _p(vshapes), shapes.shape[0], _p(out), S, _stream())
        return out
    _call("gom_encoder_reference_points", _p(shapes), _p(lsi), shapes.shape[0], _p(out), S, _stream())
    return out


def bezier_reference_points(coord_raw, topk_idx, shapes, lsi, bern, B, S, nq, P, compact=False, vshapes=None, frame_vshapes=None):
    """coord_raw: [B,S,8] (compact=False) or the selected tokens' rows [B*nq,8] (compact=True).  vshapes [L,2]: the batch's valid
    extents; frame_vshapes [B,L,2]: every frame's own (exclusive)."""
    _chk_f32(coord_raw, bern)
    out = torch.empty((B, nq, P, 2), dtype=_f32, device=coord_raw.device)
    if frame_vshapes is not None:
        assert vshapes is None, "vshapes and frame_vshapes are exclusive"
        _chk_frame_desc(frame_vshapes, B, (shapes.shape[0], 2), torch.int64, "frame_vshapes")
        _call("gom_bezier_reference_points_frames", _p(coord_raw), _p(topk_idx), _p(shapes), _p(lsi), _p(frame_vshapes),
              shapes.shape[0], _p(bern), _p(out), B, S, nq, P, 1 if compact else 0, _stream())
        return out
    if vshapes is not None:
        _call("gom_bezier_reference_points_masked", _p(coord_raw), _p(topk_idx), _p(shapes), _p(lsi), _p(vshapes), shapes.shape[0],
              _p(bern), _p(out), B, S, nq, P, 1 if compact else 0, _stream())
        return out
    _call("gom_bezier_reference_points", _p(coord_raw), _p(topk_idx), _p(shapes), _p(lsi), shapes.shape[0], _p(bern), _p(out), B, S,
          nq, P, 1 if compact else 0, _stream())
    return out


def scale_xy_(x, sx, sy):
    """In-place scaling of interleaved (x, y) pairs of a contiguous tensor."""
    _chk_f32(x)
    _call("gom_scale_xy_f32", _p(x), x.numel() // 2, float(sx), float(sy), _stream())
    return x


def scale_xy_frames_(x, frame_scales):
    """`scale_xy_` with a scale pair per frame: frame_scales [B,2], x = B equal runs of (x, y) pairs."""
    _chk_f32(x)
    B = frame_scales.shape[0] if frame_scales.dim() else 0
    n = x.numel() // 2
    if B <= 0 or n % B:
        raise _lib_mod.GomError("frame_scales: %d pairs do not divide into %s frames" % (n, B))
    _chk_frame_desc(frame_scales, B, (2,), _f32, "frame_scales")
    _call("gom_scale_xy_frames_f32", _p(x), n, _p(frame_scales), n // B, _stream())
    return x


def copy_words(src, dst):
    """dst <- src over 32-bit words by a kernel (src: pinned host tensor or device tensor of the same byte size)."""
    nbytes = src.numel() * src.element_size()
    assert nbytes == dst.numel() * dst.element_size() and nbytes % 4 == 0 and src.is_contiguous() and dst.is_contiguous()
    _call("gom_copy_words", src.data_ptr(), dst.data_ptr(), nbytes // 4, _stream())
    return dst


def add(a, b):
    _chk_f32(a, b)
    out = torch.empty_like(a)
    _call("gom_add_f32", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def broadcast_rows(src, B):
    _chk_f32(src)
    out = torch.empty((B,) + tuple(src.shape), dtype=_f32, device=src.device)
    _call("gom_broadcast_rows_f32", _p(src), _p(out), src.numel(), B, _stream())
    return out


def topk_tokens(logits, B, S, k, valid=None, invalid_logit=None, with_rows=False, frame_valid=None):
    """logits: [B*S, ld] (column 0 used) -> int32 [B,k] sorted by value desc.  valid [S]: one validity row for the batch;
    frame_valid [B,S]: a row per frame (exclusive)."""
    nbytes = _L().gom_topk_workspace_bytes(B, S, k)
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=logits.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=logits.device)
    rows = torch.empty((B, k), dtype=torch.int32, device=logits.device) if with_rows else None
    _lib_form("gom_topk_set_lean", TOPK_LEAN)
    if frame_valid is not None:
        assert valid is None, "valid and frame_valid are exclusive"
        _chk_frame_desc(frame_valid, B, (S,), torch.uint8, "frame_valid")
        _call("gom_topk_tokens_frames", _p(logits), logits.stride(0), _p(frame_valid), _p(invalid_logit), B, S, k, _p(ws), _p(idx),
              _p(rows), _stream())
        return (idx, rows) if with_rows else idx
    _call("gom_topk_tokens", _p(logits), logits.stride(0), _p(valid), _p(invalid_logit), B, S, k, _p(ws), _p(idx), _p(rows),
          _stream())
    return (idx, rows) if with_rows else idx


def argmax_rows(x):
    rows, V = x.shape
    out = torch.empty((rows,), dtype=torch.int32, device=x.device)
    _call("gom_argmax_rows_f32", _p(x), x.stride(0), V, rows, _p(out), _stream())
    return out


def detect_post(cls, recls, ctrl, bd, recs, B, nq, P, img_h, img_w, det_thr, nms_thr, asso_thr, frame_sizes=None):
    """frame_sizes [B,2] fp32 (img_h, img_w): a size per frame instead of the two scalars (pass img_h = img_w = None)."""
    dev = cls.device
    # count | keep_idx | scores | boxes share one buffer so the host needs a single D2H copy per step
    small = torch.zeros((B * (1 + 6 * nq),), dtype=torch.int32, device=dev)
    o1, o2, o3 = B, B + B * nq, B + 2 * B * nq
    out = {
        "small": small, "small_layout": (o1, o2, o3),
        "count": small[:o1],
        "keep_idx": small[o1:o2].view(B, nq),
        "scores": small[o2:o3].view(_f32).view(B, nq),
        "boxes": small[o3:].view(_f32).view(B, nq, 4),
        "ctrl": torch.zeros((B, nq, P * 2), dtype=_f32, device=dev),
        "bd": torch.zeros((B, nq, P, 4), dtype=_f32, device=dev),
        "recs": torch.zeros((B, nq, P), dtype=torch.int64, device=dev),
    }
    if frame_sizes is not None:
        assert img_h is None and img_w is None, "img_h / img_w and frame_sizes are exclusive"
        _chk_frame_desc(frame_sizes, B, (2,), _f32, "frame_sizes")
        _call("gom_detect_post_sizes", _p(cls), cls.stride(0), _p(recls), recls.stride(0) if recls is not None else 0, _p(ctrl),
              _p(bd), _p(recs), B, nq, P, _p(frame_sizes), float(det_thr), float(nms_thr), float(asso_thr), _p(out["count"]),
              _p(out["keep_idx"]), _p(out["scores"]), _p(out["boxes"]), _p(out["ctrl"]), _p(out["bd"]), _p(out["recs"]), _stream())
        return out
    _call("gom_detect_post", _p(cls), cls.stride(0), _p(recls), recls.stride(0) if recls is not None else 0, _p(ctrl), _p(bd),
          _p(recs), B, nq, P, float(img_h), float(img_w), float(det_thr), float(nms_thr), float(asso_thr), _p(out["count"]),
          _p(out["keep_idx"]), _p(out["scores"]), _p(out["boxes"]), _p(out["ctrl"]), _p(out["bd"]), _p(out["recs"]), _stream())
    return out


# ------------------------------------------------------------------------------------------ Swin glue
def gemm_gelu(A, W, bias=None):
    """GELU(A @ W^T + bias): fused into the f16x3 epilogue, a separate in-place pass on the other back-ends."""
    if isinstance(W, SplitWeight) and W.kind == "f16x3":
        return gemm(A, W, bias=bias, relu="gelu")
    return gelu_(gemm(A, W, bias=bias))


def layernorm_any(x, gamma, beta, eps=1e-5):
    _chk_f32(x, gamma, beta)
    D = x.shape[-1]
    out = torch.empty_like(x)
    _call("gom_layernorm_any_f32", _p(x), _p(gamma), _p(beta), _p(out), x.numel() // D, D, eps, _stream())
    return out


def gelu_(x):
    _chk_f32(x)
    _call("gom_gelu_f32", _p(x), x.numel(), _stream())
    return x


def swin_patchify(img):
    """[B,H,W,4] -> ([B*Hp*Wp, 64], Hp, Wp)."""
    _chk_f32(img)
    B, H, W, _ = img.shape
    Hp, Wp = (H + 3) // 4, (W + 3) // 4
    out = torch.empty((B * Hp * Wp, 64), dtype=_f32, device=img.device)
    _call("gom_swin_patchify_f32", _p(img), _p(out), B, H, W, _stream())
    return out, Hp, Wp


def swin_window_gather(x, B, H, W, shift):
    _chk_f32(x)
    C = x.shape[-1]
    Hp, Wp = (H + 6) // 7 * 7, (W + 6) // 7 * 7
    out = torch.empty((B * Hp * Wp, C), dtype=_f32, device=x.device)
    _call("gom_swin_window_gather_f32", _p(x), _p(out), B, H, W, C, shift, _stream())
    return out


def swin_window_scatter_add(windows, shortcut, B, H, W, shift):
    _chk_f32(windows, shortcut)
    C = shortcut.shape[-1]
    out = torch.empty_like(shortcut)
    _call("gom_swin_window_scatter_add_f32", _p(windows), _p(shortcut), _p(out), B, H, W, C, shift, _stream())
    return out


def swin_patch_merge(x, B, H, W):
    _chk_f32(x)
    C = x.shape[-1]
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    out = torch.empty((B * H2 * W2, 4 * C), dtype=_f32, device=x.device)
    _call("gom_swin_patch_merge_f32", _p(x), _p(out), B, H, W, C, _stream())
    return out, H2, W2


def swin_window_attention(qkv, bias, mask, windows_per_image, heads):
    _chk_f32(qkv, bias, mask)
    C = qkv.shape[1] // 3
    out = torch.empty((qkv.shape[0], C), dtype=_f32, device=qkv.device)
    _call("gom_swin_window_attention_f32", _p(qkv), _p(out), _p(bias), _p(mask), qkv.shape[0] // 49, windows_per_image, heads, C,
          _stream())
    return out


# ------------------------------------------------------------------------------------------ ViTAEv2 glue
def im2col(x, KH, KW, stride, pad, dilation, ldo):
    """[B,H,W,C] -> ([B*OH*OW, ldo], OH, OW): columns (kh, kw, c), zeros beyond KH*KW*C."""
    _chk_f32(x)
    B, H, W, C = x.shape
    OH = (H + 2 * pad - dilation * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dilation * (KW - 1) - 1) // stride + 1
    out = torch.empty((B * OH * OW, ldo), dtype=_f32, device=x.device)
    _call("gom_im2col_nhwc_f32", _p(x), _p(out), B, H, W, C, KH, KW, stride, pad, dilation, ldo, _stream())
    return out, OH, OW


def grouped_conv3x3(x, w, scale, shift, groups, stride=1, silu=False, R=None):
    """x [B,H,W,Cin], w [3,3,Cout,Cin/groups] (tap-major: a wave's lanes read contiguous weights) -> [B,OH,OW,Cout] =
    act(conv*scale + shift) + R (padding 1)."""
    _chk_f32(x, w, scale, shift, R)
    B, H, W, Cin = x.shape
    Cout = w.shape[2]
    assert w.shape == (3, 3, Cout, Cin // groups)
    y = torch.empty((B, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout), dtype=_f32, device=x.device)
    if R is not None:
        assert R.numel() == y.numel()
    _call("gom_grouped_conv3x3_nhwc_f32", _p(x), _p(w), _p(scale), _p(shift), _p(R), 3 if silu else 0, _p(y), B, H, W, Cin, Cout,
          groups, stride, _stream())
    return y


def silu_(x):
    _chk_f32(x)
    _call("gom_silu_f32", _p(x), x.numel(), _stream())
    return x


def vitae_window_gather(x, B, H, W):
    """tokens [B*H*W, C] -> window rows [B*nW*49, C] over the centred zero-padded grid."""
    _chk_f32(x)
    C = x.shape[-1]
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    out = torch.empty((B * Hp * Wp, C), dtype=_f32, device=x.device)
    _call("gom_vitae_window_gather_f32", _p(x), _p(out), B, H, W, C, _stream())
    return out


def vitae_window_crop(windows, B, H, W, R1=None, R2=None):
    """window rows -> tokens [B*H*W, C] (+ R1 + R2)."""
    _chk_f32(windows, R1, R2)
    C = windows.shape[-1]
    out = torch.empty((B * H * W, C), dtype=_f32, device=windows.device)
    _call("gom_vitae_window_crop_f32", _p(windows), _p(R1), _p(R2), _p(out), B, H, W, C, _stream())
    return out


def vitae_window_attention(qkv, heads):
    _chk_f32(qkv)
    C = qkv.shape[1] // 3
    out = torch.empty((qkv.shape[0], C), dtype=_f32, device=qkv.device)
    _call("gom_vitae_window_attention_f32", _p(qkv), _p(out), qkv.shape[0] // 49, heads, C, _stream())
    return out


def softmax_rows_scaled_(x, cols, scale):
    """In place over the first `cols` columns of a 2-D row-strided view."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == _f32
    _call("gom_softmax_rows_scaled_f32", _p(x), x.shape[0], cols, x.stride(0), float(scale), _stream())
    return x


def relu_backward(dy, y):
    _chk_f32(dy, y)
    dx = torch.empty_like(dy)
    _call("gom_relu_backward_f32", _p(dy), _p(y), _p(dx), dy.numel(), _stream())
    return dx


def softmax_rows_backward(P, dP, cols, scale):
    """dS = scale * P * (dP - rowsum(dP * P)) over the first `cols` columns of same-shape row-strided matrices."""
    assert P.shape == dP.shape and P.stride() == dP.stride() and P.stride(1) == 1
    dS = torch.zeros_like(P)
    _call("gom_softmax_rows_backward_f32", _p(P), _p(dP), _p(dS), P.shape[0], cols, P.stride(0), float(scale), _stream())
    return dS


def dropout_args(p, seed, site, iteration, rank):
    """The stream arguments every dropout entry point takes, from (p, seed, site, iteration, rank): threshold = floor(p 2^32) in
    double and scale = float(1 / (1 - p)), formed here once (include/gomatching_hip.h; the library refuses p outside [0, 1))."""
    p = float(p)
    scale = 1.0 / (1.0 - p) if p < 1.0 else float("inf")
    return (int(seed) & 0xFFFFFFFFFFFFFFFF, int(site), int(iteration), int(rank), int(math.floor(p * 4294967296.0)), scale)


def _row_view(t):
    """A 2-D row-strided fp32 view of `t` for the dropout kernels: 1-D and contiguous tensors as they are laid out."""
    assert t.dtype == _f32 and t.is_cuda
    if t.dim() != 2:
        assert t.is_contiguous()
        t = t.view(1, -1) if t.dim() < 2 else t.view(-1, t.shape[-1])
    assert t.stride(1) == 1 or t.shape[1] <= 1
    return t


def dropout(x, stream, residual=None, out=None):
    """out = [residual +] mask * scale * x with the mask of `stream` = (p, seed, site, iteration, rank) over the LOGICAL elements
    of x (row * cols + col): 2-D row-strided views of any leading dimension and alignment give the same bits.  Also the backward:
    dx = dropout(dy, same stream).  `out` may be x."""
    xv = _row_view(x)
    rows, cols = xv.shape
    if out is None:
        out = torch.empty(x.shape, dtype=_f32, device=x.device)
    ov = _row_view(out)
    rv = None if residual is None else _row_view(residual)
    assert ov.shape == xv.shape and (rv is None or rv.shape == xv.shape)
    ld = lambda t: max(t.stride(0), cols) if rows > 1 else cols
    _call("gom_dropout_f32", _p(xv), ld(xv), _p(rv), 0 if rv is None else ld(rv), _p(ov), ld(ov), rows, cols,
          *dropout_args(*stream), _stream())
    return out


def relu_backward_scaled(dy, y, scale):
    """dx = y > 0 ? dy * scale : 0 (ReLU's backward behind a dropout whose output y was saved)."""
    _chk_f32(dy, y)
    dx = torch.empty_like(dy)
    _call("gom_relu_backward_scaled_f32", _p(dy), _p(y), _p(dx), dy.numel(), float(scale), _stream())
    return dx


def softmax_dropout_rows_(x, cols, scale, stream, elem0=0):
    """In place over the first `cols` columns of a 2-D row-strided view: x <- P = softmax(scale x) (the bits of
    `softmax_rows_scaled_`); returns the dropped weights mask * scale_p * P in a tensor of x's shape whose other columns are
    zero.  Row r covers the logical elements elem0 + r cols ... of `stream` = (p, seed, site, iteration, rank)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == _f32
    pd = torch.zeros_like(x)
    assert pd.stride() == x.stride()
    _call("gom_softmax_dropout_rows_f32", _p(x), _p(pd), x.shape[0], cols, x.stride(0), float(scale), int(elem0),
          *dropout_args(*stream), _stream())
    return pd


def softmax_dropout_rows_backward(P, dPd, cols, scale, stream, elem0=0):
    """dS = scale * P * (G - rowsum(G * P)) with G = mask * scale_p * dPd, the mask of `stream` regenerated in the kernel."""
    assert P.shape == dPd.shape and P.stride() == dPd.stride() and P.stride(1) == 1
    dS = torch.zeros_like(P)
    assert dS.stride() == P.stride()
    _call("gom_softmax_dropout_rows_backward_f32", _p(P), _p(dPd), _p(dS), P.shape[0], cols, P.stride(0), float(scale), int(elem0),
          *dropout_args(*stream), _stream())
    return dS


def asso_ce(logits, frame_offsets, gt, want_loss=True, grad_scale=None):
    """Per (row, frame) cross entropy with a zero background logit (lstmatcher.py:436-475) -> loss [rows, T] and / or
    dlogits = grad_scale * (softmax - onehot); gt int32 [rows, T] (index in frame | n_t = background | -1 = not counted)."""
    _chk_f32(logits)
    R, T = gt.shape
    assert gt.dtype == torch.int32 and gt.is_contiguous() and frame_offsets.dtype == torch.int32
    loss = torch.empty((R, T), dtype=_f32, device=logits.device) if want_loss else None
    dl = torch.zeros_like(logits) if grad_scale is not None else None
    lp, dp = _p(logits), _p(dl)
    if R > 0 and logits.numel() == 0:
        # rows without a single proposal column (every frame empty): the kernel reads and writes no logit, but an empty tensor has
        # no address and the entry refuses a null pointer -- one float stands in for both
        anchor = torch.zeros((1,), dtype=_f32, device=logits.device)
        lp, dp = _p(anchor), (None if dl is None else _p(anchor))
    _call("gom_asso_ce_f32", lp, logits.shape[1] if logits.dim() == 2 else 0, _p(frame_offsets), T, _p(gt), R, _p(loss),
          _p(grad_scale), dp, _stream())
    return loss, dl


def sigmoid_focal(x, target, alpha, gamma, want_loss=True, want_grad=True):
    _chk_f32(x, target)
    loss = torch.empty_like(x) if want_loss else None
    dx = torch.empty_like(x) if want_grad else None
    _call("gom_sigmoid_focal_f32", _p(x), _p(target), float(alpha), float(gamma), x.numel(), _p(loss), _p(dx), _stream())
    return loss, dx


def clipped_adamw_step(rows, beta1, beta2, eps, clip_value, workspace=None, norm_out=None):
    """One full-model-clipped AdamW step (`gom_clipped_adamw_step`, csrc/optim.hip) over rows = [(param, grad, exp_avg,
    exp_avg_sq, step, lr, weight_decay)]: dense fp32 CUDA tensors of one size per row, `step` the count including this step.
    Updates param / exp_avg / exp_avg_sq in place, leaves grad as it is.  Returns (norm_out, workspace): norm_out = device
    [2] {total gradient norm, clip coefficient}; pass both back in to reuse them.  Launches only: nothing is read back."""
    table = (_lib_mod.OptimTensor * max(len(rows), 1))()
    for i, (p, g, m, v, step, lr, wd) in enumerate(rows):
        _chk_f32(p, g, m, v)
        if any(t.device != rows[0][0].device for t in (p, g, m, v)):
            raise ValueError("clipped_adamw_step: every tensor of the table must be on one device")
        for t in (g, m, v):
            if t.numel() != p.numel() or not t.is_contiguous():
                raise ValueError("clipped_adamw_step: param, grad and both moments must be contiguous and of one size")
        if not p.is_contiguous():
            raise ValueError("clipped_adamw_step: non-contiguous parameter")
        table[i] = _lib_mod.OptimTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), int(step), float(lr),
                                        float(wd))
    n = _L().gom_clipped_adamw_partials(table, len(rows))
    if n < 0:
        raise _lib_mod.GomError("gom_clipped_adamw_partials failed: GOM_ERR_INVALID_ARG (violated precondition)")
    dev = rows[0][0].device
    if workspace is None or workspace.numel() < n or workspace.device != dev:
        workspace = torch.empty((max(n, 1),), dtype=_f32, device=dev)
    if norm_out is None or norm_out.device != dev:
        norm_out = torch.empty((2,), dtype=_f32, device=dev)
    _call("gom_clipped_adamw_step", table, len(rows), float(beta1), float(beta2), float(eps), float(clip_value), _p(workspace),
          workspace.numel(), _p(norm_out), _stream())
    return norm_out, workspace


def transpose_into(x, out):
    """out[c, r] = x[r, c] for 2-D row-strided views (out may be wider than x has rows)."""
    assert x.dim() == 2 and out.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1
    assert out.shape[0] == x.shape[1] and out.shape[1] >= x.shape[0]
    _call("gom_transpose_f32", _p(x), _p(out), x.shape[0], x.shape[1], x.stride(0), out.stride(0), _stream())
    return out


def flash_attention(qkv, B, N, heads):
    """qkv [B*N, 3C] (q | k | v, heads contiguous inside each) -> [B*N, C]: full attention per (image, head), the score
    matrix never leaves the CU (attn_flash.hip; f16x3 products)."""
    _chk_f32(qkv)
    assert qkv.dim() == 2 and qkv.is_contiguous() and qkv.shape[0] == B * N
    C = qkv.shape[1] // 3
    out = torch.empty((B * N, C), dtype=_f32, device=qkv.device)
    f = qkv.view(-1)
    _call("gom_flash_attention_f32", _p(f), _p(f[C:]), _p(f[2 * C:]), _p(out), B, N, heads, C // heads, 3 * C, C,
          _p(range_flag(qkv.device)), _stream())
    return out


# ------------------------------------------------------------------------------------------ tracker
def gather_rows(src, rows):
    n, D = rows.numel(), src.shape[1]
    out = torch.empty((n, D), dtype=_f32, device=src.device)
    _call("gom_gather_rows_f32", _p(src), _p(rows), _p(out), n, D, _stream())
    return out


def asso_activate(logits, offsets, T, out=None):
    """logits [n_k, N], rows `logits.stride(0)` apart (a column slice of a wider buffer is fine); out: a caller's [n_k, >= N]
    buffer (rows `out.stride(0)` apart) instead of a new one."""
    n_k, N = logits.shape
    if out is None:
        out = torch.empty((n_k, N), dtype=_f32, device=logits.device)
    _call("gom_asso_activate_f32", _p(logits), _ld(logits), _p(offsets), T, n_k, _p(out), _ld(out), _stream())
    return out


def track_score(act, meta, decay, boxes, img_w, img_h, n_k, Np, M, with_iou, max_center_dist, out=None):
    traj = torch.empty((n_k, M), dtype=_f32, device=act.device) if out is None else out
    _call("gom_track_score_f32", _p(act), _ld(act), _p(meta), _p(decay), _p(boxes), float(img_w), float(img_h), n_k, Np, M,
          1 if with_iou else 0, float(max_center_dist), _p(traj), _stream())
    return traj


def asso_score(logits, offsets, T, meta, decay, boxes, img_w, img_h, n_k, Np, M, with_iou, max_center_dist, out=None):
    """asso_activate + track_score of one match as ONE launch (the form the native matcher runs for N <= 16 384): logits
    [n_k, N = Np + n_k], rows `logits.stride(0)` apart -> traj [n_k, M], the same values as the two launches."""
    traj = torch.empty((n_k, M), dtype=_f32, device=logits.device) if out is None else out
    _call("gom_asso_score_f32", _p(logits), _ld(logits), _p(offsets), T, _p(meta), _p(decay), _p(boxes), float(img_w), float(img_h),
          n_k, Np, M, 1 if with_iou else 0, float(max_center_dist), _p(traj), _stream())
    return traj


def pack_records(pool, row_base, det, frames, nq, feature_dim, num_points, image_size):
    """One launch: a step's detections (the nq-padded arrays of detect_post + their pool rows) -> [frames, nq+1, D] fp32."""
    D = feature_dim + 5 + 7 * num_points
    out = torch.empty((frames, nq + 1, D), dtype=_f32, device=pool.device)
    recs = det["recs"]
    assert recs.dtype == torch.int64 and recs.is_contiguous() and det["ctrl"].is_contiguous() and det["bd"].is_contiguous()
    _call("gom_pack_records_f32", _p(pool), pool.stride(0), int(row_base), _p(det["count"]), _p(det["boxes"]), _p(det["scores"]),
          _p(det["ctrl"]), _p(det["bd"]), _p(recs), frames, nq, feature_dim, num_points, float(image_size[0]), float(image_size[1]),
          _p(out), _stream())
    return out


BATCHED_SHORT_TERM = True  # False: per-pair kernels (kept for the A/B parity test and for > 320 detections per frame)
SHORT_TERM_MAX_PREV = 320


def short_term_pairs(tgt, memory, pairs, row_pair, boxes, img_w, img_h, with_iou, total_rows, max_prev, s_floats, out=None):
    """All pairs' S = max(softmax-with-background(q.k^T), IoU) in one launch; returns the packed fp32 buffer (`out`: a caller's)."""
    S = torch.empty((max(s_floats, 1),), dtype=_f32, device=tgt.device) if out is None else out
    _call("gom_short_term_pairs_f32", _p(tgt), _p(memory), tgt.shape[1], _p(pairs), _p(row_pair), _p(boxes), float(img_w),
          float(img_h), 1 if with_iou else 0, total_rows, max_prev, _p(S), _stream())
    return S


NATIVE_TRACKER = True      # the per-frame id recurrence of a track_frames call in native code (tracker_rt.hip); False: Python loop
NATIVE_MATCHER = True      # False: compose the match from per-kernel calls in Python (kept for the A/B parity test)


def gemm_small_rows(A, W, bias, out):
    """out = A @ W^T + bias by the tracker's small-GEMM kernel WHATEVER the number of rows (in row chunks): every output has
    the bits that kernel gives it inside a match, which is what lets per-row projections be hoisted out of the match chain."""
    assert A.dim() == 2 and A.stride(1) == 1 and W.dim() == 2 and W.stride(1) == 1 and out.stride(1) == 1
    M, K = A.shape
    N = W.shape[0]
    assert out.shape == (M, N) and K % 4 == 0
    for t_ in (A, W, bias, out):                              # row-strided views are fine (lda / ldw / ldc below)
        assert t_ is None or (t_.dtype == _f32 and t_.is_cuda)
    step = max(8, ((1 << 22) // N) // 8 * 8)
    lda, ldw, ldc = _ld(A), _ld(W), _ld(out)
    for a in range(0, M, step):
        m = min(step, M - a)
        _call("gom_gemm_small_f32", _p(A[a:]), None, lda, _p(W), ldw, None, _p(bias), None, 0, 0, _p(out[a:]), ldc, m, N, K,
              _stream())
    return out


def matcher_layers(layers):
    """layers: list of dicts {"in": (w, b), "out": (w, b), ["lin1": (w, b), "lin2": (w, b)]} of fp32 CUDA tensors ->
    ctypes array for gom_match_scores_f32 (the tensors must outlive it: the caller keeps `layers`)."""
    arr = (_lib_mod.MatcherLayer * max(len(layers), 1))()
    for i, L in enumerate(layers):
        for key in ("in", "out", "lin1", "lin2"):
            w, b = L.get(key, (None, None))
            if w is not None:
                _chk_f32(w, b)
            setattr(arr[i], key + "_w", w.data_ptr() if w is not None else None)
            setattr(arr[i], key + "_b", b.data_ptr() if b is not None else None)
    return arr


def match_scores(pool, rows, frame_offsets, meta, boxes, decay, N, T, lo, hi, num_tracks, enc, n_enc, dec, n_dec, d,
                 heads, ffn, img_w, img_h, with_iou, max_center_dist):
    """One FFI crossing for the whole device chain of a match (gom_match_scores_f32): returns traj [hi-lo, num_tracks]."""
    n_k = hi - lo
    nws = _L().gom_match_workspace_floats(N, n_k, d, ffn)
    ws = torch.empty((nws,), dtype=_f32, device=pool.device)
    traj = torch.empty((n_k, num_tracks), dtype=_f32, device=pool.device)
    _call("gom_match_scores_f32", _p(pool), pool.stride(0), _p(rows), _p(frame_offsets), _p(meta), _p(boxes), _p(decay), N, T, lo,
          hi, num_tracks, enc, n_enc, dec, n_dec, d, heads, ffn, float(img_w), float(img_h), 1 if with_iou else 0,
          float(max_center_dist), _p(ws), nws, _p(traj), _stream())
    return traj


def match_scores_proj(pool, proj, rows, frame_offsets, meta, boxes, decay, N, T, lo, hi, num_tracks, enc, n_enc, dec, n_dec, d,
                      heads, ffn, img_w, img_h, with_iou, max_center_dist):
    """The match with hoisted projections (proj [pool rows, >= 4 d]: encoder-layer-0 in-projection | decoder-layer-0 query
    projection of every pool row): the chain of 13 launches (gom_match_scores_proj_f32).  Returns traj [hi - lo, num_tracks]."""
    n_k = hi - lo
    nws = _L().gom_match_workspace_floats(N, n_k, d, ffn)
    ws = torch.empty((nws,), dtype=_f32, device=pool.device)
    traj = torch.empty((n_k, num_tracks), dtype=_f32, device=pool.device)
    _call("gom_match_scores_proj_f32", _p(pool), pool.stride(0), _p(proj), proj.stride(0), _p(rows), _p(frame_offsets), _p(meta),
          _p(boxes), _p(decay), N, T, lo, hi, num_tracks, enc, n_enc, dec, n_dec, d, heads, ffn, float(img_w), float(img_h),
          1 if with_iou else 0, float(max_center_dist), _p(ws), nws, _p(traj), _stream())
    return traj


def linear_sum_assignment(cost):
    """Host LSA with SciPy-compatible tie-breaking; cost: 2-D numpy array."""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    n = min(nr, nc)
    ri = (ctypes.c_long * max(n, 1))()
    ci = (ctypes.c_long * max(n, 1))()
    rc = _L().gom_linear_sum_assignment(cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nr, nc, ri, ci)
    if rc < 0:
        raise _lib_mod.GomError("gom_linear_sum_assignment failed (%d): cost matrix is infeasible or invalid" % rc)
    return np.asarray(ri[:rc], dtype=np.int64), np.asarray(ci[:rc], dtype=np.int64)
