/* gomatching_hip.h -- C ABI of libgomatching_hip.so: the MI355X (gfx950) GoMatching inference hot path.
 *
 * Drop-in boundary.  The reference (Hxyz-123/GoMatching) has exactly one native
 * interface on this path, the pybind module `adet._C` (third_party/adet/layers/csrc/vision.cpp:52-55); its
 * forward entry is replaced 1:1 by gom_ms_deform_attn_forward below.  Everything else on the path is
 * stock torch.nn in the reference; here those ops are hand-written HIP kernels behind the remaining entry
 * points, which the Python mirror of the reference's META_ARCH / ROI_HEADS classes
 * (gomatching_amd/modeling) binds through ctypes.  INTEGRATION.md shows the reference-side stubs.
 * Training of the association head adds gom_relu_backward_f32 ... gom_sigmoid_focal_f32 (losses and backward pieces),
 * gom_dropout_f32 ... gom_softmax_dropout_rows_backward_f32 (training-mode dropout) and gom_clipped_adamw_partials /
 * gom_clipped_adamw_step (the optimizer step), at the end of this file.
 *
 * Conventions
 *   - plain pointers and sizes only; every tensor pointer is DEVICE memory unless marked [host];
 *   - tensors are dense row-major fp32, channels-last (NHWC / token-major), 16-byte aligned;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and capture-safe
 *     (no allocation, no synchronisation) unless stated;
 *   - return value: GOM_OK, GOM_ERR_INVALID_ARG for a violated precondition (the reference raises a
 *     RuntimeError from AT_ASSERTM there, ms_deform_attn_cuda.cu:28-52), GOM_ERR_UNSUPPORTED, or
 *     GOM_ERR_HIP_BASE + hipError_t for a launch failure (the reference only printf()s those,
 *     ms_deform_im2col_cuda.cuh:948-952).
 */
#ifndef GOMATCHING_HIP_H_
#define GOMATCHING_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOM_OK 0
#define GOM_ERR_INVALID_ARG 1
#define GOM_ERR_UNSUPPORTED 2
#define GOM_ERR_HIP_BASE 1000

#define GOM_DTYPE_F32 0
#define GOM_DTYPE_F64 1

#define GOM_ABI_VERSION 1
int gom_abi_version(void);
/* gfx arch string of device 0's code object target, e.g. "gfx950" (static storage). */
const char* gom_built_for_arch(void);

/* ---- A7: multi-scale deformable attention, forward --------------------------------------------
 * Replaces at::Tensor ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc,
 * attn_weight, im2col_step)  (third_party/adet/layers/csrc/DeformAttn/ms_deform_attn.h:20-39 ->
 * ms_deform_attn_cuda.cu:20-80 -> ms_deform_im2col_cuda.cuh:237-299).
 *   value [batch, spatial_size, num_heads, channels] ; spatial_shapes [num_levels,2] (H,W) int64 ;
 *   level_start_index [num_levels] int64 ; sampling_loc [batch, num_query, heads, levels, points, 2] ;
 *   attn_weight [batch, num_query, heads, levels, points] ; output [batch, num_query, heads*channels]
 * The caller owns `output` (the reference allocates it with at::zeros; every element is written here).
 * im2col_step has no equivalent: the whole batch is one launch.  Any shape: 8 heads x 32 channels x 4 levels x 4 points
 * (every shipped config) runs the wave-per-query kernel of msda.hip, anything else the general kernel of msda_any.hip. */
int gom_ms_deform_attn_forward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* sampling_loc, const float* attn_weight, float* output, int batch,
                               int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                               int num_point, void* stream);

/* The reference's dispatch on the value dtype (AT_DISPATCH_FLOATING_TYPES, ms_deform_attn_cuda.cu:64): dtype =
 * GOM_DTYPE_F32 | GOM_DTYPE_F64 is the element type of value, sampling_loc, attn_weight and output; anything else
 * -> GOM_ERR_UNSUPPORTED (the macro throws there).  Always the general kernel. */
int gom_ms_deform_attn_forward_any(int dtype, const void* value, const int64_t* spatial_shapes,
                                   const int64_t* level_start_index, const void* sampling_loc, const void* attn_weight,
                                   void* output, int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                   int num_query, int num_point, void* stream);

/* Replaces std::vector<at::Tensor> ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc,
 * attn_weight, grad_output, im2col_step)  (ms_deform_attn.h:41-61 -> ms_deform_attn_cuda.cu:83-156 ->
 * ms_deform_im2col_cuda.cuh:301-921).  grad_output [batch, num_query, heads*channels]; the three gradients have the
 * shapes of value / sampling_loc / attn_weight, are owned by the caller and need NO zero fill (grad_value is cleared
 * in-stream here, the other two are written exactly once per element).  grad_value accumulates with hardware float
 * atomics, as the reference's does: its last bits depend on the order the waves arrive in. */
int gom_ms_deform_attn_backward(int dtype, const void* value, const int64_t* spatial_shapes,
                                const int64_t* level_start_index, const void* sampling_loc, const void* attn_weight,
                                const void* grad_output, void* grad_value, void* grad_sampling_loc, void* grad_attn_weight,
                                int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                int num_point, void* stream);

/* Same op, value read in place from a wider row-major buffer (row / batch strides in floats). */
int gom_ms_deform_attn_forward_strided(const float* value, long value_batch_stride, int value_row_stride,
                                       const int64_t* spatial_shapes, const int64_t* level_start_index,
                                       const float* sampling_loc, const float* attn_weight, float* output, int batch,
                                       int num_query, void* stream);

/* Fused MSDeformAttn core: gom_msda_prepare + gom_ms_deform_attn_forward_strided in one pass (locations and
 * weights never reach HBM).  raw/ref as for gom_msda_prepare with ref_levels = 1. */
int gom_msda_set_lane_distributed(int on);   /* [host] fused MSDA: 1 = per-sample arithmetic distributed over a head's lanes (default) */
int gom_msda_fused_forward(const float* raw, int ld_raw, const float* ref, const float* value, long value_batch_stride,
                           int value_row_stride, const int64_t* spatial_shapes, const int64_t* level_start_index,
                           float* output, int batch, int num_query, void* stream);
/* The same op for an ENCODER call (num_query = the pyramid's tokens, query q of a frame IS token q: the level-0 pixels in raster
 * order, then the coarser levels'; reference points = the tokens' own positions: deformable_transformer.py:288-300).  h0 x w0 and
 * h1 x w1 = host copies of spatial_shapes[0] and [1] (h1 = w1 = 0: no level-1 windows).  Level-0 and level-1 queries (tiles of
 * 8 x 16, one head per workgroup) are served from per-workgroup LDS windows of the value map -- the tile's projection on every level
 * + 5 pixels of halo; level-1 tiles (round 6) gather their level-0 samples from global memory instead (that window does not fit);
 * an octet group with a sample outside its window falls back to global memory -- the coarser levels' queries run on the kernel of
 * gom_msda_fused_forward.  Bit-identical to gom_msda_fused_forward.
 * [host] gom_msda_set_window(mask): bit 0 = level-0 windows, bit 1 = level-1 windows, bit 2 = the window kernel's overlapped fill
 *        schedule (the first window requested in front of the owner part, the others in pairs that share the buffer) instead of
 *        one fill at a time, bit 3 = the window kernel's four-lane layout (4 lanes per (query, head) pair, 8 channels each, DPP
 *        broadcasts inside the quad) for the forms that kept it instead of 8 lanes of 4 channels (default 15); 0 = always the
 *        gather kernel.  Same bits for every mask.
 * [host] gom_msda_window_count_fallbacks(ptr): diagnostic device word the window launches add their fallback octet groups to.
 * [host] gom_msda_window_plan: launches nothing; the windows of ONE tile as the kernel lays them out.  spatial_shapes: 4 x (H, W) in
 *        HOST memory; tile_level 0 / 1 (a tile of level-0 / level-1 queries); ref_first / ref_last: the reference points (x, y) of the
 *        tile's first and last query; schedule 0 / 1 as bit 2 above.  plan[3 * level + 0 .. 2] = first line in the workgroup's buffer,
 *        width, rows ((0, 0, 0) for a level the tile gathers from global memory); *cap_lines = the buffer's lines. */
int gom_msda_set_window(int mask);
int gom_msda_window_count_fallbacks(unsigned int* device_counter);
int gom_msda_window_plan(const int64_t* spatial_shapes, int tile_level, const float* ref_first, const float* ref_last, int schedule,
                         int* plan, int* cap_lines);
int gom_msda_fused_forward_encoder(const float* raw, int ld_raw, const float* ref, const float* value, long value_batch_stride,
                                   int value_row_stride, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                   float* output, int batch, int num_query, int h0, int w0, int h1, int w1, void* stream);

/* Sampling-location + softmax arithmetic of MSDeformAttn.forward (ms_deform_attn.py:136-145).
 * raw [Q, ld_raw]: columns [0,256) = sampling_offsets output, [256,384) = attention_weights logits;
 * ref [Q, ref_levels, 2] (ref_levels 1 = same point on every level, the unpadded case). */
int gom_msda_prepare(const float* raw, int ld_raw, const float* ref, int ref_levels, const int64_t* spatial_shapes,
                     float* sampling_loc, float* attn_weight, long num_query_total, void* stream);

/* ---- A2/A4/A6/A9/A10/A13/A14: dense contractions on fp32 MFMA -----------------------------------
 * C[M,N] = act( (A[+A2])[M,K] . W[N,K]^T * scale[N] + shift[N] + R[M,N] )
 * nn.Linear: W = weight, shift = bias, scale = NULL.  a_rows (optional) gathers rows of A (and A2).
 * K, lda, ldw multiples of 4. */
int gom_gemm_f32_set_narrow_tile(int on);   /* [host] 1 (default): N <= 32 on 128-row tiles while 256-row tiles would fill under half the CUs; same bits */
int gom_gemm_f32(const float* A, const float* A2, const int* a_rows, int lda, const float* W, int ldw,
                 const float* scale, const float* shift, const float* R, int ldr, int relu, float* C, int ldc, int M,
                 int N, int K, void* stream);

/* Same contraction for skinny problems (M <= 256; tracker / re-id head, weight-read bound): K split over
 * workgroups, partial sums reduced in slice order (deterministic) with the epilogue.  No A2. */
long gom_gemm_splitk_workspace_bytes(int M, int N, int K);
int gom_gemm_f32_splitk(const float* A, const int* a_rows, int lda, const float* W, int ldw, const float* scale,
                        const float* shift, const float* R, int ldr, int relu, float* C, int ldc, int M, int N, int K,
                        void* workspace, long workspace_bytes, void* stream);

/* Implicit-GEMM convolution, NHWC activations, OHWI weights [Cout, KH, KW, Cin], square kernel 1/3/7,
 * Cin a power of two >= 4.  Epilogue as above: FrozenBatchNorm as (scale, shift) (Detectron2
 * FrozenBatchNorm2d), conv bias as shift, bottleneck shortcut as R, ReLU.  Y [B, OH, OW, Cout]. */
int gom_conv2d_nhwc_f32(const float* X, const float* Wt, const float* scale, const float* shift, const float* R,
                        int relu, float* Y, int B, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride,
                        int pad, void* stream);

/* Tiny products (tracker association logits tgt . memory^T, transformer.py:92-96; at most 2^22 outputs): one wave per
 * output element on the VALU, K % 4 == 0, same epilogue as gom_gemm_f32 (no A2).  Deterministic. */
int gom_gemm_small_f32(const float* A, const int* a_rows, int lda, const float* W, int ldw, const float* scale,
                       const float* shift, const float* R, int ldr, int relu, float* C, int ldc, int M, int N, int K,
                       void* stream);

/* fp32-accurate variants on the bf16 matrix cores ("bf16x6": operands split into three bf16 planes, six MFMA
 * products of weight <= 2; error ~ one fp32 rounding per product; 2.67x the fp32 matrix rate).
 * The weight operand is pre-split once: planes_out [3][N][Kpad] bf16, Kpad a multiple of 32 (zero padded).
 * No second A operand; the residual R applies to columns < r_cols only (lets one launch serve fused heads). */
int gom_split_bf16x3(const float* W, int ldw, int N, int K, void* planes_out, int Kpad, void* stream);
int gom_gemm_f32_bf16x6(const float* A, const int* a_rows, int lda, const void* Wplanes, long w_plane_stride, int ldw,
                        const float* scale, const float* shift, const float* R, int ldr, int r_cols, int relu, float* C,
                        int ldc, int M, int N, int K, void* stream);
int gom_conv2d_nhwc_f32_bf16x6(const float* X, const void* Wplanes, long w_plane_stride, int ldw, const float* scale,
                               const float* shift, const float* R, int relu, float* Y, int B, int H, int Wd, int Cin,
                               int Cout, int KH, int KW, int stride, int pad, void* stream);

/* "f16x3": the same products on the fp16 matrix cores from TWO fp16 planes per operand and three MFMA passes
 * (a0b0 + a0b1 + a1b0; 22 significand bits, relative error ~7e-7 per product, half the MFMA work of bf16x6).
 * Weights: gom_split_f16x2 scales each row by a power of two into fp16's upper normal range before the split and returns
 * the inverse scales (`wscale`, applied to the accumulator).  Activations are split unscaled: |a| <= 65504, absolute
 * accuracy 3e-8 below ~0.25; a non-finite result sets *flag (device int, may be NULL) -- checked by the host once per
 * step.  Otherwise the arguments of the bf16x6 entry points; `splits` / workspace as gom_conv2d_nhwc_f32_bf16x6_splitk. */
int gom_split_f16x2(const float* W, int ldw, int N, int K, void* planes_out, int Kpad, float* inv_scale, void* stream);
int gom_gemm_f32_f16x3(const float* A, const int* a_rows, int lda, const void* Wplanes, long w_plane_stride, int ldw,
                       const float* wscale, const float* scale, const float* shift, const float* R, int ldr, int r_cols,
                       int relu, float* C, int ldc, int M, int N, int K, int* flag, void* stream);
/* ... with a PERIODIC residual: row m adds R[m % r_period] (r_period = 0: R[m]).  The encoder's position term
 * (src + pos) W^T = src W^T + (pos W^T) is such a table -- S rows shared by the frames of a step (57 MB instead of 457 MB
 * per layer call at 8 frames of 1000x1778). */
int gom_gemm_f32_f16x3_rp(const float* A, const int* a_rows, int lda, const void* Wplanes, long w_plane_stride, int ldw,
                          const float* wscale, const float* scale, const float* shift, const float* R, int ldr, int r_cols,
                          int r_period, int relu, float* C, int ldc, int M, int N, int K, int* flag, void* stream);
int gom_conv2d_nhwc_f32_f16x3(const float* X, const void* Wplanes, long w_plane_stride, int ldw, const float* wscale,
                              const float* scale, const float* shift, const float* R, int relu, float* Y, int B, int H,
                              int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                              long workspace_bytes, int splits, int* flag, void* stream);
/* 3x3 / stride 1 / pad 1 convolution with the input patch resident in LDS (csrc/conv3x3_patch.hip): the bottleneck blocks'
 * conv2 (Detectron2 BottleneckBlock behind gom_lstmatcher.py:42-61).  Cin and Cout multiples of 64
 * (gom_conv3x3_patch_supported).  gom_conv3x3_patch_image: one-time fragment-linear image of the gom_split_f16x2 planes of
 * W [Cout, 3, 3, Cin] (gom_conv3x3_patch_image_bytes bytes; -1 = shape not served); wscale = the split's inverse row scales.
 * fp32-class like the implicit-GEMM kernel (k order: 64-channel chunk, tap, channel; 32-wide k-steps): not its bits. */
int gom_conv3x3_patch_supported(int Cin, int Cout);
long gom_conv3x3_patch_image_bytes(int Cin, int Cout);
int gom_conv3x3_patch_image(const void* w_planes, long w_plane_stride, int ldw, int Cin, int Cout, void* image, long image_bytes,
                            void* stream);
int gom_conv3x3_patch_f32_f16x3(const float* X, const void* image, const float* wscale, const float* scale, const float* shift,
                                int relu, float* Y, int B, int H, int Wd, int Cin, int Cout, int* flag, void* stream);
/* The ResNet stem as one launch (csrc/stem_pool.hip): conv 7x7 / stride 2 / pad 3 from the 4-channel NHWC input to 64 channels
 * (weights = the gom_split_f16x2 planes of the [64, 7*7*4] matrix, K padded to ldw) + per-channel scale / shift (folded
 * BatchNorm, may be NULL) + ReLU + max_pool2d(3, stride 2, pad 1): Y [B, PH, PW, 64], PH = ((H - 1) / 2) / 2 + 1 likewise PW
 * (detectron2 BasicStem: modeling/backbone/resnet.py as built by adet's build_resnet_backbone).  Equal bit
 * for bit to gom_conv2d_nhwc_f32_f16x3 followed by gom_maxpool3x3s2_nhwc_f32, same range contract and *flag. */
int gom_stem_conv_pool_f32(const float* X, const void* Wplanes, long w_plane_stride, int ldw, const float* wscale,
                           const float* scale, const float* shift, float* Y, int B, int H, int Wd, int* flag, void* stream);

/* Output projection + residual + LayerNorm of an attention block in ONE launch (csrc/proj_ln.hip):
 *     Y = LayerNorm(X W^T + b + R) * gamma + beta,   X, R, Y [M, 256] fp32 (row strides ldx / ldr / ldy; Y may alias R), W [256, 256]
 * = `norm1(src + out_proj(...))` of an encoder layer and the three `norm_*(tgt + out_proj(...))` of a decoder layer
 * (deformable_transformer.py:258-264, 386-422): 3 KB of HBM traffic per token instead of the 5 KB of GEMM + LayerNorm.  f16x3
 * scheme, range contract and *flag of gom_gemm_f32_f16x3 (fp32-class agreement with it, k-steps of 32).  gom_proj_ln_image:
 * one-time weight preparation from the gom_split_f16x2 planes (gom_proj_ln_image_bytes bytes; -1 = shape not served);
 * w_inv_scale = the split's inverse row scales, bias may be NULL. */
long gom_proj_ln_image_bytes(int n, int k);
int gom_proj_ln_image(const void* w_planes, long w_plane_stride, int ldw, int n, int k, void* image, long image_bytes,
                      void* stream);
int gom_proj_ln_f32(const float* X, int ldx, const void* image, const float* w_inv_scale, const float* bias, const float* R,
                    int ldr, const float* gamma, const float* beta, float eps, float* Y, int ldy, int M, int* flag,
                    void* stream);
/* R may be NULL in gom_proj_ln_f32 (Y = LayerNorm(X W^T + b): enc_output + enc_output_norm, deformable_transformer.py:171-172).
 * Dot form: out[m] = <LayerNorm(X[m] W^T + b) * gamma + beta, dot_w[256]> + dot_b -- the proposal class logit of every encoder
 * token (:171-175) with the normalised rows never stored; the winners' rows are recomputed by gom_proj_ln_f32 on the gathered
 * rows (row-independent arithmetic: the same bits). */
int gom_proj_ln_dot_f32(const float* X, int ldx, const void* image, const float* w_inv_scale, const float* bias,
                        const float* gamma, const float* beta, float eps, const float* dot_w, float dot_b, float* out, int M,
                        int* flag, void* stream);

/* Tail of a ResNet bottleneck block fused with the head of the next (csrc/bneck_fused.hip; Detectron2 BottleneckBlock as built
 * through gom_lstmatcher.py:42-61, STRIDE_IN_1X1 = False, FrozenBN folded):
 *     X  = relu(scale3 * (A W3^T) + shift3 + R)       A [M, k1] conv2's output, R / X [M, c4 = 4 k1] (X must not alias R)
 *     Y1 = relu(scale1 * (X W1^T) + shift1)           [M, mp]: the next block's conv1
 * X is written once and never read back.  Served (k1, mp): (64, 64 | 128), (128, 128 | 256); gom_bneck_image_bytes
 * returns -1 otherwise.  gom_bneck_image: one-time weight preparation from the gom_split_f16x2 planes of conv3's [c4, k1] and the
 * next conv1's [mp, c4] matrices; scale3 / shift3 = conv3's folded BatchNorm (its weight row scales are folded in here), scale1
 * must already hold conv1's folded BatchNorm scale TIMES its weight's inverse row scales.  f16x3 scheme, range contract and *flag
 * of gom_gemm_f32_f16x3; X equals that kernel's conv3 output up to the ReLU'd last bit, Y1 to summation order. */
long gom_bneck_image_bytes(int k1, int c4, int mp);
int gom_bneck_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
                    const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1, int k1, int c4, int mp, void* image,
                    long image_bytes, void* stream);
int gom_bneck_f32(const float* A, int lda, const void* image, const float* R, int ldr, const float* scale1, const float* shift1,
                  float* X, int ldx, float* Y1, int ldy, int M, int k1, int c4, int mp, int* flag, void* stream);
/* Shortcut form, for the FIRST block of a stage: the residual is the block's 1x1 projection shortcut, computed inside the launch
 * from the block's input instead of being read ([M, c4] written by one launch to be read by the next, gone):
 *     R  = fl32(scale_s * (S Wsc^T) + shift_s)        S [B, Hs, Ws, ks] NHWC (pixel stride lds floats), sampled at (b, stride y, stride x)
 *     X  = relu((scale3 * (A W3^T) + shift3) + R),  Y1 as above;   A / X / Y1 have B x OH x OW rows, OH = (Hs - 1) / stride + 1
 * i.e. the arithmetic of the shortcut's own launch followed by gom_bneck_f32's.  S is split into fp16 planes like A (range contract,
 * *flag).  Served (k1, c4, mp, ks, stride): (64, 256, 64, 64, 1) = res2.0; gom_bneck_sc_image_bytes returns -1 otherwise.
 * gom_bneck_sc_image: gom_bneck_image's arguments plus the gom_split_f16x2 planes of the shortcut's [c4, ks] matrix, its inverse
 * row scales and its folded BatchNorm. */
long gom_bneck_sc_image_bytes(int k1, int c4, int mp, int ks, int stride);
int gom_bneck_sc_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
                       const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1, const void* ws_planes,
                       long ws_plane_stride, int lds, const float* ws_inv_scale, const float* scale_s, const float* shift_s, int k1,
                       int c4, int mp, int ks, int stride, void* image, long image_bytes, void* stream);
int gom_bneck_sc_f32(const float* A, int lda, const void* image, const float* S, int lds, int B, int Hs, int Ws, int stride,
                     const float* scale1, const float* shift1, float* X, int ldx, float* Y1, int ldy, int k1, int c4, int mp, int ks,
                     int* flag, void* stream);
/* The same pair for the wide shapes (res4: k1 = 256, c4 = 1024, mp = 256; the res3 -> res4 transition: 128, 512, 256) on
 * csrc/bneck2.hip: 16-pixel waves on the 16x16x32 MFMA shape, eight per workgroup (two per SIMD) sharing one weight ring.
 * gom_bneck2_image / gom_bneck2_f32: arguments as gom_bneck_image / gom_bneck_f32 (gom_bneck2_image_bytes: -1 = shape not served). */
long gom_bneck2_image_bytes(int k1, int c4, int mp);
int gom_bneck2_image(const void* w3_planes, long w3_plane_stride, int ld3, const float* w3_inv_scale, const float* scale3,
                     const float* shift3, const void* w1_planes, long w1_plane_stride, int ld1, int k1, int c4, int mp, void* image,
                     long image_bytes, void* stream);
int gom_bneck2_f32(const float* A, int lda, const void* image, const float* R, int ldr, const float* scale1, const float* shift1,
                   float* X, int ldx, float* Y1, int ldy, int M, int k1, int c4, int mp, int* flag, void* stream);

/* The two self-attention blocks of a DeepSolo composite decoder layer, each as ONE launch (csrc/dec_attn.hip), replacing
 * nn.MultiheadAttention + residual + LayerNorm of deformable_transformer.py:386-394 (inter = 0: attention over the
 * `group_tokens` <= 32 points of a query, q = k = X + P, v = X; rows of a group are consecutive) and :396-404 (inter = 1:
 * attention over the `group_tokens` <= 128 queries of one (frame, point), q = k = v = X, P = NULL; token t of group g is row
 * ((g / inner) * group_tokens + t) * inner + g % inner, inner = points per query):
 *     Y = LayerNorm(X + out_proj(MHA_8x32(...))) * gamma + beta,   X, P, Y [rows, 256] fp32; Y must not alias X.
 * f16x3 scheme, range contract and *flag of gom_gemm_f32_f16x3 (q, k, v, the inputs and the probabilities are split into two
 * fp16 planes; fp32 accumulation and softmax).  gom_dec_attn_image: one-time weight preparation from the gom_split_f16x2
 * planes of in_proj_weight [768, 256] (+ inverse row scales, in_proj_bias) and out_proj.weight [256, 256] (+ inverse row
 * scales, bias) and the LayerNorm's gamma / beta [256]. */
long gom_dec_attn_image_bytes(int d_model, int heads);
int gom_dec_attn_image(const void* in_planes, long in_plane_stride, int ld_in, const float* in_inv_scale, const float* in_bias,
                       const void* out_planes, long out_plane_stride, int ld_out, const float* out_inv_scale,
                       const float* out_bias, const float* gamma, const float* beta, int inter, void* image, long image_bytes,
                       void* stream);
int gom_dec_attn_f32(const float* X, int ldx, const float* P, int ldp, const void* image, float eps, float* Y, int ldy, int groups,
                     int group_tokens, int inner, int inter, int* flag, void* stream);
/* The inter-instance block (inter = 1) followed, in the same launch, by the cross attention's sampling_offsets | attention_weights
 * product on its output (deformable_transformer.py:396-404, then ms_deform_attn.py:117-131 on query = tgt + query_pos):
 *     raw [rows, 384] = (Y + P2) Wraw^T + braw        P2 = query_pos [rows, 256]
 * `image`: gom_dec_attn_raw_image_bytes() bytes, filled by gom_dec_attn_image (inter = 1) and then gom_dec_attn_raw_image (the
 * gom_split_f16x2 planes of the [384, 256] weight, its inverse row scales and bias).  group_tokens <= 128. */
long gom_dec_attn_raw_image_bytes(void);
int gom_dec_attn_raw_image(const void* raw_planes, long raw_plane_stride, int ld_raw, const float* raw_inv_scale,
                           const float* raw_bias, void* image, long image_bytes, void* stream);
int gom_dec_attn_raw_f32(const float* X, int ldx, const void* image, float eps, float* Y, int ldy, const float* P2, int ldp2,
                         float* raw, int ldraw, int groups, int group_tokens, int inner, int* flag, void* stream);

/* The same two blocks and the same contract on 16-token waves, two per SIMD (csrc/dec_attn2.hip, round 6): eight waves per workgroup
 * on v_mfma_f32_16x16x32_f16 sharing one weight ring, an attention group spread over a pair of waves (inter = 0) or all eight
 * (inter = 1) that exchange a head's K / V fragments through LDS.  Arguments as the gom_dec_attn_* entry of the same name; the images
 * differ (16x16x32 fragment order, the epilogue vectors in front) and are NOT interchangeable with gom_dec_attn_image's. */
long gom_dec_attn2_image_bytes(int d_model, int heads);
int gom_dec_attn2_image(const void* in_planes, long in_plane_stride, int ld_in, const float* in_inv_scale, const float* in_bias,
                        const void* out_planes, long out_plane_stride, int ld_out, const float* out_inv_scale,
                        const float* out_bias, const float* gamma, const float* beta, int inter, void* image, long image_bytes,
                        void* stream);
int gom_dec_attn2_f32(const float* X, int ldx, const float* P, int ldp, const void* image, float eps, float* Y, int ldy, int groups,
                      int group_tokens, int inner, int inter, int* flag, void* stream);
long gom_dec_attn2_raw_image_bytes(void);
int gom_dec_attn2_raw_image(const void* raw_planes, long raw_plane_stride, int ld_raw, const float* raw_inv_scale,
                            const float* raw_bias, void* image, long image_bytes, void* stream);
int gom_dec_attn2_raw_f32(const float* X, int ldx, const void* image, float eps, float* Y, int ldy, const float* P2, int ldp2,
                          float* raw, int ldraw, int groups, int group_tokens, int inner, int* flag, void* stream);

/* The inter-instance attention (deformable_transformer.py:396-404) for MORE than 128 queries per frame (GoMatching_PP_DSText.yaml:
 * 300), csrc/dec_inter.hip: in_proj + the 8 x 32 attention core, one workgroup per (group, head) with the head's K / V^T of all
 * `group_tokens` <= 352 tokens in LDS and an online softmax over the key blocks:
 *     O[token, 32 h .. 32 h + 31] = softmax(q_h k_h^T / sqrt(32)) v_h,    q | k | v = X . in_proj_weight^T + in_proj_bias
 * X, O [rows, 256] fp32 (token t of group g is row ((g / inner) * group_tokens + t) * inner + g % inner); `image` = the
 * gom_dec_attn_image of the block with inter = 1 (its in_proj stages are read).  out_proj + residual + LayerNorm follow as one
 * gom_proj_ln_f32 launch.  Same f16x3 scheme, range contract and *flag as gom_dec_attn_f32. */
int gom_dec_inter_heads_f32(const float* X, int ldx, const void* image, float* O, int ldo, int groups, int group_tokens,
                            int inner, int* flag, void* stream);

/* Row-resident K = 256 form of gom_gemm_f32_f16x3 for SHORT problems (the decoder's Q-side nn.Linear layers at
 * M = frames x queries x points rows: deformable_transformer.py:386-422,470-488), csrc/gemm_k256.hip:
 *     C[M, N] = act( (A [+ A2])[M, 256] . W[N, 256]^T + bias [+ R on columns < r_cols] ),   N, r_cols multiples of 32.
 * Same split scheme, plane-product order and epilogue arithmetic as gom_gemm_f32_f16x3: bit-identical results, same range
 * contract and *flag.  gom_gemm_k256_image: one-time weight preparation from the gom_split_f16x2 planes, their inverse row
 * scales and the bias (may be NULL) into the kernel's fragment-linear stream (gom_gemm_k256_image_bytes bytes; -1 = shape
 * not served).  col_groups: workgroups along N (0 = chosen from M: about two workgroups per CU). */
long gom_gemm_k256_image_bytes(int N, int K);
int gom_gemm_k256_image(const void* w_planes, long w_plane_stride, int ldw, const float* w_inv_scale, const float* bias,
                        int N, int K, void* image, long image_bytes, void* stream);
int gom_gemm_k256_f32(const float* A, const float* A2, int lda, const void* image, const float* R, int ldr, int r_cols,
                      int relu, float* C, int ldc, int M, int N, int K, int col_groups, int* flag, void* stream);
/* ... with a PERIODIC residual: r_period > 0 -> row m reads R[m % r_period] (the encoder's position-embedding table, one copy
 * per frame: deformable_transformer.py:235-248 with_pos_embed folded into the projection); r_period >= 32, table < 4 GB.
 * gom_gemm_k256_f32 = r_period 0.  Long problems (>= 512 row tiles) run the kernel's whole-line-store form, short ones its
 * 16-byte-store form -- the same bits; gom_gemm_k256_set_lines(0 / 1) forces one (tests, tools), -1 = by M. */
int gom_gemm_k256_rp_f32(const float* A, const float* A2, int lda, const void* image, const float* R, int ldr, int r_cols,
                         int r_period, int relu, float* C, int ldc, int M, int N, int K, int col_groups, int* flag,
                         void* stream);
void gom_gemm_k256_set_lines(int mode);
/* Periodic residual, several periods (frames), long problem: workgroups take the row tiles frame-interleaved per XCD, so that the
 * table rows of a position are fetched into an XCD's L2 once for all frames (1 = on, 0 = index order = default: the interleave
 * measured 3 % slower, the re-reads hit the Infinity Cache; same bits). */
void gom_gemm_k256_set_interleave(int on);
/* Row-list form: C[rows[i]] = A[rows[i]] . W^T + bias for i < *count (rows, count: device memory; rows of [0, M)), every other row
 * of C untouched; per listed row the bits of gom_gemm_k256_f32.  The grid is the dense problem's (M = the list's capacity), so a
 * captured launch serves any count.  clear (may be NULL): byte clear[rows[i]] = 0 for every listed row. */
int gom_gemm_k256_rows_f32(const float* A, int lda, const void* image, const int* rows, const int* count, unsigned char* clear,
                           float* C, int ldc, int M, int N, int K, int* flag, void* stream);

/* The rows of the encoder memory that a decoder layer's fused MSDA call LOADS (csrc/dec_value_rows.hip; raw, ref, shapes and level
 * starts as for gom_msda_fused_forward, whose gather kernel shares the corner arithmetic): gom_dec_value_mark sets the byte
 * flags[frame * rows_per_frame + row] = 1 for every such row, weight-0 loads included; gom_dec_value_compact turns flags[0, n) into
 * the ascending list rows[0, *count) (rows: n ints).  flags: gom_dec_value_flag_bytes(n) bytes (n rounded up to the compaction's
 * tile), zero where nothing is marked; the marks stay set until gom_gemm_k256_rows_f32 (clear = flags) or the caller clears them.
 * No atomics, deterministic. */
int gom_dec_value_set_lean_mark(int on);   /* [host] 1 (default): gom_dec_value_mark reads a flag before it stores it; same bytes */
long gom_dec_value_flag_bytes(int n);
int gom_dec_value_mark(const float* raw, int ld_raw, const float* ref, const int64_t* spatial_shapes,
                       const int64_t* level_start_index, int batch, int num_query, int rows_per_frame, unsigned char* flags,
                       void* stream);
int gom_dec_value_compact(const unsigned char* flags, int n, int* rows, int* count, void* stream);

/* Fused FFN block of a DeepSolo transformer layer (deformable_transformer.py:250-251,266-273 encoder linear1/ReLU/linear2 +
 * residual + norm2; :352-354,368-369 decoder + norm3):
 *     Y = LayerNorm(X + relu(X W1^T + b1) W2^T + b2) * gamma + beta,   X, Y [M, d_model] fp32 (row strides ldx / ldy; Y may
 * alias X), d_model = 256, d_hidden a multiple of 32, on the f16x3 scheme of gom_gemm_f32_f16x3 (same accuracy and range
 * contract, same *flag).  The hidden activations never leave the CU (csrc/ffn_fused.hip).
 * gom_ffn_fused_image: one-time weight preparation -- the two gom_split_f16x2 plane sets (W1 [d_hidden, d_model] with its
 * inverse row scales, W2 [d_model, d_hidden]) and b1 re-ordered into the kernel's fragment-linear stream
 * (gom_ffn_fused_image_bytes bytes; -1 = shape not served).  gom_ffn_fused_ln_f32 additionally takes W2's inverse row
 * scales and b2. */
long gom_ffn_fused_image_bytes(int d_model, int d_hidden);
int gom_ffn_fused_image(const void* w1_planes, long w1_plane_stride, int ld1, const float* w1_inv_scale, const float* b1,
                        const void* w2_planes, long w2_plane_stride, int ld2, int d_model, int d_hidden, void* image,
                        long image_bytes, void* stream);
int gom_ffn_set_stream_cus(int cus); /* [host] compute units of the (CU-masked) stream the fused FFN is launched on; 0 = whole device */
int gom_ffn_set_half_tail(int on);   /* [host] 1 (default): the partly filled last round of a long launch as half-height (64-row) tiles; same bits */
int gom_ffn_fused_ln_f32(const float* X, int ldx, const void* image, const float* w2_inv_scale, const float* b2,
                         const float* gamma, const float* beta, float eps, float* Y, int ldy, int M, int d_model,
                         int d_hidden, int* flag, void* stream);

/* The same kernel as a plain two-layer perceptron, Y = [relu](relu(X W1^T + b1) W2^T + b2), X / Y [M, 256] (csrc/ffn_fused.hip,
 * PLAIN form): the decoder's ref_point_head (deformable_transformer.py:470-473) and the first two layers of the three-layer
 * coordinate / boundary heads (:484-488, detection_transformer_wobackbone.py:238-253).  `image` = gom_ffn_fused_image. */
int gom_mlp2_fused_f32(const float* X, int ldx, const void* image, const float* w2_inv_scale, const float* b2, int relu_out,
                       float* Y, int ldy, int M, int d_model, int d_hidden, int* flag, void* stream);

/* The row-local TAIL of a composite decoder layer as one launch (csrc/dec_tail.hip; deformable_transformer.py:352-354,368-369
 * FFN + norm3, :484-488 ctrl_point_coord MLP + reference refinement, :470-473 the NEXT layer's ref_point_head over the sine
 * embedding of the refined points):
 *     Y       = LayerNorm(X + relu(X W1^T + b1) W2^T + b2) * gamma + beta
 *     new_ref = sigmoid(W3 relu(Wc2 relu(Wc1 Y + bc1) + bc2) + b3 + inverse_sigmoid(ref))           [M, 2]
 *     qpos    = Wq2 relu(Wq1 point_pos_embed(new_ref) + bq1) + bq2                                   [M, 256]; qpos == NULL: skipped
 * `image` = gom_ffn_fused_image(FFN) | gom_ffn_fused_image_acc_order(ctrl_point_coord layers 1-2) [| gom_ffn_fused_image_acc_order(
 * ref_point_head)], concatenated (gom_dec_tail_image_bytes).  *_inv_scale / *_b2: the inverse row scales and bias of each block's
 * SECOND weight.  Same f16x3 accuracy / range contract and *flag as gom_ffn_fused_ln_f32. */
long gom_dec_tail_image_bytes(int d_model, int d_hidden, int with_qpos);
int gom_ffn_fused_image_acc_order(const void* w1_planes, long w1_plane_stride, int ld1, const float* w1_inv_scale, const float* b1,
                                  const void* w2_planes, long w2_plane_stride, int ld2, int d_model, int d_hidden, void* image,
                                  long image_bytes, void* stream);
int gom_dec_tail_f32(const float* X, int ldx, const void* image, int d_hidden, const float* w2_inv_scale, const float* b2,
                     const float* gamma, const float* beta, float eps, const float* c_inv_scale, const float* c_b2,
                     const float* W3, const float* b3, const float* ref, const float* dim_t128, const float* q_inv_scale,
                     const float* q_b2, float* Y, int ldy, float* new_ref, float* qpos, int ldq, int M, int* flag, void* stream);
/* ... with the cross-attention's out_proj + residual + norm_cross in front (deformable_transformer.py:406-422):
 *     tgt3 = LayerNorm(R + S Wo^T + bo) * p_gamma + p_beta     S = the rows sampled by the fused MSDA op, R = tgt in front of the block
 * then the chain above on tgt3.  `image` = gom_dec_tail_lin_image(out_proj planes) | gom_ffn_fused_image_acc_order x 3 (the FFN's
 * input now arrives in accumulator order too).  Y must not alias S or R (it holds tgt3 while the FFN runs). */
long gom_dec_tail_lin_image_bytes(void);
int gom_dec_tail_lin_image(const void* w_planes, long w_plane_stride, int ld, void* image, long image_bytes, void* stream);
int gom_dec_tail_proj_f32(const float* S, int lds, const float* R, int ldr, const void* image, int d_hidden,
                          const float* p_inv_scale, const float* p_bias, const float* p_gamma, const float* p_beta, float p_eps,
                          const float* w2_inv_scale, const float* b2, const float* gamma, const float* beta, float eps,
                          const float* c_inv_scale, const float* c_b2, const float* W3, const float* b3, const float* ref,
                          const float* dim_t128, const float* q_inv_scale, const float* q_b2, float* Y, int ldy, float* new_ref,
                          float* qpos, int ldq, int M, int* flag, void* stream);

/* The same tail as a CU-COOPERATIVE launch (csrc/dec_tail2.hip, round 6): a workgroup's four waves share 80 rows (held in LDS as
 * MFMA operand fragments) and split the output columns; every wave streams its quarter of the weights straight from L2.  At the
 * decoder's M = 20 000 rows: 250 workgroups = one round of the chip (gom_dec_tail_*: 157 workgroups, two row groups on the busiest
 * SIMD).  `image` = `waves` per-wave streams of `wave_bytes` each (gom_dec_tail2_wave_bytes), filled block by block at `offset_bytes`
 * inside every stream: [gom_dec_tail2_image_lin(out_proj)] | gom_dec_tail2_image_mlp(FFN) | ..._mlp(ctrl_point_coord layers 1-2) |
 * [..._mlp(ref_point_head)].  S / R / p_*: R == NULL = no out_proj block (S is then tgt behind norm_cross); qpos == NULL = the last
 * layer (image without ref_point_head's part).  *_inv1 / *_b1, *_inv2 / *_b2: inverse row scales (gom_split_f16x2) and biases of each
 * block's first / second weight.  Same f16x3 accuracy / range contract and *flag as gom_dec_tail_f32; the LayerNorm statistics are
 * combined from per-wave (mean, M2) pairs (Chan), so results agree with gom_dec_tail_* to rounding, not bit for bit.
 * `waves` = 4 (one wave per SIMD; a wave owns 64 output columns) or 8 (two per SIMD, 32 columns each: one wave's epilogues and
 * activation phases under the other's MFMAs); the image is `waves` streams and belongs to the `waves` it was built for. */
long gom_dec_tail2_wave_bytes(int d_model, int d_hidden, int with_proj, int with_qpos, int waves);
int gom_dec_tail2_image_lin(const void* w_planes, long w_plane_stride, int ld, void* image, long wave_bytes, long offset_bytes,
                            int waves, void* stream);
int gom_dec_tail2_image_mlp(const void* w1_planes, long w1_plane_stride, int ld1, const void* w2_planes, long w2_plane_stride, int ld2,
                            int d_hidden, void* image, long wave_bytes, long offset_bytes, int waves, void* stream);
int gom_dec_tail2_f32(const float* S, int lds, const float* R, int ldr, const void* image, long wave_bytes, int d_hidden,
                      const float* p_inv_scale, const float* p_bias, const float* p_gamma, const float* p_beta, float p_eps,
                      const float* w1_inv_scale, const float* b1, const float* w2_inv_scale, const float* b2, const float* gamma,
                      const float* beta, float eps, const float* c_inv1, const float* c_b1, const float* c_inv2, const float* c_b2,
                      const float* W3, const float* b3, const float* ref, const float* dim_t128, const float* q_inv1,
                      const float* q_b1, const float* q_inv2, const float* q_b2, float* Y, int ldy, float* new_ref, float* qpos,
                      int ldq, int M, int waves, int* flag, void* stream);

/* Split-K form for convolutions with few output tiles and a long K (input_proj[3]: 3x3 s2 2048 -> 256 on res5, M = 3584,
 * K = 18432): `splits` K-slices run as separate workgroups into workspace [splits][M][Cout] fp32, a second kernel sums
 * them in slice order (deterministic) and applies the epilogue.  gom_conv_bf16x6_splits: recommended slice count, 0 =
 * do not split. */
int gom_conv_bf16x6_splits(int M, int N, int K);
int gom_conv2d_nhwc_f32_bf16x6_splitk(const float* X, const void* Wplanes, long w_plane_stride, int ldw,
                                      const float* scale, const float* shift, const float* R, int relu, float* Y, int B,
                                      int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                      void* workspace, long workspace_bytes, int splits, void* stream);

/* ---- normalisation ---------------------------------------------------------------------------------*/
/* out = LayerNorm(x + residual) * gamma + beta over rows of dim 256 or 1024 (residual may be NULL). */
int gom_layernorm_f32(const float* x, const float* residual, const float* gamma, const float* beta, float* out,
                      long rows, int dim, float eps, void* stream);
/* GroupNorm(32, 256) over [B, HW, 256]; writes out[b*out_batch_stride + r*256 + c] (lets the caller scatter a
 * level straight into the flattened multi-level token buffer).  stats_ws: B*64 doubles of scratch. */
int gom_groupnorm32_nhwc_f32(const float* x, const float* gamma, const float* beta, double* stats_ws, float* out,
                             long out_batch_stride, int B, int HW, int channels, float eps, void* stream);

/* ---- attention core: O = softmax(Q K^T / sqrt(head_dim)) V per (batch, head) -------------------------
 * batch = batch_outer x batch_inner.  Element (bo, bi, i, h, d) of q lives at
 * q[bo*S[0] + bi*S[1] + i*S[2] + h*head_dim + d]; strides [host] S[12] = q(bo,bi,seq) k(..) v(..) o(..).
 * head_dim 32 (DeepSolo decoder, deformable_transformer.py:388-402) or 128 (matcher, transformer.py:208,287). */
int gom_mha_core_f32(const float* q, const float* k, const float* v, float* o, int batch_outer, int batch_inner,
                     int heads, int head_dim, int Lq, int Lk, const long* strides, void* stream);

/* Ragged batch of independent attention problems over row ranges of shared q / k / v / o matrices (every frame pair
 * of the short-term matcher at once).  segments [device] int32 [S][4] = (first query row, Lq, first key row, Lk);
 * ld_* row strides in floats; head_dim 128. */
int gom_mha_core_segments_f32(const float* q, const float* k, const float* v, float* o, const int* segments,
                              int num_segments, int heads, int head_dim, int ld_q, int ld_k, int ld_v, int ld_o, int max_Lq,
                              int max_Lk, void* stream);

/* ---- glue (A1, A2 stem pool, A3, A5, A8, A9) ----------------------------------------------------------*/
/* mean3/std3 are [host] arrays.  images [B,3,H,W] -> out [B,H,W,4] (4th channel 0). */
int gom_preprocess_nchw_to_nhwc4(const float* images, const float* mean3, const float* std3, float* out, int B, int H,
                                 int W, void* stream);
/* ---- f2: frame ingest (text_track_visualizer.py:315-324 + gom_lstmatcher.py:159-170) -----------------------
 * Replaces the host-side `aug.get_transform(frame).apply_image(frame)` (Detectron2 ResizeShortestEdge ->
 * Pillow Image.resize(BILINEAR) on uint8), the BGR->RGB flip (:316-318), `astype("float32")` (:321) and
 * the model's normaliser for uint8 frames resident in HBM.  Bit-exact with Pillow's fixed-point resampler.
 * Coefficient tables come from the [host] helper (Pillow Resample.c precompute_coeffs/normalize_coeffs_8bpc):
 * bounds [out,2] = (first tap, tap count), kk [out,ksize] 22-bit fixed point; upload both before the launch. */
int gom_resample_ksize_bilinear(int in_size, int out_size);                        /* [host], -1 on bad sizes */
int gom_resample_coeffs_bilinear(int in_size, int out_size, int* bounds, int* kk, int ksize);   /* [host] */
/* src [B,H,W,3] u8 -> dst [B,OH,OW,3] u8 (flip_channels != 0 swaps channels 0 and 2). */
int gom_resize_bilinear_u8_hwc3(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                int xksize, const int* ybounds, const int* ykk, int yksize, uint8_t* dst, int OH,
                                int OW, int flip_channels, void* stream);
/* src [B,H,W,3] u8 -> dst [B,OH,OW,4] f32 = (resized[flipped] - mean) / std, 4th channel 0 (the stem's layout). */
int gom_ingest_u8_hwc3_to_nhwc4(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                int xksize, const int* ybounds, const int* ykk, int yksize, const float* mean3,
                                const float* std3, float* dst, int OH, int OW, int flip_channels, void* stream);
/* Training augmentation (custom_transform.py:46-59, EfficientDetResizeCropTransform.apply_image): Pillow resize to
 * SH x SW followed by the slice [y0 : y0+OH, x0 : x0+OW], in one launch and without the SH x SW intermediate.  The tables
 * are those of H -> SH (ybounds/ykk) and W -> SW (xbounds/xkk); output pixel (oy, ox) is pixel (oy+y0, ox+x0) of the
 * resized image, with the arithmetic of the two entry points above.  GOM_ERR_INVALID_ARG, before any HIP call, when a
 * size is non-positive or the window leaves the resized image (x0 < 0, x0+OW > SW, likewise y).
 * src [B,H,W,3] u8 -> dst [B,OH,OW,3] u8. */
int gom_resize_crop_bilinear_u8_hwc3(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                     int xksize, const int* ybounds, const int* ykk, int yksize, uint8_t* dst, int SH,
                                     int SW, int y0, int x0, int OH, int OW, int flip_channels, void* stream);
/* src [B,H,W,3] u8 -> dst [B,OH,OW,4] f32 = (window[flipped] - mean) / std, 4th channel 0. */
int gom_ingest_crop_u8_hwc3_to_nhwc4(const uint8_t* src, int B, int H, int W, const int* xbounds, const int* xkk,
                                     int xksize, const int* ybounds, const int* ykk, int yksize, const float* mean3,
                                     const float* std3, float* dst, int SH, int SW, int y0, int x0, int OH, int OW,
                                     int flip_channels, void* stream);
/* A GEN_IMAGE_MOTION clip (vts_dataset_mapper.py:181-202 + `ImageList.from_tensors`, gom_lstmatcher.py:168-169): ONE source
 * image, T frames, one launch.  Frame t is the OH_t x OW_t window at (y0_t, x0_t) of its own SH_t x SW_t resize, normalised as
 * gom_ingest_crop_u8_hwc3_to_nhwc4 does (the same bits), at the top-left of a PH x PW frame; every other element of the frame,
 * the 4th channel included, is written as 0.0f by the kernel: dst needs no memset and may hold anything before the call.
 * frames [host] int32 [T][GOM_INGEST_MOTION_DESC_WORDS] = (SH, SW, y0, x0, OH, OW, xksize, yksize, xbounds, xkk, ybounds, ykk),
 * the last four being offsets in int32 words into `tables` [device, table_words words], which holds the tables of
 * gom_resample_coeffs_bilinear for W -> SW_t and H -> SH_t (frames may share a table).  GOM_ERR_INVALID_ARG, before any
 * HIP call: a null pointer, T outside 1..GOM_INGEST_MOTION_MAX_FRAMES, a window that leaves its resized image or PH x PW, a
 * tap count that is not gom_resample_ksize_bilinear's, a table that does not lie inside `tables`.
 * src [H,W,3] u8 -> dst [T,PH,PW,4] f32. */
#define GOM_INGEST_MOTION_MAX_FRAMES 16
#define GOM_INGEST_MOTION_DESC_WORDS 12
int gom_ingest_motion_u8_hwc3_to_nhwc4(const uint8_t* src, int H, int W, const int* tables, long table_words,
                                       const int* frames, int T, const float* mean3, const float* std3, float* dst, int PH,
                                       int PW, int flip_channels, void* stream);
/* ---- f1: result rows (eval.py:346-363, the per-instance conversion in front of the XML / JSON writers) --------
 * The per-instance work of the host's `frame_lines` for all n instances of a clip in ONE launch (one wave64 per instance):
 *   bd [n,25,4] fp32 (top x, top y, bottom x, bottom y per point, frame pixels), recs [n,25] int64 class ids,
 *   track_ids [n] int64 (may be NULL: the two id words are then 0), out [n, ld] int32, ld >= GOM_RESULT_ROWS_WORDS.
 * Words of one output row (polygon point p = top point p for p < 25, bottom point 49 - p otherwise):
 *   GOM_RR_POLY_I32  + 2p, +2p+1 : the polygon point truncated toward zero (numpy astype(int)), x then y
 *   GOM_RR_POLY_F32  + 2p, +2p+1 : the same point's fp32 bit patterns (the host finishes the rectangle from them)
 *   GOM_RR_RECS      + c         : recs[c] as int32 (saturated), c < 25
 *   GOM_RR_EMIT                  : bit c set iff character c is emitted by the CTC collapse: id < voc_size - 1 and
 *                                  (c == 0 or id[c-1] is a blank or id[c] != id[c-1])
 *   GOM_RR_NHULL                 : number of convex-hull points (de-duplicated points, sorted by (x, y), monotone chain
 *                                  popping on cross <= 0, order lower[:-1] + upper[:-1]; <= 2 distinct points are their hull)
 *   GOM_RR_HULL_MASK, +1         : bit p (low word: p < 32) set iff polygon point p is a hull point (first occurrence
 *                                  of a repeated point)
 *   GOM_RR_EDGE, +1              : polygon indices of the two ends (hull order) of the hull edge whose enclosing rectangle
 *                                  has the smallest area, first hull index winning ties, zero-length edges skipped;
 *                                  -1, -1 with fewer than 2 hull points.  GOM_RR_EDGE + 2 is 0 (padding).
 *   GOM_RR_TRACK_ID, +1          : track_ids[i], low word then high word (8-byte aligned for ld even)
 * The search is fp64 with the host code's operations in its order, each rounded once (no contraction; edge length
 * sqrt(ex*ex + ey*ey)); centre, size, angle and corners are left to the host (their libm calls differ in the last bit).
 * n == 0 is GOM_OK without a launch.  Coordinates are expected finite. */
#define GOM_RR_POLY_I32 0
#define GOM_RR_POLY_F32 100
#define GOM_RR_RECS 200
#define GOM_RR_EMIT 225
#define GOM_RR_NHULL 226
#define GOM_RR_HULL_MASK 227
#define GOM_RR_EDGE 229
#define GOM_RR_TRACK_ID 232
#define GOM_RESULT_ROWS_WORDS 234
int gom_result_rows_i32(const float* bd, const int64_t* recs, const int64_t* track_ids, int n, int voc_size,
                        int32_t* out, int ld, void* stream);
/* ---- Result rows of an online session (gomatching_amd/online.py): gathered from a ring, scaled per row ------------
 * The settling rule that decides WHEN a frame's rows may leave the model.  L = test_len, M = min_track_len,
 * R = max(L - 1, 1) = how many frames back a match can reach (meta_arch.py `track_frames`: the long-term window starts at
 * win_st = real + 1 - test_len and the short-term match sees frame real - 1; the native path carries
 * instances[-max(test_len - 1, 1):]).  After frame t (0-based) is tracked, with c(id) the detections of a track so far and
 * s(id) the last frame it was seen in, a track is
 *   confirmed  c >= M                : its rows are kept, past ones included;
 *   dead       c <  M and t >= s + R : frame t + 1 can no longer reach frame s, no later frame can take the id; rows dropped;
 *   open       otherwise.
 * A frame is settled when none of its ids is open; frames leave in frame order (the longest settled prefix of the pending
 * ones); M <= 0 settles every frame at once; closing the stream makes every open track dead.  A frame therefore leaves at
 * most D = max(M - 1, 0) * R frames after it was tracked, with exactly the rows `_remove_short_track` keeps offline.
 *
 * gom_result_rows_gather_i32: the rows of the n instances a descriptor names, one launch whatever frames they belong to.
 *   bd [cap,25,4] fp32 and recs [cap,25] int64: the session's ring, in NETWORK-input pixels (unscaled);
 *   desc [n][GOM_RR_DESC_WORDS] int32: ring row, track id low word, track id high word, sx bits, sy bits, 0.
 * Row k of out is word for word the row gom_result_rows_i32 writes for ONE instance whose boundary is bd[desc[k].row] with
 * every x multiplied by sx and every y by sy in fp32, each product rounded once (what gom_scale_xy_f32 leaves in place),
 * whose class ids are recs[desc[k].row] and whose track id is the descriptor's.  The scale pair is per row, so frames of
 * different sizes share a launch.  A ring row outside [0, cap) is clamped into the ring by the kernel (it never reads past
 * it); the Python wrapper refuses such a descriptor.  n == 0 is GOM_OK without a launch; otherwise cap >= 1 and no pointer
 * is NULL. */
#define GOM_RR_DESC_WORDS 6
int gom_result_rows_gather_i32(const float* bd, const int64_t* recs, long cap, const int32_t* desc, int n, int voc_size,
                               int32_t* out, int ld, void* stream);
/* ---- Result text (csrc/result_text.hip, csrc/result_text_core.h; results.write_video(device_text=True); eval --device-write)
 * The bytes of <out>/jsons/<video>.json and <out>/preds/res_<video>.xml, made from the rows where they lie on the device.
 * THE RULE: the bytes are those `results.write_video_results` / `VideoResultWriter` write, that is json.dumps(indent=4,
 * ensure_ascii=False) of the annotation and minidom's toprettyxml(indent="  "); spelled out below so that the kernels, the
 * shared core (built for the host by tools/result_text_hostcheck.cpp) and the plain-Python statement
 * (tests/result_text_statement.py) agree byte for byte.  Bytes are UTF-8.  <k> is k spaces, \n is one byte 0x0A.
 * A call covers frames first_frame .. first_frame + F - 1 of a video (0-based; frame f is written under the key f + 1).
 * A ROW is one row of gom_result_rows_i32 / gom_result_rows_gather_i32 (words) with its eight rectangle points pts[r][0..7]
 * (int64, finished on the host: results.finish_points) and keep[r]; a row with keep[r] == 0 writes nothing and counts nothing.
 * Frame f of the call owns rows frame_rows[f] .. frame_rows[f+1] - 1.
 *   JSON, frame f : ",\n" unless f == 0 (the ABSOLUTE index: first_frame + the frame's place in the call), then
 *                   <4>"<f+1>": [] for a frame without kept rows, else <4>"<f+1>": [\n, the rows joined by ",\n", \n<4>]
 *   JSON, row     : <8>{\n
 *                   <12>"points": [\n   <16>P0,\n <16>P1,\n ... <16>P7\n   <12>],\n
 *                   <12>"ID": I,\n
 *                   <12>"transcription": "T",\n
 *                   <12>"segmentation": [\n <16>[\n
 *                       50 times  <20>[\n <24>X,\n <24>Y\n <20>]   joined by ",\n"
 *                   \n<16>]\n <12>]\n <8>}
 *                   (spaces between the pieces above only separate them; the bytes are the pieces, one after another)
 *   The host writes "{\n" before frame 0 and "\n}" after the last frame; a video without frames is "{}".
 *   XML, frame f  : <2><frame ID="f+1"/>\n without kept rows, else <2><frame ID="f+1">\n, the objects, <2></frame>\n
 *   XML, object   : <4><object ID="I" Transcription="T">\n
 *                   4 times <6><Point x="P2i" y="P2i+1"/>\n
 *                   <4></object>\n
 *   The host writes <?xml version="1.0" ?>\n<Frames>\n before frame 0 and </Frames>\n at the end (a video without frames:
 *   the declaration line alone).
 *   Integers      : plain decimal, '-' in front of a negative one, no other sign, no leading zero.  P0..P7 = pts (int64),
 *                   I = the int64 in words GOM_RR_TRACK_ID (low), +1 (high), X Y = words GOM_RR_POLY_I32 + 2p, + 2p + 1 (int32).
 *                   INT64_MIN is -9223372036854775808.
 *   T             : for c = 0 .. 24 in order, where bit c of word GOM_RR_EMIT is set: the table entry of id = word
 *                   GOM_RR_RECS + c.  A table is [ntab][GOM_RT_ENTRY_BYTES] u8 with ntab = voc_size - 1: byte 0 = the
 *                   entry's length L (0 .. 7; a larger byte counts as 7), bytes 1 .. L = the character as the writer
 *                   escapes it -- json_tab for the JSON stream, xml_tab for the XML stream (results.text_tables builds both
 *                   from json.dumps and minidom themselves).  An emitted id outside [0, ntab) is never used as an index: its
 *                   row is left out of both streams and totals[GOM_RT_STATUS] is set to GOM_RT_BAD_ID (the wrapper raises).
 * Two calls, because the size of the text is a result:
 *   gom_result_text_count_scan : `count` (one wavefront per row: the JSON and XML byte lengths of every row, 0 for a dropped one,
 *                   -1 for a bad id) and `scan` (ONE block: exclusive int64 scans over the rows, then over the frames with their
 *                   wrappers and row separators).  Leaves row_len int32 [2][n], row_off int64 [2][n+1] (bytes of the kept rows
 *                   before row r, wrappers and separators not counted), row_kept int32 [n+1] (kept rows before row r),
 *                   frame_off int64 [2][F+1] (frame f's first byte in the JSON / XML stream of this call) and totals int64
 *                   [GOM_RT_TOTALS] = {JSON bytes, XML bytes, status, 0}: the one thing the caller reads back.
 *   gom_result_text_emit       : `emit`, with buffers of json_cap / xml_cap bytes (the totals, as the caller read them): one
 *                   wavefront per row formats the row into LDS (the same core functions that counted it, a lane per piece: a
 *                   polygon point, a rectangle point, the id, the transcription; a wave scan places them) and stores it; one
 *                   wavefront per frame writes the frame's wrappers.  Every store index is checked against the length the count
 *                   pass left and against the cap: a byte that does not fit is not written.  The arrays must be the ones the
 *                   count_scan call left for the same inputs.
 * No atomics, no scratch, one writer per output byte, plain and vector stores only; the result depends on nothing but the
 * input: bitwise reproducible.  frame_rows must be non-decreasing with frame_rows[0] = 0 and frame_rows[F] = n (the wrapper
 * checks it on the host; the kernels clamp what they read into [0, n], so nothing is read or written out of bounds either way).
 * GOM_ERR_INVALID_ARG before any HIP call: n < 1, F < 1, ld < GOM_RESULT_ROWS_WORDS, ntab < 1, first_frame < 0 or
 * first_frame + F > 2^31 - 2, a negative cap, a null pointer. */
#define GOM_RT_ENTRY_BYTES 8
#define GOM_RT_TOTALS 4
#define GOM_RT_STATUS 2
#define GOM_RT_BAD_ID 1
#define GOM_RT_SCAN_BLOCK 256
int gom_result_text_count_scan(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                               const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                               const uint8_t* xml_tab, int ntab, int32_t* row_len, int64_t* row_off, int32_t* row_kept,
                               int64_t* frame_off, int64_t* totals, void* stream);
int gom_result_text_emit(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                         const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab, const uint8_t* xml_tab,
                         int ntab, const int32_t* row_len, const int64_t* row_off, const int32_t* row_kept,
                         const int64_t* frame_off, uint8_t* json, long json_cap, uint8_t* xml, long xml_cap, void* stream);
/* ---- Result parse (csrc/result_parse.hip, csrc/result_parse_core.h; results.parse_json_device; show --device-read) ----------
 * The inverse of the JSON stream above: the bytes of jsons/<video>.json -> the rows, where they lie on the device.
 * THE RULE.  ACCEPTED is a byte string that equals, byte for byte, json.dumps(A, ensure_ascii=False, indent=4) for an annotation
 * A of the canonical shape: keys "1", "2", .. "F" in that order (F = 0: the two bytes {}); every value a list of objects; every
 * object "points" (exactly 8 integers), "ID" (an integer), "transcription" (a string), in that order, and then possibly
 * "segmentation": a list of exactly one contour of n >= 0 [x, y] integer pairs.  Integers are plain decimal: an optional '-',
 * no leading zero, no "-0", no fraction, no exponent; ID fits int64, every other integer int32.  Everything else is REFUSED
 * with a status word (a set of the GOM_RP_BAD_* bits below); a refused file is no error: its caller reads it with json.load.
 * THE PROPERTY: for any bytes, either the status is nonzero or json.dumps(.., ensure_ascii=False, indent=4) of the parsed rows
 * gives the input back byte for byte.  The rule may refuse too much; it never accepts what json.loads reads differently.
 * The text holds one token per line and a raw 0x0A never lies inside a JSON string, so every value sits at a fixed line offset
 * from the line that opens its object; the rule is stated over LINES (<k> is k spaces, \n one byte 0x0A):
 *   Lines   : the bytes between the 0x0A bytes; L = (number of 0x0A) + 1; line i is [line_start[i], line_start[i+1] - 1),
 *             line_start[0] = 0, line_start[L] = size + 1.
 *   Stage 1 : L == 1: accepted with F = 0 iff the bytes are {} , else GOM_RP_BAD_ENDS.  L >= 2: the file begins {\n and ends
 *             \n} or GOM_RP_BAD_ENDS.  A nonzero status ends the parse here (and after stage 2): the later stages are not run.
 *   Stage 2 : a line longer than GOM_RP_MAX_LINE bytes: GOM_RP_BAD_LINE.  MARKS: an object line is exactly <8>{ ; a key line
 *             begins <4>" .  N = the object lines, F = the key lines; F == 0 here: GOM_RP_BAD_PLACE.  The marks in line order,
 *             and the file's last line after them, bound each other's spans.
 *   Stage 3 : every object and every frame is held against its template; the status is the OR over all of them.
 *     object o, opened at line s, the next mark (or the last line) at line e: nl = e - s if that mark is an object line, else
 *             e - s - 1 (the frame's closing line).  n = (nl - 18) / 4 if nl >= 22 and 4 divides nl - 18, else 0; poly_off is
 *             the exclusive scan of n.  Among the offsets j = 2 .. min(nl, 64) - 1 the first line that is <12>], : none:
 *             GOM_RP_BAD_PLACE; not at j = 10: GOM_RP_BAD_POINTS; either way the object is checked no further.  nl not 14, 17
 *             or 18 + 4 n with n >= 1: GOM_RP_BAD_PLACE, and no further.  Else line s + j must be, for
 *               j = 0 <8>{    1 <12>"points": [    2 .. 9 <16>P,  (no comma at 9; int32)    10 <12>],    11 <12>"ID": I,  (int64)
 *               12 <12>"transcription": "T"  followed by a comma iff nl > 14        nl - 1 <8>}  followed by a comma iff the
 *               next mark is an object line;        and for nl > 14:   13 <12>"segmentation": [    nl - 2 <12>]
 *               nl == 17: 14 <16>[]        nl > 17: 14 <16>[    nl - 3 <16>]    and for point p < n at j = 15 + 4 p:
 *               <20>[    <24>X,    <24>Y    <20>]  followed by a comma iff p < n - 1.
 *             A line that is not its template: GOM_RP_BAD_PLACE.  An integer token (the bytes between the indent or key and
 *             the line's end or comma) that holds a byte outside -+.eE0-9 or begins with none of -0123456789:
 *             GOM_RP_BAD_PLACE; one that is not canonical or out of range: GOM_RP_BAD_INT.  T ends at the first " that no
 *             backslash precedes (a backslash takes the byte after it with it); none on the line: GOM_RP_BAD_LINE.
 *     frame f, its key at line k, the next mark at line e, the next key line (or the last line) at line x, rows r0 .. r1 - 1:
 *             f == 0 and (k != 1 or r0 != 0): GOM_RP_BAD_PLACE.  The key line is <4>"K": [ or <4>"K": [] and then possibly
 *             a comma, or GOM_RP_BAD_PLACE and the frame is checked no further; K not canonical or K != f + 1:
 *             GOM_RP_BAD_KEY.  Without rows: the [] form, e == k + 1, a comma iff f < F - 1.  With rows: the [ form without a
 *             comma, e == k + 1, and line x - 1 is <4>] followed by a comma iff f < F - 1.  Else GOM_RP_BAD_PLACE.
 *   Strings : the device only locates T (t_off, t_len: the bytes between the quotes).  The host decodes every distinct span
 *             once with json.loads and refuses the file (GOM_RP_BAD_STRING) unless json.dumps(.., ensure_ascii=False) of the
 *             decoded string gives the span back.
 * Three calls, because L, then F and N, are results the next call's buffers are sized by; totals int64 [GOM_RP_TOTALS] is what
 * the caller reads between them (zeroed by the caller before the first; every slot has one writing call):
 *   gom_result_parse_lines : a thread per GOM_RP_THREAD_BYTES bytes counts the 0x0A bytes, a block per GOM_RP_BLOCK_BYTES; ONE
 *             block scans the nblk = ceil(size / GOM_RP_BLOCK_BYTES) block counts in place (tiles of GOM_RP_BLOCK) and does
 *             stage 1.  -> totals[GOM_RP_L], totals[GOM_RP_STATUS_LINES].
 *   gom_result_parse_marks : writes line_start int32 [L + 1]; a lane per line flags the marks and the long lines, a block per
 *             GOM_RP_BLOCK lines (nmblk = ceil(L / GOM_RP_BLOCK); mblk int32 [2][nmblk], sblk int32 [nmblk]); ONE block scans.
 *             -> totals[GOM_RP_F], totals[GOM_RP_N], totals[GOM_RP_STATUS_MARKS].
 *   gom_result_parse_emit  : writes mark_line int32 [N + F + 1], obj_mark int32 [N], frame_mark int32 [F], frame_rows int32
 *             [F + 1]; ONE block scans n -> poly_off int32 [N + 1]; a wavefront per object and per frame does stage 3, a lane
 *             per line, and stores ids int64 [N], pts int32 [N][8], has_seg u8 [N], t_off int64 [N], t_len int32 [N], poly_xy
 *             int32 [cap_p][2] (cap_p >= P; floor(L / 4) always is) and its status into unit_status int32 [N + F]; ONE block
 *             folds them.  -> totals[GOM_RP_P], totals[GOM_RP_STATUS].  A value that does not fit its array (cap_p too
 *             small) is not stored: GOM_RP_BAD_CAP.
 * No atomics, no scratch, one writer per output word; every read is bounded by the file's end, every store index checked; the
 * result depends on nothing but the input: bitwise reproducible.  The outputs of a refused file are unspecified.
 * GOM_ERR_INVALID_ARG before any HIP call: a null pointer, size < 1 or size >= 2^31 - 1 (the wrapper refuses such a file with
 * GOM_RP_BAD_SIZE and launches nothing), nblk or nmblk that is not the count above, L < 2 or L > size + 1, F < 1, N < 0,
 * F + N > L, cap_p < 0. */
#define GOM_RP_BAD_PLACE 1
#define GOM_RP_BAD_INT 2
#define GOM_RP_BAD_KEY 4
#define GOM_RP_BAD_POINTS 8
#define GOM_RP_BAD_LINE 16
#define GOM_RP_BAD_ENDS 32
#define GOM_RP_BAD_SIZE 64
#define GOM_RP_BAD_STRING 128
#define GOM_RP_BAD_CAP 256
#define GOM_RP_BLOCK 256
#define GOM_RP_THREAD_BYTES 16
#define GOM_RP_BLOCK_BYTES 4096
#define GOM_RP_MAX_LINE 1024
#define GOM_RP_MAX_SIZE 2147483646
#define GOM_RP_TOTALS 8
#define GOM_RP_L 0
#define GOM_RP_F 1
#define GOM_RP_N 2
#define GOM_RP_P 3
#define GOM_RP_STATUS 4
#define GOM_RP_STATUS_LINES 5
#define GOM_RP_STATUS_MARKS 6
int gom_result_parse_lines(const uint8_t* data, long size, int32_t* blk, int nblk, int64_t* totals, void* stream);
int gom_result_parse_marks(const uint8_t* data, long size, const int32_t* blk, int nblk, long L, int32_t* line_start,
                           int32_t* mblk, int32_t* sblk, int nmblk, int64_t* totals, void* stream);
int gom_result_parse_emit(const uint8_t* data, long size, const int32_t* line_start, long L, const int32_t* mblk, int nmblk,
                          int F, int N, int32_t* mark_line, int32_t* obj_mark, int32_t* frame_mark, int32_t* frame_rows,
                          int32_t* poly_off, int64_t* ids, int32_t* pts, uint8_t* has_seg, int64_t* t_off, int32_t* t_len,
                          int32_t* poly_xy, long cap_p, int32_t* unit_status, int64_t* totals, void* stream);
/* ---- The scene of parsed rows (csrc/scene_polygons.hip; show.draw_video(parsed=...); show --device-read) ------------------
 * What `show.Scene` / `score_json.MaskSet` build on the host for the rows of frames f0 .. f1 - 1 of a video, made from the
 * arrays gom_result_parse_emit left (frame_rows int32 [F + 1], ids int64 [N], poly_off int32 [N + 1], poly_xy int32 [P][2]) for
 * an H x W frame, without the polygons becoming host lists.  The chunk's instances are i0 = frame_rows[f0] .. i1 - 1,
 * i1 = frame_rows[f1]; instance k of the chunk is row i0 + k with the points poly_xy[poly_off[i0 + k] .. poly_off[i0 + k + 1]).
 *   points   : poly_xy from point poly_off[i0] on, as it lies (the caller passes that address on; nothing is copied)
 *   mcoff    int32 [n_inst + 1] : the exclusive scan of (an instance has at least one point): an empty contour is dropped
 *   coff     int32 [n_cont + 1] : coff[mcoff[k]] = poly_off[i0 + k] - poly_off[i0] for a kept contour; coff[n_cont] = the points
 *   boxes    int32 [n_inst][4]  : with (xmin, xmax, ymin, ymax) over the instance's points, x0 = max(xmin, 0), y0 = max(ymin, 0),
 *                                 x1 = min(xmax, W - 1), y1 = min(ymax, H - 1): (y0, y1 + 1, x0 >> 5, (x1 >> 5) + 1) if x0 <= x1 and
 *                                 y0 <= y1, else (and without points) four zeros
 *   woff     int64 [n_inst + 1] : the exclusive scan of (boxes[k][1] - boxes[k][0]) * (boxes[k][3] - boxes[k][2])
 *   inst_off int32 [f1 - f0 + 1]: frame_rows[f0 + j] - i0
 *   inst_rgb u8 [n_inst][3]     : palette[m][c] with m = ids mod GOM_SP_PALETTE, the non-negative remainder (Python's %); with
 *                                 bgr != 0 the channels reversed.  palette: u8 [GOM_SP_PALETTE][3].
 *   status   int32 [1]          : GOM_SP_BAD_COORD if a coordinate of a point lies beyond +-GOM_SP_MAX_COORD (the wrapper raises
 *                                 MaskSet's message); GOM_SP_BAD_SHAPE if n_inst is not i1 - i0 or n_cont not the kept contours
 *                                 (the caller counts both from its copy of frame_rows and poly_off).
 * Two launches: a lane per instance (boxes, colours, a status word each in inst_status int32 [n_inst]), then ONE block of
 * GOM_SP_BLOCK threads (the scans, coff, inst_off, the fold of the status words).  No atomics, no scratch, one writer per output
 * word; every index read from the arrays is clamped into its array before use, every store index checked.  Bitwise
 * reproducible.  GOM_ERR_INVALID_ARG before any HIP call: a null pointer, F < 1, N < 0, P < 0, not 0 <= f0 < f1 <= F, n_inst < 0,
 * n_cont < 0 or > n_inst, H < 1, W < 1, H * W > 2^31 - 1, boxes not 16-byte aligned, poly_xy not 8-byte aligned. */
#define GOM_SP_PALETTE 500
#define GOM_SP_MAX_COORD 1048576
#define GOM_SP_BLOCK 256
#define GOM_SP_BAD_COORD 1
#define GOM_SP_BAD_SHAPE 2
int gom_scene_polygons_i32(const int32_t* frame_rows, int F, const int64_t* ids, const int32_t* poly_off, int N,
                           const int32_t* poly_xy, int P, int f0, int f1, int H, int W, const uint8_t* palette, int bgr,
                           int32_t* coff, int n_cont, int32_t* mcoff, int32_t* boxes, int64_t* woff, int32_t* inst_off,
                           uint8_t* inst_rgb, int32_t* inst_status, int n_inst, int32_t* status, void* stream);
/* ---- Track vote (csrc/track_vote.hip, csrc/track_vote_core.h; results.TrackVote; eval --device-write --device-vote) --------
 * The bytes of <out>/preds/res_<video>.txt, one line per track with the track's majority transcription, made from the rows
 * where they lie on the device.  THE RULE: the bytes are those `results.write_track_transcriptions` writes after parsing the
 * video's XML (eval.py:182-210, getid_text); spelled out below so that the kernels, the shared core (built for the host by
 * tools/track_vote_hostcheck.cpp) and the plain-Python statement (tests/track_vote_statement.py) agree byte for byte.
 *   Which rows vote : a video's voting rows are its kept rows in file order: frame ascending, row order within the frame.  A row
 *                   with keep == 0 (the min-extent drop of results.finish_points) is not in the XML and does not vote.
 *   A row's text    : for c = 0 .. 24 in order, where bit c of word GOM_RR_EMIT is set: the txt-table entry of id = word
 *                   GOM_RR_RECS + c.  The txt table is [ntab][GOM_RT_ENTRY_BYTES] u8 with ntab = voc_size - 1, byte 0 = the
 *                   entry's length L (0 .. 4; a larger byte counts as 4), bytes 1 .. L = the character as the host function
 *                   reads it back from the XML (results.txt_table: minidom's attribute serialisation, then the parser of
 *                   write_track_transcriptions), UTF-8.  A text is therefore at most 100 bytes.
 *   The vote        : two rows of a track agree when their text BYTES are equal (different ids may share an entry; ids are not
 *                   compared).  A row's count is the number of rows of its track, itself included, that agree with it.  The
 *                   winner of a track is the first row, in file order, with the greatest count: max(txts, key=txts.count).
 *                   Equality is exact: the length and every byte are compared, no hash stands in for them.
 *   The output      : for each track id that has a voting row, ascending as an int64: the line  "I","W"\n  -- I the id in plain
 *                   decimal ('-' in front of a negative one, INT64_MIN is -9223372036854775808), W the winner's text bytes as
 *                   they are, nothing escaped, \n one byte 0x0A.  A video without voting rows gives no bytes.
 *   Bad ids         : an emitted id outside [0, ntab) is never used as an index: its row gets the length GOM_TV_LEN_BAD, does
 *                   not vote, and totals[GOM_TV_STATUS] of the vote that sees it is GOM_TV_BAD_ID (the wrapper raises).
 * A RECORD is GOM_TV_RECORD_WORDS int32 words: the track id's low and high word, the text's byte length (GOM_TV_LEN:
 * GOM_TV_LEN_DROPPED for a row that does not vote, GOM_TV_LEN_BAD for a bad id; the text words of both are 0), then
 * GOM_TV_TEXT_WORDS words of text from GOM_TV_TEXT on, byte b in bits 8 * (b % 4) .. of word b / 4, zero after the last byte: two
 * texts are equal iff their length words and all their text words are.
 *   gom_track_vote_records_i32 : one lane per row of a call: records [n][GOM_TV_RECORD_WORDS] from words (rows of
 *                   gom_result_rows_i32 / gom_result_rows_gather_i32, leading dimension ld) and keep [n].  Python appends every
 *                   call's records to the video's LOG; a record's log position is its place in file order.
 *   gom_track_vote_count_scan  : the vote over a log of m records.  order int32 [nv]: the log positions of the records with a
 *                   length other than GOM_TV_LEN_DROPPED, sorted by (track id, log position); seg int32 [T + 1]: track t owns
 *                   order[seg[t] .. seg[t+1] - 1] (the ordering itself is a stable sort, done by the caller).  One workgroup of
 *                   GOM_TV_BLOCK lanes per track: a lane holds its record in registers and walks the track's records, every
 *                   lane reading the same one (streamed from L2; a track need not fit LDS, nor have one row per frame); the
 *                   winner is the workgroup's maximum of count << 32 | (0xFFFFFFFF - place in the track).  Leaves winner
 *                   int32 [T][GOM_TV_WINNER_WORDS] = {the winner's log position, its count, the line's byte length, status}.
 *                   Then ONE block: exclusive int64 scans of the line lengths in tiles of the block -> line_off int64 [T + 1],
 *                   and totals int64 [GOM_TV_TOTALS] = {bytes, status}: the one thing the caller reads back.
 *   gom_track_vote_emit        : one wavefront per track writes its line, a lane per byte, into out [cap] (cap = the bytes read
 *                   back).  The arrays must be the ones the count_scan call left for the same log.
 * No atomics, no scratch, one writer per output word and byte; every store index is checked (a line that does not lie inside
 * [0, cap) or whose length is not the one the scan saw is not written); an order or seg entry outside its array is clamped or
 * skipped and sets GOM_TV_BAD_ORDER, it is never used as an index unchecked.  The result depends on nothing but the input:
 * bitwise reproducible.  GOM_ERR_INVALID_ARG before any HIP call: n < 1, ld < GOM_RESULT_ROWS_WORDS, ntab < 1, m < 1 or
 * m > 2^31 - 1, nv < 1 or nv > m, T < 1 or T > nv, a negative cap, a null pointer. */
#define GOM_TV_RECORD_WORDS 28
#define GOM_TV_LEN 2
#define GOM_TV_TEXT 3
#define GOM_TV_TEXT_WORDS 25
#define GOM_TV_ENTRY_MAX 4
#define GOM_TV_LEN_DROPPED -1
#define GOM_TV_LEN_BAD -2
#define GOM_TV_WINNER_WORDS 4
#define GOM_TV_TOTALS 2
#define GOM_TV_STATUS 1
#define GOM_TV_BAD_ID 1
#define GOM_TV_BAD_ORDER 2
#define GOM_TV_BLOCK 256
int gom_track_vote_records_i32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint8_t* txt_tab, int ntab,
                               int32_t* records, void* stream);
int gom_track_vote_count_scan(const int32_t* records, long m, const int32_t* order, long nv, const int32_t* seg, int T,
                              int32_t* winner, int64_t* line_off, int64_t* totals, void* stream);
int gom_track_vote_emit(const int32_t* records, long m, const int32_t* winner, const int64_t* line_off, int T, uint8_t* out,
                        long cap, void* stream);
/* ---- Quad -> Bezier control points (csrc/prepare.hip; python -m gomatching_amd.prepare) ------------------------
 * What datasets/vts.py:154-162 derives from a `poly` quad on every load (polygon2rbox -> LinearRing.is_ccw -> cpt_bezier_pts),
 * computed once per dataset: quads int32 [n,8] (x1,y1,..,x4,y4), hw int32 [n,2] (the quad's image H, W), out int32 [n,16]
 * = the two Bezier curves, 4 control points each, x then y.  One lane per quad, ONE launch for all n.
 * The rule for one quad, in integers and fp64 (each fp64 product, sum, quotient and square root rounded once: no contraction,
 * no fast-math), with no trigonometry, so that the kernel, the numpy path (prepare.quad_bezier_host) and the plain-Python
 * statement (tests/prepare_statement.py) give the same 16 words:
 *   1. Hull of the DISTINCT points: sorted by (x, y), monotone chain popping on cross <= 0 (cross products exact in int64),
 *      order lower[:-1] + upper[:-1]; one or two distinct points are their own hull.  Sizes 1, 2 (collinear), 3 (concave or a
 *      repeated point) and 4 all occur.
 *   2. Minimum-area rectangle over the hull's edges in hull order (edge i = hull[i] -> hull[(i+1) % size]; two points give two
 *      edges): norm = sqrt(ex*ex + ey*ey), ux = ex/norm, uy = ey/norm; for every hull point pu = x*ux + y*uy and
 *      pv = y*ux - x*uy; area = (umax-umin)*(vmax-vmin); the first strict minimum wins.
 *   3. Corners straight from the unit vector, c(u,v) = (u*ux - v*uy, u*uy + v*ux), in the order (umin,vmin), (umax,vmin),
 *      (umax,vmax), (umin,vmax), each coordinate truncated toward zero.  A one-point hull gives four equal corners.
 *   4. get_tight_rect (bezier_tools.py:44-77): the corners stably sorted by x into ps[0..3]; (p1, p4) = (ps[0], ps[1]) if
 *      ps[1].y > ps[0].y, else (ps[1], ps[0]); (p2, p3) = (ps[2], ps[3]) if ps[3].y > ps[2].y, else (ps[3], ps[2]); then
 *      x = min(max(x, 1), W-1) and y = min(max(y, 1), H-1) for p1, p2, p3, p4.
 *   5. Orientation: S = sum_i (x_i*y_{i+1} - x_{i+1}*y_i) over (p1, p2, p3, p4) cyclically, in int64; the four points are
 *      reversed iff S < 0.
 *   6. cpt_bezier_pts: of the four edges (p_i, p_{(i+1)%4}) the two longest, by integer squared length, ties to the lower
 *      index, longest first; per edge: p_i, then int((1-t)*a + t*b) per coordinate at t = 1/3 and t = 2/3 (t = k/3 in fp64, two
 *      products and a sum, truncated toward zero), then p_{i+1}.
 * UNPINNED against the reference: cv2.minAreaRect / cv2.boxPoints compute in float32 with their own calipers and corner
 * order (which can move a corner across a truncation and decides ties of the stable sort), and LinearRing.is_ccw at zero
 * area; steps 4 and 6 are pinned by the reference's own functions (tests/golden/prepare_geometry.json).
 * Coordinates are expected within +-2^20 and H, W positive.  quads and out must be 16-byte aligned, hw 8-byte aligned (a quad
 * is read as two 16-byte words, a row written as four).  GOM_ERR_INVALID_ARG before any HIP call: n < 0, null or misaligned
 * pointers with n > 0.  n == 0 is GOM_OK without a launch.  The grid is sized by n alone; plain stores, no atomics: the
 * output is bitwise reproducible. */
int gom_quad_bezier_i32(const int32_t* quads, const int32_t* hw, int n, int32_t* out, void* stream);
/* Scoring (csrc/score.hip): the pairwise convex-quadrilateral measure of one video's objects, as the count pass and the
 * emit pass of a stream compaction over the (ground truth, detection) pairs of every frame.
 *   gt_quads [G,8], det_quads [D,8] int32 : x1,y1,..,x4,y4 in any point order (the convex hull is taken)
 *   gt_off [F+1], det_off [F+1] int32      : first object of each frame (CSR, gt_off[F] = G, det_off[F] = D); pairs exist
 *                                            only within a frame
 *   gt_key [G], det_key [D] int32          : a pair is eligible only when its two keys are equal
 *   pairs                                  : the sum over the frames of (ground truth) x (detections), as the caller counts it
 *   measure                                : 0 = IoU of the two hulls, 1 = overlap = intersection / area(detection hull)
 *   threshold                              : a pair is kept when its value is STRICTLY greater
 * Per pair: hull of each 4-gon (64-bit integer cross products; duplicate and collinear points collapse); 0 when either
 * hull has no area; otherwise the detection hull clipped by the ground-truth hull (Sutherland-Hodgman, <= 8 vertices) and
 * the shoelace area, in fp64 with every operation rounded once (side tests are fp64 cross products, exact on integer
 * vertices below 2^25).
 * gom_quad_pairs_count_f64: counts[g] = kept detections of ground-truth object g.
 * gom_quad_pairs_emit_f64 : scan [G] int64 = exclusive prefix sum of counts, total = their sum; writes, per kept pair, the
 *   detection's index within its frame (out_det, int32 [total]) and the value (out_val, fp64 [total]), ordered by ground
 *   truth, then detection.  One wavefront per ground-truth object, ballot + popcount prefix, no atomics: the output is
 *   bitwise reproducible and does not depend on the launch geometry.
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers, negative sizes, F == 0 with objects, measure outside {0, 1},
 * threshold outside (0, 1), pairs negative, above G * D or above INT32_MAX, total negative or above pairs.  G == 0 (and
 * for the emit pass total == 0) is GOM_OK without a launch; frames without ground truth or detections are valid. */
int gom_quad_pairs_count_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                             const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D, int F,
                             long pairs, int measure, double threshold, int32_t* counts, void* stream);
int gom_quad_pairs_emit_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                            const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D, int F,
                            long pairs, int measure, double threshold, const int64_t* scan, long total, int32_t* out_det,
                            double* out_val, void* stream);
/* Scoring, the detection protocol (csrc/score_det.hip): per frame, the ICDAR15-style greedy matching of ground truth and
 * detections, one launch per video.  Inputs as gom_quad_pairs_* takes them: gt_quads [G,8], det_quads [D,8], gt_off /
 * det_off [F+1] (CSR); gt_care [G] int32, 0 = a "don't care" object.
 * THE RULE, per frame with ground truth g = 0..Gf-1 and detections d = 0..Df-1 (indices within the frame):
 *   geometry   : exactly that of gom_quad_pairs_* (the same device functions): iou(g,d) is measure 0, over(g,d) measure 1 --
 *                the intersection over the detection's area, 0 for a detection without area; a hull without area gives 0.
 *   det_care[d]: 0 iff some don't-care g of the frame has over(g,d) > area_thr (STRICT), else 1.
 *   match[g]   : for g ascending over the care objects, the SMALLEST d with det_care[d] == 1, not taken by an earlier g, and
 *                iou(g,d) > iou_thr (STRICT); -1 when there is none; don't-care g get -1.  A matched d is taken.
 *   frame_stats[f] = (matched = the frame's match[g] >= 0, gt_care = its care objects, det_care_count = its det_care == 1).
 * Outputs: det_care int32 [D], match int32 [G] (the detection's index within its frame), frame_stats int32 [F,3].
 * One wavefront per frame; ballots and popcounts, no atomics, every output word has one writer: bitwise reproducible and
 * independent of the launch geometry.  Every index made from the device-side offsets is clamped.  A frame's detections
 * past its first 4096 are never matched (their det_care is still written): the caller refuses such frames beforehand.
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers (of a non-empty array), negative sizes, F == 0 with objects,
 * iou_thr or area_thr outside (0, 1).  F == 0 is GOM_OK without a launch; frames without ground truth, without detections
 * or without both are valid. */
int gom_quad_det_match_f64(const int32_t* gt_quads, const int32_t* det_quads, const int32_t* gt_off,
                           const int32_t* det_off, const int32_t* gt_care, int G, int D, int F, double iou_thr,
                           double area_thr, int32_t* det_care, int32_t* match, int32_t* frame_stats, void* stream);
/* Scoring on the pixel grid (csrc/mask_pairs.hip): the mask IoU of the ArTVideo protocol.
 *
 * Representation.  A mask is a box plus bit rows: boxes int32 [N,4] = (y0, y1, wx0, wx1), rows [y0, y1), 32-pixel word
 * columns [wx0, wx1) in ABSOLUTE alignment -- word wx holds the pixels 32*wx .. 32*wx+31, bit b is pixel 32*wx + b -- so two
 * masks are ANDed without shifts.  All masks of a call live in one uint32 buffer `words` [nwords]; mask k owns the
 * (y1-y0)*(wx1-wx0) words from word_off[k] (int64 [N+1], CSR), row-major.  Boxes and offsets are the caller's, computed
 * from the vertex extents or from the runs and clipped to the H x W image; a box that is too small loses pixels, one that
 * leaves the image or the buffer is cut back: only a mask's own words are ever written.
 *
 * Rasterisation rule (gom_mask_fill_polygons_u32): the project's statement of cv2.fillPoly(img, contours, 1) with lineType 8
 * and shift 0 -- PARITY with OpenCV is UNPINNED -- in 64-bit signed integers with S = 16.  The set is the union over a
 * mask's contours of Fill(contour) and Boundary(contour).
 *   Boundary: for every edge (v[i-1], v[i]), the closing edge included, the 8-connected line between the integer end
 *     points, both inclusive.  If x1 < x0 the end points are swapped (left to right).  M = max(|dx|, |dy|), m = min(|dx|,
 *     |dy|), err = M - 2m; M + 1 times: emit the pixel; if err < 0 step both axes and err += 2M - 2m, else step the major
 *     axis only and err -= 2m.  The major axis is x unless |dy| > |dx|.  Pixels outside the image are dropped.
 *   Fill: an edge with ya != yb is active on the scanlines min(ya, yb) <= y < max(ya, yb), at X(y) = (x_top << S) +
 *     (y - y_top) * dxq, dxq = ((x_bottom - x_top) << S) / (y_bottom - y_top) in C division (toward zero).  The active
 *     positions of a scanline sorted, c_1 <= c_2 <= .., each pair (c_1, c_2), (c_3, c_4), .. fills the pixels
 *     ceil(c_odd / 2^S) .. floor(c_even / 2^S) clipped to [0, W-1]; rows outside [0, H-1] are dropped; the lowest row of a
 *     contour gets its pixels from Boundary only.  Sort-free form, the one the kernel evaluates: for pixel x, Xp = x << S,
 *     a = the number of active positions < Xp, b = the number <= Xp: filled iff b > a or a is odd.
 *   points int32 [P,2] (x, y; expected within +-2^20), contour_off int32 [C+1] (first point of each contour), mask_coff
 *   int32 [N+1] (first contour of each mask).
 * gom_mask_fill_rle_u32: COCO run lengths, runs alternating 0 / 1 starting with 0 in column-major order (pixel index
 *   x * H + y).  ends int32 [R] = the cumulative run ends of every mask, run_off int32 [N+1] (first run of each mask): a
 *   pixel is set when an odd number of its mask's ends are <= its index.
 * Both: H * W <= INT32_MAX; sel = NULL fills all N masks (M must equal N), else int32 [M] names the masks to fill and the
 * others' words and areas are left alone (a set that mixes both kinds takes one call of each); area[k] int32 = the
 * popcount of mask k.  A thread owns a word: plain stores, bitwise reproducible.
 *
 * gom_mask_pairs_count_f64 / gom_mask_pairs_emit_f64: the contract of gom_quad_pairs_* over two filled sets (words, boxes,
 * word offsets, areas, nwords of each): gt_off / det_off int32 [F+1] first mask of each frame, pairs only within a frame
 * and between equal keys, `pairs` the sum over the frames of (ground truth) x (detections), threshold STRICT.  Per pair:
 * inter = popcount of the AND over the intersection of the two boxes; value 0.0 when inter < 1, else
 * (double)inter / (double)(area_g + area_d - inter), ONE division of integer counts: bitwise the host statement.
 * counts[g] = kept detections of ground-truth mask g; the emit pass takes scan [G] int64 = exclusive prefix sum of the
 * counts and total = their sum and writes per kept pair the detection's index within its frame (out_det int32 [total]) and
 * the value (out_val fp64 [total]), ordered by ground truth, then detection.  One wavefront per ground-truth mask, ballot
 * over box tests, shuffle reduction, no atomics: the output does not depend on the launch geometry.  Every index made
 * from device-side offsets is clamped.
 * The box arrays (boxes, gt_boxes, det_boxes) must be 16-byte aligned: a box is read as one 16-byte word.
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers, a box array that is not 16-byte aligned, negative sizes, H or W < 1, H * W above INT32_MAX, M != N
 * without sel or M > N with it, F == 0 with masks, threshold outside (0, 1), pairs negative, above G * D or above
 * INT32_MAX, total negative or above pairs.  M == 0, G == 0 (and for the emit pass total == 0) are GOM_OK without a launch. */
int gom_mask_fill_polygons_u32(const int32_t* points, int P, const int32_t* contour_off, int C, const int32_t* mask_coff,
                               const int32_t* boxes, const int64_t* word_off, int N, long nwords, const int32_t* sel, int M,
                               int H, int W, uint32_t* words, int32_t* area, void* stream);
int gom_mask_fill_rle_u32(const int32_t* ends, int R, const int32_t* run_off, const int32_t* boxes, const int64_t* word_off,
                          int N, long nwords, const int32_t* sel, int M, int H, int W, uint32_t* words, int32_t* area,
                          void* stream);
int gom_mask_pairs_count_f64(const uint32_t* gt_words, const int32_t* gt_boxes, const int64_t* gt_woff,
                             const int32_t* gt_area, long gt_nwords, const uint32_t* det_words, const int32_t* det_boxes,
                             const int64_t* det_woff, const int32_t* det_area, long det_nwords, const int32_t* gt_off,
                             const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D, int F,
                             long pairs, double threshold, int32_t* counts, void* stream);
int gom_mask_pairs_emit_f64(const uint32_t* gt_words, const int32_t* gt_boxes, const int64_t* gt_woff,
                            const int32_t* gt_area, long gt_nwords, const uint32_t* det_words, const int32_t* det_boxes,
                            const int64_t* det_woff, const int32_t* det_area, long det_nwords, const int32_t* gt_off,
                            const int32_t* det_off, const int32_t* gt_key, const int32_t* det_key, int G, int D, int F,
                            long pairs, double threshold, const int64_t* scan, long total, int32_t* out_det,
                            double* out_val, void* stream);
/* Drawing tracked text on frames (csrc/overlay.hip): an outline pass over the bit-row masks above and a compositor.
 *
 * gom_mask_outline_polygons_u32: the arguments and the mask representation of gom_mask_fill_polygons_u32 (boxes, CSR word
 * offsets, sel) without `area`; writes Boundary(contour) of the rasterisation rule above ALONE, unioned over a mask's
 * contours, clipped to the image.  A thread owns a word: plain stores.  Same argument checks as the fill.
 *
 * gom_overlay_compose_u8: frames u8 [F,H,W,3] -> out u8 [F,H,W,3] (out may be frames; rows and frames start at any byte
 * alignment).  Device inputs:
 *   face_words, outline_words uint32 [nwords] : two mask sets over the SAME boxes int32 [N,4] and word_off int64 [N+1] -- what
 *                                               the fill call (Fill u Boundary) and the outline call leave
 *   inst_off int32 [F+1]                      : first instance of each frame (CSR, inst_off[F] = N)
 *   inst_rgb u8 [N,3]                         : an instance's colour, in the frames' own channel order
 *   label_off int32 [F+1], label_pos int32 [L,2] (x0, y0 of the top-left corner; any value, may lie outside the image),
 *   label_glyph int32 [L] (index into the atlas), label_rgb u8 [L,3]
 *   glyph_wh int32 [G,2] (w, h), glyph_woff int64 [G+1], glyph_words uint32 [glyph_nwords] : the atlas of label bitmaps, rows
 *                                               padded to whole words and label-local: bit b of word j of a row is column
 *                                               32 j + b; bitmap g owns h * ((w + 31) / 32) words from glyph_woff[g]
 *   a_face, a_box                             : 0 .. 255
 * Rule, in integers.  For pixel (x, y) of frame f, v = frames[f,y,x,:], then
 *   1. for the instances k = inst_off[f] .. inst_off[f+1] - 1 IN ORDER: if the outline bit of (x, y) is set v = inst_rgb[k],
 *      else if the face bit is set v = blend(v, inst_rgb[k], a_face);
 *   2. then for the labels k = label_off[f] .. label_off[f+1] - 1 IN ORDER, g = label_glyph[k], when x0 <= x < x0 + w and
 *      y0 <= y < y0 + h: if bit (x - x0, y - y0) of bitmap g is set v = label_rgb[k], else v = blend(v, (255,255,255), a_box);
 *   3. blend(p, c, a) = (p * (255 - a) + c * a + 127) / 255 per channel, exact integer division;
 *   out[f,y,x,:] = v.  Pixels no instance and no label covers come out byte-identical.
 * A pixel is read and written by exactly one thread, instances and labels are walked in ballot order: no atomics, the
 * result does not depend on the launch geometry.  Offsets, boxes, positions and atlas indices are clamped or tested against
 * their buffers (a mask word outside the words its box owns, or outside the buffer, reads as 0).
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers, negative sizes, H or W < 1, H * W above INT32_MAX, a_face or a_box
 * outside 0 .. 255, a box array that is not 16-byte aligned, labels without an atlas (L > 0 with G == 0).  F == 0 is GOM_OK
 * without a launch; N == 0 and L == 0 with F > 0 copy frames to out when they differ.
 *
 * gom_overlay_compose_gather_u8: the same rule over frames that lie in a ring (the pending frames of an online session):
 * ring u8 [cap,H,W,3], slots int32 [F] on the device, out u8 [F,H,W,3], dense.  Rule: out[f] is word for word what
 * gom_overlay_compose_u8 writes for frames[f] = ring[slots[f]].  The ring is only read; a slot may repeat; `out` must not
 * overlap the ring.  The kernel clamps a slot outside [0, cap) into the ring, so it never reads past it (callers refuse such
 * a table).  One launch whatever the ring's wrap, the same kernel body with another source address.
 * GOM_ERR_INVALID_ARG before any HIP call: what the dense entry refuses, cap < 1, a null ring, out or (with F > 0) slots,
 * and an `out` [F,H,W,3] that overlaps [ring, ring + cap * H * W * 3).  F == 0 is GOM_OK without a launch; N == 0 and L == 0
 * copy ring[slots[f]] to out[f]. */
int gom_mask_outline_polygons_u32(const int32_t* points, int P, const int32_t* contour_off, int C, const int32_t* mask_coff,
                                  const int32_t* boxes, const int64_t* word_off, int N, long nwords, const int32_t* sel,
                                  int M, int H, int W, uint32_t* words, void* stream);
int gom_overlay_compose_u8(const uint8_t* frames, uint8_t* out, int F, int H, int W, const uint32_t* face_words,
                           const uint32_t* outline_words, const int32_t* boxes, const int64_t* word_off, int N, long nwords,
                           const int32_t* inst_off, const uint8_t* inst_rgb, const int32_t* label_off,
                           const int32_t* label_pos, const int32_t* label_glyph, const uint8_t* label_rgb, int L,
                           const int32_t* glyph_wh, const int64_t* glyph_woff, const uint32_t* glyph_words, int G,
                           long glyph_nwords, int a_face, int a_box, void* stream);
int gom_overlay_compose_gather_u8(const uint8_t* ring, int cap, const int32_t* slots, uint8_t* out, int F, int H, int W,
                                  const uint32_t* face_words, const uint32_t* outline_words, const int32_t* boxes,
                                  const int64_t* word_off, int N, long nwords, const int32_t* inst_off, const uint8_t* inst_rgb,
                                  const int32_t* label_off, const int32_t* label_pos, const int32_t* label_glyph,
                                  const uint8_t* label_rgb, int L, const int32_t* glyph_wh, const int64_t* glyph_woff,
                                  const uint32_t* glyph_words, int G, long glyph_nwords, int a_face, int a_box, void* stream);
/* ---- Lexicon correction of transcriptions (csrc/lexicon.hip; python -m gomatching_amd.lexicon) ------------------
 * The reference's `find_match_word` (third_party/adet/evaluation/text_evaluation_all.py:249-264, accepted at :332): a
 * recognised word is snapped to the first lexicon word at the smallest edit distance.  THE RULE, integer-exact, so that the
 * kernel, the numpy path (lexicon.host_match) and the plain-Python statement (tests/lexicon_statement.py) agree word for word:
 *   Normalisation : norm(s) = s.upper(), Python's str.upper (it can lengthen a string: 'ß' -> 'SS'), taken as a sequence of
 *                   Unicode code points.  Both sides are normalised on the host; the device sees code points only.
 *   Length limit  : at most GOM_LEXICON_MAX_LEN = 64 code points after normalisation, for queries and for words (a longer
 *                   lexicon line is an error naming the file and line, a longer transcription one naming the video and frame).
 *   Lexicon       : the lines of a text file, stripped, blank lines skipped, in file order, duplicates kept.
 *   Display map   : `pairs`.  With a pair-list file, for each stripped line key = line.split(' ')[0].upper(),
 *                   value = line[len(key)+1:], later lines win (:206-210).  Without one pairs[norm(line)] = line over the
 *                   lexicon's lines, later lines win (:198).  A lexicon word whose normal form has no entry is an error (the
 *                   reference raises KeyError).
 *   Match         : of a query q against a segment of words w_0 .. w_{n-1}: d_i = the Levenshtein distance of q and w_i (unit
 *                   insert, delete and substitute, NO transposition: "AB" against "BA" is 2); the result is (i*, d*) with
 *                   d* = min d_i and i* the LOWEST index that attains it (the reference's strict `<` in file order); an
 *                   empty segment gives (-1, 100), the reference's initial values.
 *   Acceptance    : d* <= max_dist, by default 1 (the reference's `< 1.5`); an accepted transcription becomes
 *                   pairs[norm(w_i*)], one that is not accepted is kept (`keep`) or its row removed (`drop`).  On the host.
 * gom_lexicon_match_u32: ONE launch for all queries of all segments (per-video lexicons and one shared lexicon are the same call).
 *   q_chars uint32 [q_nchars], q_off int32 [S+1] : the queries' code points (CSR)
 *   q_seg int32 [S]                              : each query's segment
 *   w_chars uint32 [w_nchars], w_off int32 [W+1] : the words' code points (CSR), all segments one after the other
 *   seg_off int32 [n_seg+1]                      : first word of each segment (CSR, seg_off[n_seg] = W)
 *   max_len                                      : the largest length of a query or a word, as the caller counts it
 *   best_index, best_dist int32 [S]              : i* WITHIN the query's segment (or -1) and d*
 * Code points are 32-bit words, not packed 16-bit ones: an astral code point needs 21 bits, surrogate pairs would change the
 * distance, and the whole 90 000-word vocabulary is 3 MB that stays in L2 -- the launch is bound by integer ALU, not by bytes.
 * One 256-thread workgroup per query; lanes stride over the segment's words in ascending index; per pair the Hyyro bit-vector
 * form of the Levenshtein recurrence on one 32- or 64-bit word (the query is the pattern; the equality masks of the code
 * points below 256 are a per-query LDS table, any other code point is compared against the query's); a lane skips a word when
 * |len(w) - len(q)| >= its own running best, which is exact because a lane's indices ascend and a distance is never below the
 * length difference -- nothing depends on max_dist; (dist << 32 | index) is minimised by shuffles within a wave and through
 * LDS across the four waves, one lane writes.  No atomics, no scratch, every output word has one writer: bitwise
 * reproducible.  Offsets, segments and lengths are device data the host cannot vouch for: every index made from them is
 * clamped (a length above the limit is cut to it).
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers of non-empty arrays, negative sizes, q_nchars or w_nchars above
 * INT32_MAX, max_len above GOM_LEXICON_MAX_LEN, queries without a segment (S > 0 with n_seg == 0).  S == 0 is GOM_OK without
 * a launch. */
#define GOM_LEXICON_MAX_LEN 64
#define GOM_LEXICON_NO_MATCH_DIST 100
int gom_lexicon_match_u32(const uint32_t* q_chars, long q_nchars, const int32_t* q_off, const int32_t* q_seg, int S,
                          const uint32_t* w_chars, long w_nchars, const int32_t* w_off, int W, const int32_t* seg_off,
                          int n_seg, int max_len, int32_t* best_index, int32_t* best_dist, void* stream);
/* ---- Lexicon correction of rows on the device (csrc/lexicon_rows.hip, csrc/lexicon_rows_core.h; eval --device-lexicon) ------
 * The corrected files OUT/lexicon/{jsons,preds} made from the rows where they lie, in the call that formats the original files:
 * nothing is parsed and nothing is dumped.  THE RULE: the bytes are those `lexicon.correct_results` writes from the original
 * files; spelled out below so that the kernels, the shared core (built for the host by tools/lexicon_rows_hostcheck.cpp) and
 * the plain-Python statement (tests/lexicon_rows_statement.py) agree byte for byte.
 *   Query of a row : for c = 0 .. 24 in order, where bit c of word GOM_RR_EMIT is set: the entry of id = word GOM_RR_RECS + c in
 *                   the norm table, uint32 [ntab][GOM_LR_NORM_WORDS] with ntab = voc_size - 1: word 0 = a count 0 .. 3 (a larger
 *                   one counts as 3), then the code points of label.upper() (`str.upper` works character by character and gives
 *                   at most 3 code points: lexicon.norm_table builds the entries from it and refuses anything else).  The query
 *                   is those code points one after another: lexicon.norm of the row's text.  A row with keep == 0 has the empty
 *                   query and its match is ignored.  An emitted id outside [0, ntab) is never used as an index: its row has the
 *                   empty query (the result text flags it: GOM_RT_BAD_ID).  A kept row whose query has more than
 *                   GOM_LEXICON_MAX_LEN code points has the length GOM_LR_LEN_LONG, is matched as the empty query, is never
 *                   accepted and sets q_status = {GOM_LR_TOO_LONG, the first such row} ({0, -1} otherwise); the wrapper raises.
 *   Match          : gom_lexicon_match_u32 as it is, one segment per call (the video's lexicon), a query per row: equal strings
 *                   are not deduplicated.
 *   Apply          : a row is accepted when keep and 0 <= index < W and dist <= max_dist.  ov[r] = index (the word's index
 *                   within its lexicon) for an accepted row, -1 for any other.  keep_out[r] = keep[r] and accepted with
 *                   drop = 1 (`unmatched = drop`), keep[r] with drop = 0.  totals int64 [GOM_LR_TOTALS] = {kept rows in,
 *                   accepted, dropped, q_status[0], q_status[1]}.
 *   Text of a row  : with ov[r] < 0 exactly what it is without a lexicon (the character tables).  With ov[r] = i entry i of the
 *                   stream's DISPLAY TABLE, as it is: a CSR byte table over the lexicon's W words, u8 bytes [dbytes] and int32
 *                   off [W + 1], built on the host from the libraries themselves over the WHOLE display form d = pairs[norm(w_i)]:
 *                   JSON json.dumps(d, ensure_ascii=False) without its quotes, XML minidom's attribute value, txt that value as
 *                   write_track_transcriptions' parser reads it back.  A JSON or XML form is at most 175 bytes (25 *
 *                   (GOM_RT_ENTRY_BYTES - 1): a row is no longer than the longest one without a lexicon), a txt form at most 100
 *                   (4 * GOM_TV_TEXT_WORDS); the host refuses a longer one before any upload, the kernels cut it.  An index or
 *                   an offset outside its table gives the empty form.  The vote still compares text bytes: an accepted row and
 *                   one that is not, with equal bytes, agree.
 * gom_lexicon_rows_queries_u32: count (a lane per row) / scan (ONE block, tiles of GOM_LR_BLOCK) / emit (a lane per row, one writer
 *   per word): q_len int32 [n], q_off int32 [n + 1] (CSR over q_chars; rows flagged GOM_LR_LEN_LONG own nothing), q_status int32
 *   [2], q_chars uint32 [q_cap] with q_cap >= n * GOM_LEXICON_MAX_LEN, so that no size has to be read back.  The offsets are
 *   int32: GOM_LR_MAX_ROWS is the largest n with n * GOM_LEXICON_MAX_LEN <= INT32_MAX.
 * gom_lexicon_rows_apply_i32: ONE block; ov int32 [n], keep_out u8 [n], totals.
 * gom_result_text_count_scan_ov / gom_result_text_emit_ov / gom_track_vote_records_ov_i32: the entries without `_ov` (their
 *   contracts, launches and checks) with ov, keep_out (a row writes and votes iff keep[r] and keep_out[r]) and the display
 *   table(s); with ov all -1 and keep_out = keep they leave the bytes of the entries without `_ov`.
 * No atomics, no scratch, plain stores, one writer per output word and byte; every index made from device data is checked or
 * clamped, every store checked against the counted extent and the cap; bitwise reproducible.  GOM_ERR_INVALID_ARG before any
 * HIP call: a null pointer, n < 0 or n > GOM_LR_MAX_ROWS, ld < GOM_RESULT_ROWS_WORDS, ntab < 1, q_cap < n * GOM_LEXICON_MAX_LEN,
 * W < 0, max_dist < 0, drop outside {0, 1}, a negative dbytes.  n == 0 is GOM_OK without a launch (the `_ov` text entries keep
 * n >= 1, as the entries without `_ov` do). */
#define GOM_LR_NORM_WORDS 4
#define GOM_LR_LEN_LONG -1
#define GOM_LR_TOO_LONG 1
#define GOM_LR_BLOCK 256
#define GOM_LR_MAX_ROWS 33554431
#define GOM_LR_TOTALS 5
#define GOM_LR_KEPT 0
#define GOM_LR_ACCEPTED 1
#define GOM_LR_DROPPED 2
#define GOM_LR_STATUS 3
#define GOM_LR_FIRST_LONG 4
int gom_lexicon_rows_queries_u32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint32_t* norm_tab, int ntab,
                                 int32_t* q_len, int32_t* q_off, int32_t* q_status, uint32_t* q_chars, long q_cap,
                                 void* stream);
int gom_lexicon_rows_apply_i32(const uint8_t* keep, const int32_t* q_len, const int32_t* q_status, const int32_t* best_index,
                               const int32_t* best_dist, int n, int W, int max_dist, int drop, int32_t* ov, uint8_t* keep_out,
                               int64_t* totals, void* stream);
int gom_result_text_count_scan_ov(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                                  const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab,
                                  const uint8_t* xml_tab, int ntab, const int32_t* ov, const uint8_t* keep_out,
                                  const uint8_t* json_disp, const int32_t* json_doff, long json_dbytes, const uint8_t* xml_disp,
                                  const int32_t* xml_doff, long xml_dbytes, int W, int32_t* row_len, int64_t* row_off,
                                  int32_t* row_kept, int64_t* frame_off, int64_t* totals, void* stream);
int gom_result_text_emit_ov(const int32_t* words, int ld, const int64_t* pts, const uint8_t* keep, int n,
                            const int32_t* frame_rows, int F, long first_frame, const uint8_t* json_tab, const uint8_t* xml_tab,
                            int ntab, const int32_t* ov, const uint8_t* keep_out, const uint8_t* json_disp,
                            const int32_t* json_doff, long json_dbytes, const uint8_t* xml_disp, const int32_t* xml_doff,
                            long xml_dbytes, int W, const int32_t* row_len, const int64_t* row_off, const int32_t* row_kept,
                            const int64_t* frame_off, uint8_t* json, long json_cap, uint8_t* xml, long xml_cap, void* stream);
int gom_track_vote_records_ov_i32(const int32_t* words, int ld, const uint8_t* keep, int n, const uint8_t* txt_tab, int ntab,
                                  const int32_t* ov, const uint8_t* keep_out, const uint8_t* txt_disp, const int32_t* txt_doff,
                                  long txt_dbytes, int W, int32_t* records, void* stream);
/* ---- JPEG encoding of drawn frames (csrc/jpeg.hip; gomatching_amd/jpeg.py; show --device-encode) -------------------
 * Baseline sequential DCT, 8 bits, three components at 4:2:0 (sampling (2,2), (1,1), (1,1)) in a JFIF 1.01 container: the
 * layout of Pillow's `save(quality=q)`, with a restart interval per MCU row so that every MCU row is coded independently.
 * THE RULE, in integers only (no floating point anywhere), so that the kernels, the numpy path (jpeg.encode_host) and the
 * plain-Python statement (tests/jpeg_statement.py) agree byte for byte.  `>>` is the arithmetic shift (floor), `/` of
 * non-negative integers is floor division.
 *   Input     : frames u8 [F,H,W,3]; bgr = 1: the channels are B, G, R (what `show` holds), 0: R, G, B.
 *   Padding   : MH = (H + 15) / 16 MCU rows of MW = (W + 15) / 16 MCUs of 16 x 16 pixels; pixel (y, x) of the padded image is
 *               pixel (min(y, H - 1), min(x, W - 1)): the last row and column replicated.  SOF0 carries the true H and W.
 *   Colour    : JFIF's full-range matrix in 16-bit fixed point, per pixel
 *                 Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                 Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *                 Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16          (each lies in 0 .. 255)
 *   Chroma    : a chrominance sample = the mean of its 2 x 2 block of Cb (Cr) values, (a + b + c + d + 2) >> 2.
 *   Blocks    : an MCU is Y00 Y01 Y10 Y11 Cb Cr (luminance blocks left to right, top to bottom); every sample s = value - 128.
 *   Transform : F = T s T^t on the integer table T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1/8),
 *               a(u) = 1/2, rows first:
 *                 T = { 2896,  2896,  2896,  2896,  2896,  2896,  2896,  2896,
 *                       4017,  3406,  2276,   799,  -799, -2276, -3406, -4017,
 *                       3784,  1567, -1567, -3784, -3784, -1567,  1567,  3784,
 *                       3406,  -799, -4017, -2276,  2276,  4017,   799, -3406,
 *                       2896, -2896, -2896,  2896,  2896, -2896, -2896,  2896,
 *                       2276, -4017,   799,  3406, -3406,  -799,  4017, -2276,
 *                       1567, -3784,  3784, -1567, -1567,  3784, -3784,  1567,
 *                        799, -2276,  3406, -4017,  4017, -3406,  2276,  -799 }
 *                 t[y][u] = (sum_x T[u][x] s[y][x] + 128) >> 8            (five fractional bits kept; |sum| < 2^23)
 *                 f[v][u] = (sum_y T[v][y] t[y][u] + (1 << 17)) >> 18     (|sum| < 2^30: 32-bit accumulators throughout)
 *   Quantise  : tables = Annex K.1 (luminance) and K.2 (chrominance), each entry (base * scale + 50) / 100 clamped to 1 .. 255
 *               with scale = 5000 / quality below 50 and 200 - 2 quality from 50 (quality 1 .. 100) -- Pillow's
 *               `Image.quantization` for the same quality.  k = sign(f) ((|f| + (q >> 1)) / q): half away from zero.  AC
 *               coefficients are clamped to -1023 .. 1023 (category 10, the largest a baseline AC code names).
 *   Entropy   : the four Annex K Huffman tables (K.3 - K.6), coefficients in zigzag order, DC as the difference from the
 *               previous block of the same component, categories and amplitude bits of F.1.2 (a negative value v is written
 *               as the low bits of v - 1), ZRL for every 16 zeros in front of a non-zero coefficient, EOB unless coefficient
 *               63 is non-zero.  Bits fill bytes from the most significant bit.
 *   Intervals : a restart interval = one MCU row (DRI = MW): the predictors start at 0, the last byte is filled with 1-bits,
 *               every byte 0xFF of the interval is followed by 0x00; between interval r and r + 1 of a frame stands RSTn,
 *               0xFF 0xD0 + (r mod 8).  A frame's DATA = its MH intervals and the MH - 1 markers between them.
 *   Container : SOI, APP0 (JFIF 1.01, density 1:1, no thumbnail), DQT 0 and DQT 1 (zigzag order), SOF0 (8 bits, H, W, components
 *               1: 0x22 table 0, 2 and 3: 0x11 table 1), DHT DC 0, AC 0, DC 1, AC 1, DRI, SOS (Ss 0, Se 63, Ah Al 0), DATA, EOI.
 *               Everything but DATA depends on H, W and quality alone and is made on the host (jpeg.header).
 * The device produces DATA of every frame, packed: payload[frame_off[f] .. frame_off[f+1]) for frame f.  Two calls, because the
 * payload's size is a result: the caller reads frame_off (F + 1 values), allocates, and packs.
 *   gom_jpeg_workspace_bytes : bytes of the workspace for F frames of H x W, or -1 (sizes the encoder refuses).  Per block 128
 *                              bytes of coefficients and 208 of staged code, per interval 416 bytes per block (+ 16) of stuffed
 *                              data -- the worst case of the format, of which a launch touches what the data needs.
 *   gom_jpeg_encode_scan_u8  : transform, entropy coding and the scan of the interval lengths (three launches): leaves every
 *                              interval's bytes in the workspace and writes frame_off int64 [F+1] (device).
 *   gom_jpeg_encode_pack_u8  : with total = frame_off[F] as the caller read it: one launch that writes payload[0 .. total)
 *                              (payload 4-byte aligned with payload_bytes >= total rounded up to 4; the bytes behind total in
 *                              the last word are written as 0).  The workspace must be the one the scan call left.
 * No atomics, no scratch; a thread owns every word it writes (a word of the bit stream, a word of the payload); the result
 * depends on nothing but the input: bitwise reproducible.  Widths up to GOM_JPEG_MAX_WIDTH = 4096 (the block starts of an
 * interval, 6 per MCU, live in LDS) and heights up to 65535 (SOF0): beyond them GOM_ERR_UNSUPPORTED before any HIP call.
 * GOM_ERR_INVALID_ARG before any HIP call: null pointers, F < 0, H or W < 1, quality outside 1 .. 100, bgr outside {0, 1}, a
 * workspace that is too small or not 256-byte aligned, a payload that is too small or not 4-byte aligned, total < 0 or above
 * what the workspace can hold.  F == 0 is GOM_OK without a launch (frame_off is not written). */
#define GOM_JPEG_MAX_WIDTH 4096
#define GOM_JPEG_MAX_HEIGHT 65535
long gom_jpeg_workspace_bytes(int F, int H, int W);
int gom_jpeg_encode_scan_u8(const uint8_t* frames, int F, int H, int W, int bgr, int quality, void* workspace,
                            long workspace_bytes, int64_t* frame_off, void* stream);
int gom_jpeg_encode_pack_u8(const void* workspace, long workspace_bytes, int F, int H, int W, long total, uint8_t* payload,
                            long payload_bytes, void* stream);
/* ---- JPEG decoding of source frames (csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h; gomatching_amd/jpeg.py; eval --device-decode)
 * File bytes go up, u8 [F,H,W,3] pixels stay in HBM.  THE RULE, in integers only, is libjpeg's published arithmetic, so that the
 * kernels, the numpy path (jpeg.decode_host), the plain-Python statement (tests/jpeg_decode_statement.py) and Pillow's
 * `Image.open(p).convert("RGB")` (libjpeg-turbo: the `islow` IDCT, fancy upsampling) agree byte for byte.  `>>` is the
 * arithmetic shift (floor).
 *   Accepted  : SOF0, 8 bits; one component (sampling 1x1), or three components Y Cb Cr (a JFIF marker, or an Adobe marker with
 *               transform 1, or neither and component ids 1, 2, 3) with luminance sampling (h, v) in {(1,1), (2,1), (2,2)} and
 *               chrominance (1,1); one interleaved scan (Ss 0, Se 63, Ah Al 0); 8-bit DQT; DC and AC Huffman tables 0 and 1 of any
 *               content (DC categories up to 11); any DRI; width up to GOM_JPEG_MAX_WIDTH, height up to 65535.
 *   Refused   : by jpeg.parse on the host, with a reason, before anything is uploaded: SOF1 / SOF2 / lossless / arithmetic
 *               coding, 12 bits, four components, another Adobe transform, any other sampling, several scans, DNL, 16-bit
 *               quantisation tables, a table the scan names but no segment defines, a header cut short.  Pillow reads those.
 *   Geometry  : an MCU is h x v luminance blocks (left to right, top to bottom), then Cb, then Cr; MW = ceil(W / 8h) MCUs a row,
 *               MH = ceil(H / 8v) rows.  Component c has a grid of (MH v_c) x (MW h_c) blocks; coefficients are int16
 *               [frame][component][block of the grid, row-major][64] in natural (row-major) order, planes are u8 of 8 x the grid.
 *   Segments  : the host cuts the entropy-coded segment at every 0xFF 0xD0..0xD7 (a vectorised scan).  Segment s of a frame
 *               holds MCUs [s R, min((s + 1) R, MH MW)) for restart interval R (one segment without DRI) and must be followed
 *               by RSTn with n = s mod 8, the last one by the end of the scan.  Predictors start at 0 in every segment.
 *   Bits      : bytes fill a 32-bit accumulator from the most significant bit; 0xFF 0x00 is the byte 0xFF; any other 0xFF, or
 *               the segment's end, ends the data: zero bits follow, and taking one of them is status 1.
 *   Walk      : per block the DC category (Huffman), its amplitude bits (a value v of s bits with its top bit clear is
 *               v - 2^s + 1), the predictor's sum wrapped to 16 bits; then k = 1: a symbol RS, R = RS >> 4, S = RS & 15:
 *               S > 0: k += R, k > 63 is status 3, else coefficient zigzag[k] = the amplitude, k += 1; S = 0 and R = 15: k += 16
 *               (k > 63 is status 3); S = 0 otherwise: end of block.  A Huffman code is looked up by its first 8 bits, longer ones
 *               by length against the largest code of each length; no code of 16 bits or fewer is status 2.
 *   Status    : per segment 0 = clean, else the first that happened of 1 ran past the segment, 2 invalid code (or a DC category
 *               above 11), 3 coefficient index above 63; a segment walked cleanly is then 5 when whole bytes are left over,
 *               else 4 when the RSTn behind it is wrong or missing (or bytes follow the last segment).  The frame's word is that
 *               of its first segment that is not clean.  The caller sends a flagged file through Pillow.
 *   Dequantise: coefficient x its quantiser (natural order).
 *   IDCT      : jidctint.c, CONST_BITS 13, PASS1_BITS 2, constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995
 *               25172 (FIX(0.298631336) .. FIX(3.072711026)).  One pass over d0 .. d7:
 *                 z1 = (d2 + d6) 4433; t2 = z1 - d6 15137; t3 = z1 + d2 6270; t0 = (d0 + d4) << 13; t1 = (d0 - d4) << 13
 *                 e0 = t0 + t3; e3 = t0 - t3; e1 = t1 + t2; e2 = t1 - t2
 *                 o0 = d7; o1 = d5; o2 = d3; o3 = d1; z1 = o0 + o3; z2 = o1 + o2; z3 = o0 + o2; z4 = o1 + o3; z5 = (z3 + z4) 9633
 *                 o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z5 - z3 16069; z4 = z5 - z4 3196
 *                 o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4
 *                 out 0..7 = e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3, each (x + 2^(n-1)) >> n
 *               down the columns with n = 11, then along the rows with n = 18; sample = clamp(value + 128, 0, 255).  (libjpeg's
 *               shortcut for a column without AC terms gives the same value.)  32-bit accumulators.
 *   Upsample  : a chrominance plane has ch = ceil(H / v) rows of cw = ceil(W / h) real samples.  h = 1: none.  cw <= 2:
 *               replication (libjpeg switches the triangle filter off there).  Otherwise, with c the sample over the pixel
 *               (row y >> 1 for v = 2, column x >> 1) and the neighbour index clamped into the real samples:
 *                 h2v1: odd x: (3 c + right + 2) >> 2, even x: (3 c + left + 1) >> 2
 *                 h2v2: s(column) = 3 c + (the row below for odd y, above for even y); odd x: (3 s + s(right) + 7) >> 4,
 *                       even x: (3 s + s(left) + 8) >> 4
 *   Colour    : with cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768)
 *               >> 16), B = Y + ((116130 cb + 32768) >> 16), each clamped to 0 .. 255.  One component: R = G = B = Y.
 * What the host uploads (jpeg.plan): the files' entropy bytes packed; per segment GOM_JPEG_DECODE_DESC_WORDS int64: first byte,
 * end (the marker excluded), the end of its frame's bytes, first MCU, MCUs, frame, table set, the RSTn byte expected behind it
 * (0: the frame's end); seg_off int32 [F+1]; the distinct table sets, GOM_JPEG_DECODE_SET_WORDS int32 each: four Huffman
 * tables (DC 0, DC 1, AC 0, AC 1) of 548 words (look[256] = length << 8 | symbol by the first 8 bits, maxcode[18], valoff[18],
 * huffval[256]), the DC table (0, 1) of components 0..3, the AC table (2, 3) of components 0..3, the quantisers [3][64].
 * All of it is data the device does not trust: every byte read is bounded by the segment's end, every offset, MCU, frame and
 * table index is checked or clamped before use, every coefficient and block index before the store.
 *   gom_jpeg_decode_workspace_bytes : coefficients (128 bytes a block) + planes (64 bytes a block), or -1 for sizes it refuses.
 *   gom_jpeg_decode_entropy_i16     : a wavefront per segment: lane 0 walks the bits into LDS, the 64 lanes store the block's
 *                                     coefficients as one 128-byte row (which also zero-fills it); then a launch that folds
 *                                     seg_status int32 [nseg] into frame_status int32 [F].
 *   gom_jpeg_decode_pixels_u8       : dequantise + IDCT into planes (8 lanes a block), then upsampling + colour into out u8
 *                                     [F,H,W,3] (bgr = 1: B G R); a thread owns four pixels (three 32-bit words).
 * No atomics, no scratch, one writer per output byte: bitwise reproducible.  GOM_ERR_UNSUPPORTED before any HIP call: W above
 * GOM_JPEG_MAX_WIDTH, H above GOM_JPEG_MAX_HEIGHT, components or sampling outside the accepted set.  GOM_ERR_INVALID_ARG: null
 * pointers, negative counts, a workspace too small or not 256-byte aligned, bgr outside {0, 1}.  F == 0: GOM_OK, no launch. */
#define GOM_JPEG_DECODE_DESC_WORDS 8
#define GOM_JPEG_DECODE_SET_WORDS 2392
long gom_jpeg_decode_workspace_bytes(int F, int H, int W, int ncomp, int hs, int vs);
int gom_jpeg_decode_entropy_i16(const uint8_t* bytes, long nbytes, const int64_t* desc, int nseg, const int32_t* seg_off,
                                const int32_t* sets, int nsets, int F, int H, int W, int ncomp, int hs, int vs, void* workspace,
                                long workspace_bytes, int32_t* seg_status, int32_t* frame_status, void* stream);
int gom_jpeg_decode_pixels_u8(const int32_t* sets, int nsets, const int32_t* frame_set, int F, int H, int W, int ncomp, int hs,
                              int vs, int bgr, void* workspace, long workspace_bytes, uint8_t* out, void* stream);
/* ---- The chunked entropy walk (csrc/jpeg_decode_chunks.h, csrc/jpeg_decode.hip; tools/jpeg_decode_chunks_hostcheck.cpp)
 * gom_jpeg_decode_entropy_i16 with many lanes per segment, for files without restart markers (one segment a file).  Huffman codes
 * are self-synchronising: a walk begun at a wrong place falls into step with the true one.  THE RULE:
 *   Chunks    : a segment's stuffed bytes [start, end) are cut every chunk_bytes (a power of two in 16 .. 4096) counted from
 *               start rounded down to 4 (the staging loads whole words), so chunk 0 may be up to 3 bytes short.
 *   State     : at a symbol boundary, everything the rest of the walk depends on: the stuffed byte that holds the next unread bit
 *               and the bits of it already read (0xFF 0x00 is one byte, named by its 0xFF), the block slot within the MCU
 *               (0 .. hs vs + 1; 0 for one component), the zigzag index (0: a DC symbol is next).  Not in it: the DC predictors
 *               and the count of blocks, which are sums and are scanned.  A chunk's exit state is the state at the first symbol
 *               boundary at or behind its end; it is the next chunk's entry.
 *   Span      : min(256, 65536 / chunk_bytes) consecutive chunks, a lane each, settled together; a workgroup takes the spans of
 *               a segment in order, the exit of a span's last chunk being the next span's true entry.  Per span:
 *               (a) cold walk: a lane walks its chunk from a guess -- its first bit (a 0x00 behind the previous chunk's 0xFF is
 *                   skipped), slot 0, index 0; chunk 0 from the true entry.  For a guess an invalid code costs one bit, a DC
 *                   category is taken mod 16, an index above 63 ends the block: no error, the guess is discarded unless it was true.
 *               (b) settling: lane i takes lane i - 1's exit as its entry; where that differs from the entry it last walked from,
 *                   it walks again; until no entry changed.  After pass p the first p + 1 chunks are exact, so at most 256 passes,
 *                   the loop's constant bound.  Equal entries give equal walks: the result is exactly the serial walk's.
 *               (c) totals: the walk also counts the blocks that begin in the chunk (a block belongs to the chunk that holds its
 *                   first bit) and sums their DC differences per component;
 *               (d) which are scanned exclusively over the span, with the carry of the spans before, in 32 bits (the stored DC
 *                   wraps to 16 bits as in the serial walk);
 *               (e) write walk: from the true entry, first block ordinal and predictors a lane stores the coefficients of the
 *                   blocks that begin in its chunk, walking behind the chunk's end to finish the last; ordinal o is slot
 *                   o mod (blocks of an MCU) of MCU first + o / (blocks of an MCU), at the serial walk's block index.
 *   End       : the walk ends with the last block of the segment's MCUs; what lies behind is judged as in the serial walk
 *               (left-over bytes, the RSTn that must follow).  What no walk stores is zero (cleared in front).
 *   Route     : anything but a clean walk is not this kernel's business: a status other than 0 in a write walk, blocks that do
 *               not add up to the segment's MCUs, a closing check other than 0 mark the segment, seg_info[s][0] = 1, and leave its
 *               coefficients unspecified.  The block count is held through the closing check: the check is made by the lane
 *               that ends block (MCUs x blocks of an MCU) - 1 and a segment nobody closed is marked, which catches too few
 *               blocks; no write walk begins a block of a higher ordinal, and bytes that would hold more are left over (status
 *               5), which catches too many.  (The counts of sub-step (c) may run past the last block into the padding bits;
 *               they only number the blocks.)  Behind the chunk launch, in the same call, gom_jpeg_decode_entropy_i16's kernel runs
 *               over all segments, returns at once for those with route 0 and walks the marked ones as it always does: a damaged
 *               stream has exactly the serial walk's status words and coefficients.  seg_info[s][1] = the most settling passes
 *               of one of its spans (0 for a segment marked before any walk).
 * One writer per coefficient, no atomics, no scratch; bitwise reproducible, and independent of chunk_bytes, the span and the pass
 * count.  Same workspace and status words as gom_jpeg_decode_entropy_i16, so gom_jpeg_decode_pixels_u8 follows unchanged.
 * GOM_ERR_INVALID_ARG before any launch: as there, and a chunk_bytes that is no power of two in 16 .. 4096, a null seg_info.
 * GOM_JPEG_DECODE_CHUNK_BYTES: the default, and GOM_JPEG_DECODE_AUTO_SEGMENT_BYTES: the mean segment length from which
 * jpeg.decode_device(walk="auto") takes this walk -- both measured (profiles/jpeg_decode_chunks_bench.log, 100 files of 1280 x
 * 720): without restart markers the entropy launch takes 38.3 / 24.4 / 16.7 / 22.1 / 35.7 ms at chunks of 64 / 128 / 256 / 512 /
 * 1024 bytes against 143.8 ms for the segment walk, so 256; the segment walk wins at segments of 4 061 bytes in the mean (7.7 ms
 * against 19.6 at best) and loses at 30 459 (27.7 ms against 8.9 .. 9.3), so 16 384, between the two. */
#define GOM_JPEG_DECODE_CHUNK_BYTES 256
#define GOM_JPEG_DECODE_AUTO_SEGMENT_BYTES 16384
int gom_jpeg_decode_entropy_chunks_i16(const uint8_t* bytes, long nbytes, const int64_t* desc, int nseg, const int32_t* seg_off,
                                       const int32_t* sets, int nsets, int F, int H, int W, int ncomp, int hs, int vs,
                                       void* workspace, long workspace_bytes, int32_t* seg_status, int32_t* frame_status,
                                       int chunk_bytes, int32_t* seg_info, void* stream);
int gom_maxpool3x3s2_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
/* out [H*W, 256] = PositionalEncoding2D(normalize=True) + level_embed, for an unpadded H x W level. */
int gom_pos_encoding_2d_f32(const float* dim_t128, const float* level_embed256, float* out, int H, int W,
                            void* stream);
int gom_point_pos_embed_f32(const float* pts, const float* dim_t128, float* out, long num_points, void* stream);
/* out[q,c] = sigmoid(delta[q*ld_delta + c] + inverse_sigmoid(ref[q, c%2])), C in {2,4}. */
int gom_ref_sigmoid_f32(const float* delta, int ld_delta, const float* ref, float* out, long num_points, int C,
                        void* stream);
/* Reference refinement of a decoder layer + the next layer's point position embedding in one launch
 * (deformable_transformer.py:484-488, :470-473): new_ref[q] = sigmoid(h[q] . W3^T + b3 + inverse_sigmoid(ref[q])),
 * W3 [2,256]; pos [Q,256] (may be NULL) = gom_point_pos_embed_f32 of new_ref * (sx, sy). */
int gom_ref_update_f32(const float* h, int ld_h, const float* W3, const float* b3, const float* ref,
                       const float* dim_t128, float sx, float sy, float* new_ref, float* pos, long num_points,
                       void* stream);
int gom_proposal_valid(const int64_t* spatial_shapes, const int64_t* level_start_index, int num_levels,
                       unsigned char* valid, long S, void* stream);
int gom_encoder_reference_points(const int64_t* spatial_shapes, const int64_t* level_start_index, int num_levels,
                                 float* ref, long S, void* stream);
/* coord_raw: [B,S,8] indexed by token (compact = 0) or [B*num_queries,8] rows of the selected tokens (compact = 1). */
int gom_bezier_reference_points(const float* coord_raw, const int* topk_idx, const int64_t* spatial_shapes,
                                const int64_t* level_start_index, int num_levels, const float* bernstein, float* refs,
                                int B, long S, int num_queries, int num_points, int compact, void* stream);
/* A18: in-place (x, y) pair scaling, detector_postprocess gom_lstmatcher.py:100-109. */
int gom_scale_xy_f32(float* x, long n_pairs, float sx, float sy, void* stream);
int gom_add_f32(const float* a, const float* b, float* out, long n, void* stream);
/* *flag |= 1 when any of x[0..n) is Inf / NaN: the result check of the bf16x6 / exact-fp32 back-ends, whose GEMM kernels carry
 * no range flag (the reference lets a non-finite activation flow on silently, gom_lstmatcher.py:268-351; here it raises). */
int gom_flag_nonfinite_f32(const float* x, long n, int* flag, void* stream);
/* dst[i] = src[i] over 32-bit words, as a kernel; src may be pinned host memory (device-mapped). */
int gom_copy_words(const void* src, void* dst, long n_words, void* stream);
int gom_broadcast_rows_f32(const float* src, float* out, long n, int B, void* stream);

/* top-k token indices per batch element (deformable_transformer.py:188-190); idx_out [B,k] int32, sorted by
 * logit descending; rows_out (optional) [B,k] = b*S + idx.  valid/invalid_logit (optional): tokens with valid[s]==0 take *invalid_logit. */
int gom_topk_set_lean(int on);   /* [host] 1 (default): k-bounded chunk sort (k <= 128), merge network sized by the candidates; same result */
long gom_topk_workspace_bytes(int B, long S, int k);
int gom_topk_tokens(const float* logits, int ld, const unsigned char* valid, const float* invalid_logit, int B, long S,
                    int k, void* workspace, int* idx_out, int* rows_out, void* stream);

/* ---- A11/A12: detection() + NMS + foreground filter ---------------------------------------------------*/
/* out[r] = index of the first maximum of x[r, 0..V), always in [0, V): 0 for a constant row (all -inf too);
 * NaN elements never win, and a row of nothing but NaN gives 0. */
int gom_argmax_rows_f32(const float* x, int ld, int V, long rows, int* out, void* stream);
/* Per frame b: count[b] kept instances, in NMS (descending score) order, written to the first count[b] slots of
 * the nq-padded outputs: keep_idx (row into [B*nq]), scores, boxes [.,4] px, ctrl_out [.,P,2] px,
 * bd_out [.,P,4] px, recs_out [.,P] int64. */
int gom_detect_post(const float* cls_logits, int ld_cls, const float* rescoring_logits, int ld_rescoring,
                    const float* ctrl_points, const float* bd_points, const int* recs, int B, int num_queries,
                    int num_points, float img_h, float img_w, float det_thresh, float nms_thresh, float asso_thresh,
                    int* count, int* keep_idx, float* scores, float* boxes, float* ctrl_out, float* bd_out,
                    long long* recs_out, void* stream);

/* ---- padded batches (gom_lstmatcher.py:63-76; deformable_transformer.py:141-148): every level's valid region is a
 * top-left rectangle valid_shapes [L][2] = (Hv, Wv) of its (H, W).  Mask-aware forms of the geometry tables, the fused
 * MSDA (reference points scaled by the level's valid ratio [L][2] = (Wv/W, Hv/H)) and the value zero-fill. */
int gom_pos_encoding_2d_valid_f32(const float* dim_t128, const float* level_embed256, float* out, int H, int W, int valid_h,
                                  int valid_w, void* stream);
int gom_proposal_valid_masked(const int64_t* spatial_shapes, const int64_t* level_start_index, int num_levels,
                              const int64_t* valid_shapes, unsigned char* valid, long S, void* stream);
int gom_encoder_reference_points_masked(const int64_t* spatial_shapes, const int64_t* level_start_index,
                                        const int64_t* valid_shapes, int num_levels, float* ref, long S, void* stream);
int gom_bezier_reference_points_masked(const float* coord_raw, const int* topk_idx, const int64_t* spatial_shapes,
                                       const int64_t* level_start_index, const int64_t* valid_shapes, int num_levels,
                                       const float* bernstein, float* refs, int B, long S, int num_queries, int num_points,
                                       int compact, void* stream);
int gom_msda_fused_forward_vr(const float* raw, int ld_raw, const float* ref, const float* value, long value_batch_stride,
                              int value_row_stride, const int64_t* spatial_shapes, const int64_t* level_start_index,
                              const float* valid_ratios, float* output, int batch, int num_query, void* stream);
/* zero columns [col0, col0+ncols) of the rows of buf [B*S, ld] whose token lies outside its level's valid region
 * (value.masked_fill(padding_mask, 0), ms_deform_attn.py:134-135). */
int gom_zero_padded_tokens_f32(float* buf, int ld, int col0, int ncols, const int64_t* spatial_shapes,
                               const int64_t* level_start_index, const int64_t* valid_shapes, int num_levels, int B, long S,
                               void* stream);

/* ---- padded batches whose frames have their OWN valid extents (a motion clip made from a still: one padded size, a valid
 * rectangle per frame).  Descriptors live on the device: valid_shapes [B][L][2] int64 (Hv, Wv), valid_ratios [B][L][2] fp32
 * (Wv/W, Hv/H), scales [B][2] fp32 (sx, sy), sizes [B][2] fp32 (img_h, img_w).  Each form computes, for frame b, what the
 * single-extent entry above computes for a batch of that frame alone -- the same arithmetic, operand for operand. */
/* ONE launch for the three geometry tables of all B frames and L levels: lvl_pos [B,S,256] (gom_pos_encoding_2d_valid_f32 +
 * level_embed [L][256]), ref [B,S,2] (gom_encoder_reference_points_masked), valid [B,S] (gom_proposal_valid_masked). */
int gom_padded_geometry_f32(const float* dim_t128, const float* level_embed, const int64_t* spatial_shapes,
                            const int64_t* level_start_index, const int64_t* valid_shapes, int num_levels, int B, long S,
                            float* lvl_pos, float* ref, unsigned char* valid, void* stream);
int gom_zero_padded_tokens_frames_f32(float* buf, int ld, int col0, int ncols, const int64_t* spatial_shapes,
                                      const int64_t* level_start_index, const int64_t* valid_shapes, int num_levels, int B,
                                      long S, void* stream);
/* gom_topk_tokens with a validity row per frame: valid [B][S] (required). */
int gom_topk_tokens_frames(const float* logits, int ld, const unsigned char* valid, const float* invalid_logit, int B, long S,
                           int k, void* workspace, int* idx_out, int* rows_out, void* stream);
int gom_bezier_reference_points_frames(const float* coord_raw, const int* topk_idx, const int64_t* spatial_shapes,
                                       const int64_t* level_start_index, const int64_t* valid_shapes, int num_levels,
                                       const float* bernstein, float* refs, int B, long S, int num_queries, int num_points,
                                       int compact, void* stream);
int gom_msda_fused_forward_vr_frames(const float* raw, int ld_raw, const float* ref, const float* value,
                                     long value_batch_stride, int value_row_stride, const int64_t* spatial_shapes,
                                     const int64_t* level_start_index, const float* valid_ratios, float* output, int batch,
                                     int num_query, void* stream);
/* pair i takes scales[i / pairs_per_frame]; point q takes scales[q / points_per_frame]. */
int gom_scale_xy_frames_f32(float* x, long n_pairs, const float* scales, long pairs_per_frame, void* stream);
int gom_ref_update_frames_f32(const float* h, int ld_h, const float* W3, const float* b3, const float* ref,
                              const float* dim_t128, const float* scales, long points_per_frame, float* new_ref, float* pos,
                              long num_points, void* stream);
int gom_detect_post_sizes(const float* cls_logits, int ld_cls, const float* rescoring_logits, int ld_rescoring,
                          const float* ctrl_points, const float* bd_points, const int* recs, int B, int num_queries,
                          int num_points, const float* sizes, float det_thresh, float nms_thresh, float asso_thresh,
                          int* count, int* keep_idx, float* scores, float* boxes, float* ctrl_out, float* bd_out,
                          long long* recs_out, void* stream);

/* ---- f3: Swin-T backbone glue (third_party/adet/modeling/swin/swin_transformer.py) ---------------------------------
 * The linear layers use the GEMM entry points above.  Tokens are [B,H,W,C] channels-last.  Window rows are ordered
 * (image, window row, window column, token 0..48), windows of 7x7 over the map zero-padded to multiples of 7. */
int gom_layernorm_any_f32(const float* x, const float* gamma, const float* beta, float* out, long rows, int dim, float eps,
                          void* stream);                                                /* dim % 4 == 0, <= 2048 */
int gom_gelu_f32(float* x, long n, void* stream);                                         /* in place, exact erf form */
/* PatchEmbed input (:473-479): image [B,H,W,4] -> rows [B*ceil(H/4)*ceil(W/4), 64] in (kh, kw, c) order, zero padded. */
int gom_swin_patchify_f32(const float* img, float* out, int B, int H, int W, void* stream);
/* pad + cyclic shift (-shift) + window_partition (:246-262) and its inverse fused with the residual add (:264-279). */
int gom_swin_window_gather_f32(const float* x, float* out, int B, int H, int W, int C, int shift, void* stream);
int gom_swin_window_scatter_add_f32(const float* windows, const float* shortcut, float* out, int B, int H, int W, int C,
                                    int shift, void* stream);
/* PatchMerging gather (:320-327): [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),4C]. */
int gom_swin_patch_merge_f32(const float* x, float* out, int B, int H, int W, int C, void* stream);
/* WindowAttention core (:139-165): qkv [num_windows*49, 3C] -> out [num_windows*49, C]; bias [heads,49,49]; mask
 * [windows_per_image,49,49] (0 / -100) or NULL; head_dim 32. */
int gom_swin_window_attention_f32(const float* qkv, float* out, const float* bias, const float* mask, long num_windows,
                                  int windows_per_image, int heads, int C, void* stream);

/* ---- f3: ViTAEv2-S backbone glue (third_party/adet/modeling/vitae_v2/) ----------------------------------------------
 * Linear layers, dense convolutions and the two products of the full attention use the GEMM entry points above. */
/* x [B,H,W,C] -> rows [B*OH*OW, ldo], columns (kh, kw, c) then zeros up to ldo: feeds the dilated strided convolutions
 * of the pyramid reduction module (PRM, ReductionCell.py:27-34,55-62) to a GEMM.  C % 4 == 0, ldo % 4 == 0. */
int gom_im2col_nhwc_f32(const float* x, float* out, int B, int H, int W, int C, int KH, int KW, int stride, int pad,
                        int dilation, int ldo, void* stream);
/* grouped 3x3 convolution, padding 1 (PCM, ReductionCell.py:97-105 / NormalCell.py:137-145): w [3,3,Cout,Cin/groups]
 * with Cin/groups in {4,16}; y = act(conv*scale + shift) + R; scale / R may be NULL; act 0 none, 3 SiLU. */
int gom_grouped_conv3x3_nhwc_f32(const float* x, const float* w, const float* scale, const float* shift, const float* R,
                                 int act, float* y, int B, int H, int W, int Cin, int Cout, int groups, int stride,
                                 void* stream);
int gom_silu_f32(float* x, long n, void* stream);                                         /* in place, n % 4 == 0 */
/* centred zero padding to multiples of 7 + window_partition, and window_reverse + crop (+ up to two addends of the token
 * shape, NULL to skip) (ReductionCell.py:147-163, NormalCell.py:160-211). */
int gom_vitae_window_gather_f32(const float* x, float* out, int B, int H, int W, int C, void* stream);
int gom_vitae_window_crop_f32(const float* windows, const float* R1, const float* R2, float* out, int B, int H, int W, int C,
                              void* stream);
/* WindowAttention core without position bias / mask (window.py:92-124): qkv [num_windows*49, 3C] -> out
 * [num_windows*49, C]; head_dim C/heads in {64,128}. */
int gom_vitae_window_attention_f32(const float* qkv, float* out, long num_windows, int heads, int C, void* stream);
/* in place x[r, :cols] = softmax(x[r, :cols] * scale), cols <= 8192 (full attention, NormalCell.py:52-54). */
int gom_softmax_rows_scaled_f32(float* x, long rows, int cols, long ld, float scale, void* stream);
/* out[c*ldo + r] = x[r*ld + c]. */
int gom_transpose_f32(const float* x, float* out, int rows, int cols, long ld, long ldo, void* stream);
/* Full self-attention with the scores kept on the CU (NormalCell.py:46-58 / token_transformer.py:27-44):
 * out[b*N + i, h*hd : (h+1)*hd] = softmax_j(q_i . k_j / sqrt(hd)) v_j over the N tokens of image b, for every head h.
 * q, k, v point at column 0 of their first head inside row-strided fp32 buffers (row stride ld, e.g. a fused qkv buffer
 * with q = qkv, k = qkv + C, v = qkv + 2C); hd in {64, 128}; products on the fp16 matrix cores with the f16x3 split
 * (operands within +-65504; a non-finite output sets *flag, which may be NULL). */
int gom_flash_attention_f32(const float* q, const float* k, const float* v, float* out, int batch, int N, int heads,
                            int head_dim, int ld, int ldo, int* flag, void* stream);

/* ---- A14/A15: tracker ---------------------------------------------------------------------------------*/
int gom_gather_rows_f32(const float* src, const int* rows, float* out, int n, int dim, void* stream);
/* per-frame softmax with an appended zero logit (lstmatcher.py:373-381); frame_offsets [num_frames+1] int32. */
int gom_asso_activate_f32(const float* logits, int ld, const int* frame_offsets, int num_frames, int n_k, float* out,
                          int ld_out, void* stream);
/* traj[n_k, M] (gom_lstmatcher.py:429-445 / 510-547).  meta int32: nonk[Np] | col_of[Np] | last_idx[M] | k_inds[n_k];
 * boxes [N,4] in pixels of the network input (img_w x img_h). */
int gom_track_score_f32(const float* act, int ld, const int* meta, const float* decay, const float* boxes, float img_w,
                        float img_h, int n_k, int Np, int M, int with_iou, float max_center_dist, float* traj,
                        void* stream);
/* gom_asso_activate_f32 + gom_track_score_f32 of one match as ONE launch (same values; Np + n_k <= 16 384). */
int gom_asso_score_f32(const float* logits, int ld, const int* frame_offsets, int num_frames, const int* meta,
                       const float* decay, const float* boxes, float img_w, float img_h, int n_k, int Np, int M,
                       int with_iou, float max_center_dist, float* traj, void* stream);
/* Short-term matching for ALL (previous, current) frame pairs of a clip in one launch: per current detection i of pair
 * p, q.k^T logits against the previous frame's rows, softmax with the zero background logit (lstmatcher.py:373-381) and
 * S[i,j] = max(a_j, IoU(i,j)) (gom_lstmatcher.py:429-445 for tracks seen once).  pairs [device] int32 [P][6] =
 * (first memory row, n_prev, n_cur, first tgt row, first box row, offset of the pair's [n_cur, n_prev] block in S);
 * row_pair [total_cur_rows]; boxes [rows,4] px in memory-row order; max_prev <= 320. */
int gom_short_term_pairs_f32(const float* tgt, const float* memory, int d, const int* pairs, const int* row_pair,
                             const float* boxes, float img_w, float img_h, int with_iou, int total_cur_rows, int max_prev,
                             float* S, void* stream);
/* [host runtime] The whole device chain of one association match -- gather of the window's embeddings, the matcher
 * transformer (roi_heads/transformer.py:60-96: n_enc post-norm encoder layers over all N rows, n_dec cross-attention
 * decoder layers for the query rows [lo, hi), norms Identity), q.k^T logits, `_activate_asso` (lstmatcher.py:373-381)
 * and the trajectory score (gom_lstmatcher.py:429-445 / 510-547) -- queued on `stream` by ONE call.  Replaces ~18
 * per-kernel FFI crossings of the launch-bound tracker recurrence.  Layer weights are nn.MultiheadAttention / Linear
 * tensors as stored in the checkpoint (in_w [3d,d], out_w [d,d], lin1_w [ffn,d], lin2_w [d,ffn]; lin* NULL for the
 * cross-attention-only decoder of SHA_FFN_CRSATTN).  workspace: device floats, gom_match_workspace_floats(...).
 * traj [hi-lo, num_tracks] device. */
typedef struct gom_matcher_layer {
    const float* in_w;
    const float* in_b;
    const float* out_w;
    const float* out_b;
    const float* lin1_w;
    const float* lin1_b;
    const float* lin2_w;
    const float* lin2_b;
} gom_matcher_layer;
long gom_match_workspace_floats(int N, int n_k, int d, int ffn);
/* [device] one launch for a match with hoisted projections: src [N, dim] <- pool[rows], qkv [N, 3 dim] <- proj[rows][0 : 3 dim],
 * qdec [n_k, dim] <- proj[rows[lo .. lo + n_k)][3 dim : 4 dim]. */
int gom_gather_match_f32(const float* pool, int ld_pool, const float* proj, int ld_proj, const int* rows, int N, int lo, int n_k,
                         int dim, float* src, float* qkv, float* qdec, void* stream);
/* gom_match_scores_f32 with the two per-row projections of the raw embeddings hoisted out of the chain: proj [pool rows,
 * ld_proj >= 4 d] = (encoder layer 0 in-projection | decoder layer 0 query projection) of every pool row, computed once per
 * detection by gom_gemm_small_f32 (same bits as in the chain).  proj == NULL: gom_match_scores_f32. */
int gom_match_scores_proj_f32(const float* pool, int ld_pool, const float* proj, int ld_proj, const int* rows,
                              const int* frame_offsets, const int* meta, const float* boxes, const float* decay, int N, int T,
                              int lo, int hi, int num_tracks, const gom_matcher_layer* enc, int n_enc,
                              const gom_matcher_layer* dec, int n_dec, int d, int heads, int ffn, float img_w, float img_h,
                              int with_iou, float max_center_dist, float* workspace, long workspace_floats, float* traj,
                              void* stream);
int gom_match_scores_f32(const float* pool, int ld_pool, const int* rows, const int* frame_offsets, const int* meta,
                         const float* boxes, const float* decay, int N, int T, int lo, int hi, int num_tracks,
                         const gom_matcher_layer* enc, int n_enc, const gom_matcher_layer* dec, int n_dec, int d,
                         int heads, int ffn, float img_w, float img_h, int with_iou, float max_center_dist,
                         float* workspace, long workspace_floats, float* traj, void* stream);
/* [host + device] The per-frame id recurrence of GoMatching.track_frames for all frames of a call behind ONE crossing
 * (tracker_rt.hip; gom_lstmatcher.py:366-564): short-term assignment from precomputed score matrices, long-term match
 * (selection, descriptors, gom_match_scores_f32, LSA, thresholds, id allocation).  Host arrays in, ids out; see the
 * comment above gom_tracker_run in tracker_rt.hip for the layout.  The handle owns its device / pinned scratch. */
void* gom_tracker_create(int test_len, float overlap_thresh, int not_mult_thresh, int use_decay, int with_iou,
                         float max_center_dist, const gom_matcher_layer* enc, int n_enc, const gom_matcher_layer* dec,
                         int n_dec, int d, int heads, int ffn);
void gom_tracker_destroy(void* tracker);
/* [host] hoisted projections (gom_match_scores_proj_f32) for the NEXT gom_tracker_run call only; NULL = none. */
int gom_tracker_set_projections(void* tracker, const float* proj_dev, int ld_proj);

int gom_tracker_run(void* tracker, int F, const int* n, const float* boxes, const int* rows, long* ids, int first_new,
                    long first_real, const float* S, const long* s_off, const float* pool_dev, int ld_pool, float img_w,
                    float img_h, const float* decay_table, long* id_count_io, double* secs, void* stream);
/* The same with one image size PER window frame (frame_wh [F, 2] = width, height): a long-term match then normalises every box
 * of its window by the size of the window's FIRST frame, as the reference does (gom_lstmatcher.py:471 builds every window
 * Instances with full_instances[0].image_size; lstmatcher.py:478-494 divides by it) -- clips that mix resolutions (BOVText). */
int gom_tracker_run_wh(void* tracker, int F, const int* n, const float* boxes, const int* rows, long* ids, int first_new,
                       long first_real, const float* S, const long* s_off, const float* pool_dev, int ld_pool,
                       const float* frame_wh, const float* decay_table, long* id_count_io, double* secs, void* stream);
/* ---- CU-partitioned streams (csrc/stream.hip): the tracker's lane of a multi-GPU step ------------------------------------
 * [host] A HIP stream whose kernels run only on the compute units of cu_mask (`words` x 32 bits, bit i = CU i of the driver's
 * enumeration).  GoMatching.reserve_tracker_cus() gives the tracker stream a few CUs of every XCD and the detector stream the
 * rest, so that the tracker's small dependent launches never queue behind the detector's resident workgroups. */
int gom_stream_create_cu_mask(const unsigned* cu_mask, int words, void** stream_out);
int gom_stream_destroy(void* stream);

/* [host] rectangular assignment, SciPy-compatible tie-breaking (gom_lstmatcher.py:447,549).  Returns the number
 * of assigned pairs (min(nr,nc)) or a negative error. */
int gom_linear_sum_assignment(const double* cost, long nr, long nc, long* row_ind, long* col_ind);

/* Multi-GPU exchange: one launch packs a step's detections into the all-gather buffer [frames, nq + 1, D]
 * fp32, D = feature_dim + 4 + 1 + 2 P + 4 P + P: row 0 of a frame = (count, image height, image width, 0...), rows 1..count =
 * reid | box | score | ctrl | bd | recs, the rest zero.  The re-id rows of frame f start at pool row
 * row_base + sum(counts[0..f)); boxes / scores / ctrl / bd / recs are the nq-padded arrays of gom_detect_post. */
int gom_pack_records_f32(const float* pool, int ld_pool, int row_base, const int* counts, const float* boxes,
                         const float* scores, const float* ctrl, const float* bd, const long* recs, int frames, int nq,
                         int feature_dim, int num_points, float img_h, float img_w, float* out, void* stream);

/* Training of the association head (only `roi_heads` trains, freeze_layers.py:20-37) -- the pieces that are
 * not contractions (those run on gom_gemm_f32 with transposed operands, gomatching_amd/training.py):
 *   gom_relu_backward_f32          dx = y > 0 ? dy : 0
 *   gom_softmax_rows_backward_f32  dS = scale * P * (dP - rowsum(dP * P))                     (attention backward)
 *   gom_asso_ce_f32                detr_asso_loss's per-frame cross entropy with a zero background logit (lstmatcher.py:
 *                                  436-475): per (row, frame) loss and / or dlogits = *grad_scale * (softmax - onehot);
 *                                  gt[row*T + t] = target index inside frame t, n_t = background, < 0 = pair not counted
 *   gom_sigmoid_focal_f32          loss_res's sigmoid focal loss per element (lstmatcher.py:237-268) and / or d loss / d x */
int gom_relu_backward_f32(const float* dy, const float* y, float* dx, long n, void* stream);
int gom_softmax_rows_backward_f32(const float* P, const float* dP, float* dS, long rows, int cols, long ld, float scale,
                                  void* stream);
int gom_asso_ce_f32(const float* logits, int ld, const int* frame_offsets, int num_frames, const int* gt, long rows,
                    float* loss, const float* grad_scale, float* dlogits, void* stream);
int gom_sigmoid_focal_f32(const float* x, const float* target, float alpha, float gamma, long n, float* loss, float* dx,
                          void* stream);

/* Training-mode dropout of that head (MODEL.ASSO_HEAD.DROPOUT; csrc/dropout.hip).  torch's semantics -- keep with probability
 * 1 - p, kept values times 1 / (1 - p), the backward uses the forward's mask -- on a counter-based mask stream, so that nothing
 * is stored and the backward regenerates the mask:
 *   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (e >> 2, site, iteration, rank) for LOGICAL element e, which
 *   uses output word e & 3 and is kept iff word >= threshold;  e = row * cols + col of the logical [rows, cols] tensor,
 *   whatever the leading dimensions, padding columns and pointer alignment (16-byte accesses where those allow, 4-byte ones
 *   otherwise: the same bits).  e >> 2 must stay below 2^32.
 * The host forms threshold = floor(p * 2^32) (in double) and scale = (float)(1.0 / (1.0 - p)) once; a pair that is not that of
 * one p in [0, 1), a null pointer or a negative size -> GOM_ERR_INVALID_ARG before any HIP call.  Launches only, no atomics.
 *   gom_dropout_f32                 y = [r +] mask * scale * x over [rows, cols] views (r may be NULL; y may be x).  Serves the
 *                                   backward as well: dx = mask * scale * dy.
 *   gom_relu_backward_scaled_f32    dx = y > 0 ? dy * scale : 0 -- ReLU's backward behind a dropout whose OUTPUT y was saved
 *   gom_softmax_dropout_rows_f32    x [rows, ld] in place: P = softmax(scale_qk * x[:, :cols]) with the bits of
 *                                   gom_softmax_rows_scaled_f32, and pd[:, :cols] = mask * scale * P; row r covers logical
 *                                   elements elem0 + r * cols ...; columns cols..ld of pd are not written.  cols <= 8192.
 *   gom_softmax_dropout_rows_backward_f32   dS = scale_qk * P * (G - rowsum(G * P)), G = mask * scale * dPd (the gradient of
 *                                   the DROPPED weights; the mask is applied inside); columns cols..ld of dS are not written */
int gom_dropout_f32(const float* x, long ldx, const float* r, long ldr, float* y, long ldy, long rows, long cols,
                    unsigned long long seed, unsigned site, unsigned iteration, unsigned rank, long threshold, float scale,
                    void* stream);
int gom_relu_backward_scaled_f32(const float* dy, const float* y, float* dx, long n, float scale, void* stream);
int gom_softmax_dropout_rows_f32(float* x, float* pd, long rows, int cols, long ld, float scale_qk, long elem0,
                                 unsigned long long seed, unsigned site, unsigned iteration, unsigned rank, long threshold,
                                 float scale, void* stream);
int gom_softmax_dropout_rows_backward_f32(const float* P, const float* dPd, float* dS, long rows, int cols, long ld,
                                          float scale_qk, long elem0, unsigned long long seed, unsigned site,
                                          unsigned iteration, unsigned rank, long threshold, float scale, void* stream);

/* The optimizer step of that training (csrc/optim.hip): AdamW with FULL-MODEL gradient clipping over a table of fp32 tensors,
 * the fp32 arithmetic of the reference's FullModelGradientClippingOptimizer(torch.optim.AdamW) (costom_solver.py:55-73):
 *   total = || all gradients ||_2 ;  coef = min(1, clip_value / (total + 1e-6))  (clip_value <= 0: coef = 1) ;  g' = coef g ;
 *   per tensor, with ITS step count t, lr and weight_decay:  p *= 1 - lr wd ;  m = m + (1 - beta1) (g' - m) ;
 *   v = beta2 v + (1 - beta2) g' g' ;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * The table [host] lists the tensors that HAVE a gradient in this iteration; `step` is the count INCLUDING this step (>= 1).  A
 * tensor that is not listed is not touched.  n = 0 is allowed (nothing happens); pointers need 4-byte alignment only: a tensor
 * whose four arrays share one offset from the 16-byte grid gets 16-byte accesses on its aligned body, any other 4-byte ones.
 * The gradients are read twice and NOT modified (the clipped gradient exists in registers only).
 * No host synchronisation, no allocation on the device, no atomics; the table travels in kernel arguments, so the call is
 * capture-safe.  Bitwise reproducible: the same inputs give the same bits whatever the alignment of the arrays.
 *   partials [device, n_partials floats]  workspace, n_partials >= gom_clipped_adamw_partials(tensors, n_tensors);
 *   norm_out [device, 2 floats]           {total, coef} of this step, readable afterwards (logging).
 * gom_clipped_adamw_partials returns -1 for a table the step would reject.  Both check their arguments before any HIP call:
 * null table, n_tensors < 1, a negative size, a null or non-4-byte-aligned array of a non-empty tensor, step < 1 ->
 * GOM_ERR_INVALID_ARG. */
typedef struct gom_optim_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long n;
    long step;
    double lr;
    double weight_decay;
} gom_optim_tensor;
long gom_clipped_adamw_partials(const gom_optim_tensor* tensors, int n_tensors);
int gom_clipped_adamw_step(const gom_optim_tensor* tensors, int n_tensors, double beta1, double beta2, double eps,
                           double clip_value, float* partials, long n_partials, float* norm_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GOMATCHING_HIP_H_ */
