/* rangedet_hip.h -- C ABI of librangedet_hip.so: the MI355X (gfx950) RangeDet inference hot path.
 *
 * Every entry point replaces one piece of the reference's native/operator surface for this path
 * (citations relative to /root/reference; see INTEGRATION.md for the binding a maintainer would add):
 *
 *   rd_meta_kernel_fwd        MetaKernel.meta_baseline_bias + BN/ReLU/1x1/BN/ReLU
 *                             rangedet/symbol/backbone/meta_kernel.py:166-240, dla_backbone.py:92-97
 *   rd_conv2d_bn_act          mx.sym.Convolution + BatchNorm (+ReLU, +residual)   mxnext/simple.py:123-158,
 *                             mxnext/complicate.py:26-45, dla_backbone.py:18-56, head/builder.py:221-240
 *   rd_conv3x3_bn_act_ex      BasicBlock conv2 (+ stride (1,2), + projection shortcut)   dla_backbone.py:18-56,139-143
 *   rd_block64_bn_act         a whole 64-channel BasicBlock (conv1 + conv2 + shortcut) in one launch   dla_backbone.py:18-56
 *   rd_deconv2d_bn_act,       mx.sym.Deconvolution + BatchNorm + ReLU + add       mxnext/simple.py:545-580,
 *   rd_deconv2d_bn_act_all,   (one call per output phase / all phases in one launch / phase pairs as 128-channel
 *   rd_deconv2d_bn_act_pairs  problems)                                           dla_backbone.py:117-127
 *   rd_head_out               1x1 logit / delta convs + cast + per-class flatten  head/builder.py:242-261,99-154
 *   rd_sorted_foreground      Custom op 'get_sorted_foreground'                   operator_py/get_sorted_foreground.py:11-40
 *   rd_decode3d_bbox          _contrib_Decode3DBbox                               operator_cxx/contrib/decode_3d_bbox-inl.h:169-305
 *   rd_score_filter_dets      score filter + bbox3d_10dim_to_11dim                tools/test.py:56-81,200-209
 *   rd_wnms_4c                processing_cxx.wnms_4c                              operator_cxx/src_cxx/nms.h:452-577,781-794
 *   rd_single_overlap         OverlapChecker::single_overlap                      operator_cxx/src_cxx/nms.h:195-249
 *   rd_wnms_order_host        the std::sort ordering of point4_wnms_4c            operator_cxx/src_cxx/nms.h:786-792
 *   rd_dets12_to_8            bbox3d_12dim_to_8dim                                tools/test.py:43-53
 *   rd_rotated_iou_8pt        _contrib_RotatedIOU (8-point boxes)                 operator_cxx/contrib/rotated_iou-inl.h:509-547
 *   rd_batch_max_iou          Custom op 'batch_rotated_iou' ('bev')               operator_py/batch_rotated_iou.py:11-49
 *   rd_nms3d                  _contrib_NMS3D (the wnms=False branch)              operator_cxx/contrib/nms_3d.cu:380-534,
 *                             head/builder.py:530-534
 *   rd_assign3d_v2            processing_cxx.assign3D_v2                          operator_cxx/src_cxx/assigner.h:11-85
 *   rd_get_point_num          processing_cxx.get_point_num                        operator_cxx/src_cxx/assigner.h:87-109
 *   rd_input_transform        test-time input transform chain                     rangedet/core/input.py:14-42,89-229,522-624
 *   rd_train_transform        training-time input chain: the same plus Bbox3dAssigner, GenerateTarget and the training
 *                             FPN targets                                         rangedet/core/input.py:276-320,323-519,522-624,
 *                                                                                 operator_cxx/src_cxx/assigner.h:11-109
 *   rd_rpn_loss               get_iou_target + get_vfl_loss + get_normalize_reg_loss of one level, with the gradients MakeLoss sends
 *                             back                                                head/builder.py:156-196,268-422, head/loss.py:4-30
 *   rd_relu_affine_bwd,       the backward of a head tower (3x3 conv + norm + ReLU layers, 1x1 output conv with bias): ReLU / scale
 *   rd_conv3x3_bwd_weight,    backward, conv weight gradient in float32, output-conv backward
 *   rd_head_out_bwd                                                               head/builder.py:221-255, tools/train.py:358-360
 *   rd_bn_stats, rd_bn_fold,  training-mode BatchNorm + ReLU of a head-tower layer (normalizer_factory(type="localbn")), forward and
 *   rd_affine_relu,           backward                                            mxnext/complicate.py:26-45, mxnext/simple.py:502-508,
 *   rd_bn_relu_bwd                                                                head/builder.py:212-240
 *   rd_range_image_from_points  get_range_image + range_image_mask                datasets/create_range_image_in_kitti.py:107-137,178
 *
 * Conventions
 *   - every function returns an int status (RD_OK == 0, negative = error); nothing aborts or exits.
 *     rd_last_error_string() gives a thread-local message for the last failure.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller owns every buffer,
 *     including workspaces (size them with the *_workspace_bytes functions).  The library never allocates
 *     device memory and never keeps a pointer past the call.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are re-entrant.
 *   - activations inside the library are channels-last: [B][H][W][Cstride] with the used channels at
 *     [coff, coff+C); element type RD_F32 (float), RD_BF16 (raw uint16 bfloat16) or RD_F16 (raw uint16 IEEE half).
 *     rd_nchw_to_nhwc / rd_nhwc_to_nchw convert at the reference's NCHW float32 boundary.
 */
#ifndef RANGEDET_HIP_H_
#define RANGEDET_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RD_OK 0
#define RD_EINVAL (-1)     /* bad argument value                       */
#define RD_ESHAPE (-2)     /* shape the kernels do not support / mismatch (mirrors the reference's CHECKs) */
#define RD_EWORKSPACE (-3) /* workspace too small                      */
#define RD_EHIP (-4)       /* HIP runtime error                        */

#define RD_F32 0
#define RD_BF16 1
#define RD_F16 2  /* IEEE binary16: the reference's own mixed-precision type (config fp16 = True, dla_backbone.py:136-137 to_fp16,
                   * builder.py:257-261 to_fp32); every 16-bit layout is shared with RD_BF16 */

/* epilogue flags of the conv family */
#define RD_RELU_PRE 1  /* ReLU directly after the BN affine (before the residual add)        */
#define RD_ADD 2       /* add `residual`                                                     */
#define RD_RELU_POST 4 /* ReLU after the residual add                                        */
#define RD_SCALE_FOLDED 8 /* 16-bit 3x3 family only: the packer folded the BatchNorm scale into the weights (fold_scale argument of
                           * the packers); `scale` must be NULL.  The shift then enters the accumulators through one extra MFMA
                           * per accumulator and the epilogue has no multiply-add (what the production lowering uses) */
#define RD_MFMA16 16 /* rd_conv3x3_bn_act_ex (with RD_SCALE_FOLDED; stride 1, cout 128, cin a multiple of 32, no fused shortcut): w_packed is
                      * the image of rd_pack_conv3x3_m16_host and the launch issues v_mfma_f32_16x16x32 instead of 32x32x16 -- the same
                      * sums in the same per-channel order of the 32-channel chunks and taps; under the power cap of the part the
                      * matrix cores sustain more of them.  Like RD_SCALE_FOLDED a property of the packed image
                      * that the caller passes along: the library keeps no state per image */

int rd_version(void);
const char* rd_last_error_string(void);

/* ---- layout -------------------------------------------------------------------------------------- */
/* src NCHW float32 (B,C,H,W) -> dst channels-last [B][H][W][dst_cstride] at channel offset dst_coff.
 * Channels [C, C+zero_pad) are written as zeros (zero_pad may be 0). */
int rd_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int dst_cstride, int dst_coff,
                    int zero_pad, int dst_dtype, void* stream);
int rd_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int src_cstride, int src_coff,
                    int src_dtype, void* stream);

/* `rows` rows of `bytes` bytes: row r from src + r*src_row_bytes to dst + r*dst_row_bytes + dst_offset_bytes (device to
 * device, on `stream`).  The per-level point / mask variables are concatenated with it (builder.py:454-458: concat of
 * pc_vehicle_frame_s{1,2,4} / range_image_mask_s{1,2,4} along the point axis), one call per level for the whole batch. */
int rd_copy_rows(const void* src, long src_row_bytes, void* dst, long dst_row_bytes, long dst_offset_bytes, long bytes,
                 int rows, void* stream);

/* ---- weight packing (HOST, no GPU needed) ---------------------------------------------------------- */
/* Packed conv weights: [ntaps][nchunk][Cout][8 slots * (16/elem) channels], zero padded; one k-chunk =
 * 8 slots of 16 bytes.  rd_conv_packed_bytes gives the size.  w_oihw_host is (Cout,Cin,KH,KW) float32
 * (mx Convolution layout); deconv weight is (Cin,Cout,KH,KW) (mx Deconvolution layout) and is packed per
 * output phase (phase = ow % stride_w) -- rd_deconv_phase_taps tells how many taps a phase's PACKED image has: the
 * phase's own tap count (<= 9, in ascending (dh, dw) order; more is RD_ESHAPE), except that a phase whose taps lie
 * inside the 3x3 window without being three rows x two adjacent columns is packed as all 9 window taps (zeros for the
 * absent ones). */
/* (every packed image ends in 256 zero bytes, included in the size: the persistent 3x3 kernel reads its padding pixels from
 * them, so the library holds no device memory of its own; upload the image whole) */
size_t rd_conv_packed_bytes(int ntaps, int cin, int cout, int dtype);
int rd_pack_conv_weight_host(const float* w_oihw_host, int cout, int cin, int kh, int kw, int dtype,
                             void* packed_host);
int rd_deconv_phase_taps(int kh, int kw, int stride_w, int pad_w, int phase);
int rd_pack_deconv_weight_host(const float* w_iohw_host, int cin, int cout, int kh, int kw, int stride_w,
                               int pad_w, int phase, int dtype, void* packed_host);
/* the same with fold_scale_host (cout) multiplied into the weights before rounding (for RD_SCALE_FOLDED launches; NULL = none) */
int rd_pack_deconv_weight_folded_host(const float* w_iohw_host, const float* fold_scale_host, int cin, int cout, int kh, int kw,
                                      int stride_w, int pad_w, int phase, int dtype, void* packed_host);

/* ---- conv family ------------------------------------------------------------------------------------ */
/* y = act( scale[c]*conv(x, w) + shift[c] (+ residual) ).  stride_h == 1 always (the backbone strides W
 * only, dla_backbone.py:139-143); kernel (kh,kw) in {(1,1),(3,3)}; pad = (k-1)/2 as mxnext/simple.py:131-135.
 * cout in {64,128}.  x: [B][H][Win][x_cstride] channels [x_coff, x_coff+cin); cin is rounded up internally to
 * the packing granule and the buffer must hold zeros there. */
int rd_conv2d_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale,
                     const float* shift, const void* residual, int r_cstride, int r_coff, void* y,
                     int y_cstride, int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw,
                     int stride_w, int flags, int dtype, void* stream);
/* Second conv of a BasicBlock in its extended forms (dla_backbone.py:18-56; dtype RD_BF16 or RD_F16, persistent kernel):
 *   stride_w 2  (`conv2` of the first unit of a down-sampling stage, dla_backbone.py:139-143): computed on the pixel-pair view
 *               of x -- [H][Win][cs] with Win even read as [H][Win/2][2*cs] -- as a stride-1 conv with six taps, so only the
 *               stored pixels are computed; weights packed by rd_pack_conv3x3_ex_host(stride_w = 2, x_cstride);
 *   sc_x != NULL  the block's projection shortcut  BN(Convolution 1x1 (stride_w) of the block input)  (dla_backbone.py:44-51)
 *               is accumulated onto the conv's accumulators in the epilogue (no shortcut tensor, no second launch).  The two
 *               BatchNorm scales must be FOLDED into the two weight sets (fold_scale of the packers), `scale` = NULL and
 *               `shift` = shift_conv + shift_shortcut; RD_ADD is implied, `residual` must be NULL.
 * Otherwise the contract of rd_conv2d_bn_act (3x3, pad 1).  sc_x: [B][H][Win][sc_cstride], channels [sc_coff, sc_coff+sc_cin). */
size_t rd_conv3x3_ex_packed_bytes(int cin, int cout, int stride_w, int x_cstride);
int rd_pack_conv3x3_ex_host(const float* w_oihw_host, const float* fold_scale_host, int cout, int cin, int stride_w,
                            int x_cstride, int dtype, void* packed_host);
/* weights of an RD_MFMA16 launch (same size as rd_conv3x3_ex_packed_bytes(cin, 128, 1, cin)); rd_conv3x3_mfma16_ok: 1 if the library has that
 * launch form for a stride_w conv cin -> cout at width W (fused_output_conv: through rd_conv2d_bn_act_head_out) -- the caller asks before
 * it packs; a launch with RD_MFMA16 where the answer is 0 fails with RD_ESHAPE */
int rd_pack_conv3x3_m16_host(const float* w_oihw_host, const float* fold_scale_host, int cout, int cin, int dtype, void* packed_host);
int rd_conv3x3_mfma16_ok(int cin, int cout, int stride_w, int W, int fused_output_conv);
size_t rd_conv1x1_sc_packed_bytes(int cin, int cout);
int rd_pack_conv1x1_sc_host(const float* w_oi_host, const float* fold_scale_host, int cout, int cin, int dtype,
                            void* packed_host);
int rd_conv3x3_bn_act_ex(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale, const float* shift,
                         const void* residual, int r_cstride, int r_coff, const void* sc_x, int sc_cstride, int sc_coff,
                         int sc_cin, const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int Win, int cin,
                         int cout, int stride_w, int flags, int dtype, void* stream);
/* A whole 64-channel BasicBlock (rangedet/symbol/backbone/dla_backbone.py:18-56: conv1 3x3 + BN + ReLU, conv2 3x3 + BN, + shortcut, ReLU;
 * stride 1, cin -> 64 -> 64) as ONE launch -- replaces the two rd_conv3x3_bn_act_ex calls of the block; the intermediate tensor is never
 * written to HBM (it lives in LDS as conv2's halo image) and the results are BIT-IDENTICAL to the two calls.
 *   cin == 64, sc_w_packed == NULL  identity shortcut (units 2.. of a stage):  y = relu(BN2(conv2(relu(BN1(conv1(x))))) + x)
 *   cin == 64, sc_w_packed != NULL  projection shortcut (unit 1, dla_backbone.py:44-51): + BNs(conv1x1(x)) instead of + x; sc_w_packed =
 *                        rd_pack_conv1x1_sc_host(cin -> 64, fold_scale = the shortcut BatchNorm's scale), shift2 = conv2's + the shortcut's.
 *   cin <= 16            the network's first block (res1_unit1: the 8-channel range image, or 5 channels for KITTI): conv1 runs as five
 *                        two-tap steps on one 16-channel k-slot; the projection shortcut is required.
 * w_packed = rd_pack_block64_host (HOST): the 3x3 weights (64, cin, 3, 3) and (64, 64, 3, 3) with their BatchNorm scales folded in;
 * shift1 / shift2 (64) floats on the device.  x: [B][H][W][x_cstride] channels [x_coff, x_coff + cin) -- the channels up to the next
 * multiple of 16 must exist in the buffer and be zero --, y: channels [y_coff, y_coff + 64); 16-bit types only. */
size_t rd_block64_packed_bytes(int cin);
int rd_pack_block64_host(const float* w1_oihw_host, const float* fold_scale1_host, const float* w2_oihw_host,
                         const float* fold_scale2_host, int cin, int dtype, void* packed_host);
int rd_block64_bn_act(const void* x, int x_cstride, int x_coff, int cin, const void* w_packed, const float* shift1, const float* shift2,
                      const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype, void* stream);
/* The same block (64 input channels) issuing v_mfma_f32_16x16x32 instead of 32x32x16 (round 6; see RD_MFMA16): w_packed from
 * rd_pack_block64_m16_host (rd_block64_packed_bytes(64) bytes), sc_w_packed (projection shortcut 64 -> 64, or NULL) from
 * rd_pack_conv1x1_sc_m16_host (rd_conv1x1_sc_packed_bytes(64, 64) bytes); results identical to rd_block64_bn_act */
int rd_pack_block64_m16_host(const float* w1_oihw_host, const float* fold_scale1_host, const float* w2_oihw_host,
                             const float* fold_scale2_host, int dtype, void* packed_host);
int rd_pack_conv1x1_sc_m16_host(const float* w_oi_host, const float* fold_scale_host, int dtype, void* packed_host);
int rd_block64_m16_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* shift1, const float* shift2,
                          const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype, void* stream);

/* Last conv of a head tower (3x3, cout 128, BN + ReLU, RD_BF16 or RD_F16) FUSED with the tower's 1x1 output conv (head/builder.py:221-261:
 * rpn_{cls,reg}_conv_3 + BN + ReLU, then rpn_cls_logit / rpn_reg_delta with bias): the 128-channel result is consumed in
 * the epilogue and never written.  out[b*out_batch_stride + (n_off + h*W + w)*nout + o], float32, like rd_head_out; nout <= 8.
 * head_w_packed: rd_pack_head_weight_host(w (nout, 128) row-major float32) -> rd_head_packed_bytes() bytes (bf16 hi + lo
 * pairs, so the fp32 weights keep their precision).  Same numbers as rd_conv2d_bn_act followed by rd_head_out up to fp32
 * summation order. */
size_t rd_head_packed_bytes(void);
int rd_pack_head_weight_host(const float* w, int nout, int cin, int dtype, void* out_host);
/* ... of an RD_MFMA16 launch of rd_conv2d_bn_act_head_out (flags carry RD_MFMA16, w_packed from rd_pack_conv3x3_m16_host): head_w_packed must be
 * THIS image (rd_head_m16_packed_bytes() = 8 KB: 16-row fragments in the order the conv's epilogue holds the channels) -- the output conv
 * then reads the rounded tower activations straight from the registers */
size_t rd_head_m16_packed_bytes(void);
int rd_pack_head_weight_m16_host(const float* w, int nout, int cin, int dtype, void* out_host);
int rd_conv2d_bn_act_head_out(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale,
                              const float* shift, int B, int H, int W, int cin, int flags, const void* head_w_packed,
                              const float* head_bias, float* out, long out_batch_stride, long n_off, int nout, int dtype,
                              void* stream);

/* 3x3 stride-1 conv + BatchNorm (+ReLU) over the channel concatenation [x1 (cin1, a multiple of 32) | x2 (cin2, a multiple of 8)]
 * of two tensors of the same B x H x W -- the concat itself (mx.sym.concat of the range image with the agg3 feature map,
 * dla_backbone.py:153-154, consumed by the level-0 tower convs head/builder.py:221-240) is never written: each tensor keeps its own
 * channel stride.  16-bit types, RD_SCALE_FOLDED weights: w_packed = rd_pack_conv3x3_cat_host (HOST) of the (cout, cin1 + cin2, 3, 3)
 * weight in that channel order, rd_conv3x3_cat_packed_bytes long (with cin1 = 64, cin2 <= 16 the x2 chunk runs as five two-tap
 * steps on its one 16-channel slot instead of nine steps of two slots).  No residual. */
size_t rd_conv3x3_cat_packed_bytes(int cin1, int cin2, int cout);
int rd_pack_conv3x3_cat_host(const float* w, const float* fold_scale, int cout, int cin1, int cin2, int dtype, void* out_host);
int rd_conv3x3_bn_act_cat(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                          const void* w_packed, const float* shift, void* y, int y_cstride, int y_coff, int B, int H, int W, int cout,
                          int flags, int dtype, void* stream);

/* Transposed conv, kernel (3,kw), stride (1,stride_w), pad (1,pad_w); one call per output phase. */
int rd_deconv2d_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed_phase,
                       const float* scale, const float* shift, const void* residual, int r_cstride,
                       int r_coff, void* y, int y_cstride, int y_coff, int B, int H, int Win, int cin,
                       int cout, int kh, int kw, int stride_w, int pad_w, int phase, int flags, int dtype,
                       void* stream);

/* The same transposed conv, ALL stride_w output phases in ONE launch (16-bit types, RD_SCALE_FOLDED weights): the tile list is
 * (tile, phase) with a tile's phases computed back to back by one workgroup, so the input is read from HBM once instead of once
 * per phase launch (mx.sym.Deconvolution + BatchNorm + ReLU + add, mxnext/simple.py:545-580, dla_backbone.py:117-127).
 * w_packed_all: the stride_w images of rd_pack_deconv_weight_folded_host, phase p at byte offset p * w_phase_bytes.
 * rd_deconv2d_all_phases_ok: 1 if this (kernel, stride, pad, cout, dtype) can run in that form -- every phase a 3 x 2 tap set
 * inside the 3 x 3 window and Wout == stride_w * Win, which k(3,8) s4 p2 and k(3,4) s2 p1 are -- else 0 (call per phase). */
int rd_deconv2d_all_phases_ok(int kh, int kw, int stride_w, int pad_w, int cout, int dtype);
int rd_deconv2d_bn_act_all(const void* x, int x_cstride, int x_coff, const void* w_packed_all, long w_phase_bytes,
                           const float* shift, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                           int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                           int flags, int dtype, void* stream);

/* The same launch with output phases 2p and 2p+1 computed as ONE 128-channel problem (cout 64, even stride, both phases of a pair
 * on the same two input columns -- k(3,8) s4 p2: dla_backbone.py:117-127 'agg1'): in the output seen as [H][Win][stride_w * cout] a
 * pair's channels are neighbours, so it is a 3 x 2-tap conv with 128 outputs and runs the cout-128 form of the kernel (bit-identical
 * to rd_deconv2d_bn_act_all).  y / residual: dense cout-channel tensors (cstride == cout, coff 0).
 * w_packed_pairs: stride_w / 2 images of rd_pack_deconv_phase_pair_host (phase images 2p, 2p+1 of rd_pack_deconv_weight_folded_host
 * interleaved; 2 x the bytes of one phase image each), pair p at byte offset p * w_pair_bytes.  shift2: the layer's shift twice
 * (2 * cout values).  rd_deconv2d_phase_pairs_ok: 1 if (kernel, stride, pad, cout, dtype) has this form, else 0. */
int rd_deconv2d_phase_pairs_ok(int kh, int kw, int stride_w, int pad_w, int cout, int dtype);
int rd_pack_deconv_phase_pair_host(const void* phase_a, const void* phase_b, int cin, int dtype, void* out);
int rd_deconv2d_bn_act_pairs(const void* x, int x_cstride, int x_coff, const void* w_packed_pairs, long w_pair_bytes,
                             const float* shift2, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                             int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                             int flags, int dtype, void* stream);

/* 1x1 conv with bias to nout <= 8 float32 outputs per pixel, written flattened: out[(n_off + h*W + w)*nout + o]
 * (== the (B, N, nout) tensor after sep_level_type's reshape/transpose/concat; nout == 1 gives (B, N)).
 * w: (nout, cin) float32 device, bias: (nout).  out_batch_stride in elements. */
int rd_head_out(const void* x, int x_cstride, int x_coff, const float* w, const float* bias, float* out,
                long out_batch_stride, long n_off, int B, int H, int W, int cin, int nout, int dtype,
                void* stream);

/* ---- Meta-Kernel unit ------------------------------------------------------------------------------- */
/* Packed parameter block for rd_meta_kernel_fwd (HOST).  Inputs in the reference's layouts:
 * w0 (32,3) b0 (32) w1 (64,32) b1 (64) [mlp0/mlp1 1x1 convs], s1,t1 (576) [BN folded, index c*9+k],
 * agg (64,576) [aggregation_conv1], s2,t2 (64).  */
size_t rd_meta_packed_bytes(int dtype);
int rd_pack_meta_host(const float* w0, const float* b0, const float* w1, const float* b1, const float* s1,
                      const float* t1, const float* agg, const float* s2, const float* t2, int dtype,
                      void* packed_host);
/* data: [B][H][W][d_cstride] (64 channels at d_coff), coord: NCHW float32 (B,3,H,W) as the reference's
 * coord_s1 variable, y: [B][H][W][y_cstride] 64 channels at y_coff. */
int rd_meta_kernel_fwd(const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                       const void* packed, void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype,
                       void* stream);

/* ---- post-processing -------------------------------------------------------------------------------- */
/* bytes for ONE batch element; pass B times that to let the B independent sorts run side by side */
size_t rd_sorted_foreground_workspace_bytes(long N, long k);
/* cls_score (B,N) [logits when apply_sigmoid != 0], bbox_delta (B,N,D), pc (B,N,3), mask (B,N) ->
 * sorted_fg_score (B,k), sorted_fg_bbox_delta (B,k,D), sorted_fg_pc (B,k,3); optional sorted_idx (B,k) int32.
 * Order: score*mask descending, ties by flat index ascending.  Requires N >= k (get_sorted_foreground.py:65).
 * (2k <= N: only the keys up to the k-th one's 12-bit bin are sorted -- same result, see k_sort.h.) */
int rd_sorted_foreground(const float* cls_score, const float* bbox_delta, const float* pc, const float* mask,
                         int B, long N, long k, int D, int apply_sigmoid, float* out_score, float* out_delta,
                         float* out_pc, int* out_idx, void* ws, size_t ws_bytes, void* stream);

/* bbox_delta (B,N,box_type) + pc (B,N,3) -> (B,N,10); box_type 8 (is_bin=0) or 7 (is_bin=1)
 * (shape checks of decode_3d_bbox.cc:30-49). */
int rd_decode3d_bbox(const float* bbox_delta, const float* pc, float* out, int B, long N, int box_type,
                     int is_bin, void* stream);

/* scores (n), boxes10 (n,10) -> dets (K,12) rows [8 corners, yaw, bottom, height, score] for score > min_score,
 * input order preserved; *d_count (device int) = K.  dets must hold n rows. */
size_t rd_score_filter_workspace_bytes(long n);
int rd_score_filter_dets(const float* scores, const float* boxes10, long n, float min_score, float* dets,
                         int* d_count, void* ws, size_t ws_bytes, void* stream);
/* B frames in one set of launches: frame b reads scores + b*scores_bstride, boxes10 + b*boxes_bstride, writes
 * dets + b*dets_bstride (strides in floats) and d_count[b]; ws_bytes >= B * rd_score_filter_workspace_bytes(n). */
int rd_score_filter_dets_batched(const float* scores, long scores_bstride, const float* boxes10, long boxes_bstride,
                                 long n, float min_score, float* dets, long dets_bstride, int* d_count, void* ws,
                                 size_t ws_bytes, int B, void* stream);

/* Weighted NMS.  dets (Kcap,12) device; the number of valid rows is *d_count when d_count != NULL, else Kcap (rows past
 * the count are ignored; a count above Kcap is clamped -- callers size Kcap from the data, up to RD_WNMS_MAX_K = more than
 * the reference's pre_nms_top_n of 50000 rows).
 * order: device int32 (Kcap) processing order (sorted positions -> row index).  NULL = the library orders on the device:
 *   tie_order RD_TIE_REFERENCE  the order std::sort gives point4_wnms_4c (nms.h:786-792; unstable: tied scores come out in
 *                               libstdc++ introsort order, replayed on the device; rows that arrive strictly sorted -- the
 *                               pipeline's case without ties -- cost one pass);
 *   tie_order RD_TIE_STABLE     score descending, ties by row index ascending (single frame only).
 * hash_scale: cell size of the reference's BBoxHash prefilter (nms.h:252-307, 459, 470, 501-507; tools/test.py:216 passes
 * 100): a pair of boxes is compared only when their cell ranges share a key, exactly like the reference.  <= 0: no
 * prefilter.  Outputs: out_dets (Kcap,12), keep (Kcap) row indices into dets in processing order, *d_nkeep = M. */
#define RD_WNMS_MAX_K 65536
#define RD_TIE_STABLE 0
#define RD_TIE_REFERENCE 1
/* Diagnostic bits that may be OR-ed into tie_order (per call; the RESULT never depends on them -- they select code paths so that tests
 * can compare them bit for bit; until round 5 these were environment variables of the library):
 *   RD_WNMS_DIAG_NO_SKIP        clip every pair the reference clips (no rejection test, see rd_wnms_pair_skippable)
 *   RD_WNMS_DIAG_TILE_W(n)      scan column chunks of n 64-row words (1..255): the column-chunked scan of K > 16 384 at any K
 *   RD_WNMS_DIAG_MERGE_LDS(n)   merge neighbourhood list of n entries in LDS (4..127): the global-scratch merge path at small K */
#define RD_WNMS_DIAG_NO_SKIP 0x100
#define RD_WNMS_DIAG_TILE_W(n) (((n) & 0xff) << 16)
#define RD_WNMS_DIAG_MERGE_LDS(n) (((n) & 0x7f) << 24)
size_t rd_wnms_workspace_bytes(int Kcap);
int rd_wnms_4c(const float* dets, int Kcap, const int* d_count, const int* order, int tie_order, float thresh,
               float thresh_vote, int is3d, int hash_scale, float* out_dets, int* keep, int* d_nkeep, void* ws,
               size_t ws_bytes, void* stream);
/* B independent frames in one set of launches (the per-frame greedy scan is one latency-bound wavefront: B of them
 * run side by side instead of back to back).  Frame b uses dets + b*dets_bstride, order + b*order_bstride (stride 0 =
 * one order shared by all frames; with order == NULL and B > 1 tie_order must be RD_TIE_REFERENCE), d_count[b],
 * out_dets + b*out_bstride, keep + b*keep_bstride, d_nkeep[b]; ws_bytes >= B * rd_wnms_workspace_bytes(Kcap).
 * Strides in elements. */
int rd_wnms_4c_batched(const float* dets, long dets_bstride, int Kcap, const int* d_count, const int* order,
                       long order_bstride, int tie_order, float thresh, float thresh_vote, int is3d, int hash_scale,
                       float* out_dets, long out_bstride, int* keep, long keep_bstride, int* d_nkeep, void* ws,
                       size_t ws_bytes, int B, void* stream);
/* OverlapChecker::single_overlap (nms.h:195-249) of n row pairs: out[i] = overlap(dets_a[i], dets_b[i]) -- BEV IoU of the two
 * 4-corner boxes, or volume IoU with is3d (rows are (n,12) dets rows).  The measure the weighted NMS thresholds. */
int rd_single_overlap(const float* dets_a, const float* dets_b, long n, int is3d, float* out, void* stream);
/* The pair kernel's rejection test on n independent row pairs (dets rows as in rd_wnms_4c): out[i] = 1 if rd_wnms_4c would NOT run
 * the polygon clip on (dets_a[i], dets_b[i]) because the reference's value cannot reach a threshold >= 1e-3 -- both boxes rectangles
 * with 0.2 .. 25 m edges and |coordinates| <= 200 m, bounding rectangles > 0.01 m apart, edge directions >= 0.01 rad apart mod 90
 * degrees (characterised on the compiled reference: oracle/ref_overlap_study.cpp; nms.h:96-149,195-249 has no empty-intersection
 * test).  Test / characterisation aid: results of rd_wnms_4c do not depend on it. */
int rd_wnms_pair_skippable(const float* dets_a, const float* dets_b, long n, unsigned char* out, void* stream);

/* out[i] = atan2f(y[i], x[i]) as the weighted NMS computes its edge angles (nms.h:71) and the score filter its yaw column: the C
 * library's float routine -- glibc's fdlibm algorithm restated operation by operation on the device (not the device math library's
 * atan2f, which differs from it in the last bit).  Test / characterisation aid: bit-equal to the host's atan2f (tests/test_kernels.py). */
int rd_edge_atan2f(const float* y, const float* x, long n, float* out, void* stream);

/* HOST: the reference's own ordering (std::sort, score descending, unstable) for dets_host (K,12). */
int rd_wnms_order_host(const float* dets_host, int K, int* order_host);

/* dets12 (M,12) -> (M,8) [cx,cy,cz,l,w,h,heading,score]; count from *d_count when not NULL. */
int rd_dets12_to_8(const float* dets12, int Mcap, const int* d_count, float* out8, void* stream);
int rd_dets12_to_8_batched(const float* dets12, long dets12_bstride, int Mcap, const int* d_count, float* out8,
                           long out8_bstride, int B, void* stream);

/* 8-point rotated IoU: boxes1 (n1,8) x boxes2 (n2,8) -> ious (n1,n2). */
int rd_rotated_iou_8pt(const float* boxes1, const float* boxes2, float* ious, long n1, long n2, void* stream);
/* Custom op 'batch_rotated_iou', iou_type 'bev' (operator_py/batch_rotated_iou.py:11-49, shapes :69-91): proposal
 * (B, N, p_stride >= 8: the 8 BEV corner coordinates lead each row; the op's rows are 10 wide), gt_bbox (B, n_gt <= 256, 8)
 * -> iou_map (B, N) = max over the frame's GT boxes of the 8-point rotated IoU after NaN / Inf / > 1 / < 0 -> 0.
 * argmax (B, N) int32, optional (NULL): index of the first GT box reaching that maximum (0 when every IoU is 0). */
int rd_batch_rotated_iou(const float* proposal, int p_stride, const float* gt_bbox, float* iou_map, int* argmax, int B, long N,
                         int n_gt, void* stream);
/* The same op with iou_type '3d' (operator_py/batch_rotated_iou.py:17-18,36-39,51-68; _contrib_RotatedIOU on 7-dim boxes,
 * operator_cxx/contrib/rotated_iou-inl.h:495-522): proposal (B, N, p_stride >= 10: 8 BEV corners + z0, z1) is converted to
 * [cx, cy, cz, length, width, height, yaw] (to_box_type_7), the yaw of proposals AND of gt_bbox7 (B, n_gt <= 256, 7) is negated, and
 * iou_map (B, N) = max over the frame's GT boxes of the VOLUME IoU after the same cleaning.  argmax as above.
 * rd_rotated_iou_7: the 7-dim IoU matrix itself, boxes [x, y, z, w, l, h, angle] as the reference op takes them. */
int rd_batch_rotated_iou_3d(const float* proposal, int p_stride, const float* gt_bbox7, float* iou_map, int* argmax, int B, long N,
                            int n_gt, void* stream);
int rd_rotated_iou_7(const float* boxes1, const float* boxes2, float* ious, long n1, long n2, void* stream);
/* one frame of the above without argmax.  proposals (n, p_stride>=8) */
int rd_batch_max_iou(const float* proposals, int p_stride, const float* gt8, float* out, long n, int n_gt,
                     void* stream);

/* ---- greedy 3-D NMS: _contrib_NMS3D(boxes, iou_thres, max_keep, normal_iou=False) ----
 * operator_cxx/contrib/nms_3d.cc:22-68 (shapes), nms_3d.cu:342-378 (overlap measures), :380-464 (mask + keep loop),
 * :466-534 (forward).  boxes (B,N,10) float32 = 4 BEV corners (x,y) + z_low, z_high, ALREADY sorted by score descending
 * (head/builder.py:519-534 feeds the decoded boxes of get_sorted_foreground).  Box i is kept when no kept box before it
 * has overlap(kept, i) > iou_thres; overlap = intersection volume / union volume (polygon clip in BEV x height overlap),
 * or the axis-aligned 2-D IoU of (x1,y1,x2,y2) = boxes[..., 0:4] when normal_iou != 0.  Stops after max_keep rows.
 * keep_idx (B,max_keep) int32 padded with -1; bbox_after_nms (B,max_keep,10) padded with 0.
 * Unlike the reference (N x N/64 words per frame) the mask is held for 1024 rows at a time. */
size_t rd_nms3d_workspace_bytes(long N, int B);
/* tools/test.py:193-196 (the `not pTest.nms.wnms` branch): out (B,max_keep) = score[b][keep_idx[b][i]], -inf where
 * keep_idx is -1, so that rd_score_filter_dets_batched on (out, bbox_after_nms) yields the reference's final rows. */
int rd_gather_keep_scores(const float* score, long score_bstride, int k, const int* keep_idx, int max_keep, float* out, int B,
                          void* stream);
int rd_nms3d(const float* boxes, int B, long N, float iou_thres, int max_keep, int normal_iou, int* keep_idx,
             float* bbox_after_nms, void* ws, size_t ws_bytes, void* stream);

/* ---- training-target assignment: processing_cxx.assign3D_v2 / get_point_num (pybinding.cpp:9-10) ----
 * assigner.h:11-85.  For every point (pc (N,3), row-major) the index of the FIRST ground-truth box that contains it, or -1.
 * bbox (M,24) = 8 corners x (x,y,z): A B C D bottom face, E.. top face; bbox_center (M,3); bbox_radius (M) is compared with
 * the SQUARED centre distance, and so is max_dist (the reference does both, :47-51); mask (N) < 0.5 or is_in_nlz (N) > 0
 * skips the point; the six limits are the caller's axis-aligned bounds of all boxes (input.py:303-308).  out (N) int32.
 * M <= 1024 (boxes are held in LDS). */
int rd_assign3d_v2(const float* pc, const float* bbox, const float* bbox_center, const float* bbox_radius, const float* mask,
                   const float* is_in_nlz, long N, int M, float max_x, float min_x, float max_y, float min_y, float max_z,
                   float min_z, float max_dist, int* out, void* stream);
/* assigner.h:87-109.  bbox_inds (N) float32 box index per point (negative = none); out (N) float32 = number of points that
 * share the point's box, -1 for points without a box.  Indices >= 500 (MAX_BOX_NUM, :92) are outside the reference's
 * contract (it writes out of bounds); here such points get -1. */
size_t rd_get_point_num_workspace_bytes(void);
int rd_get_point_num(const float* bbox_inds, long N, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- test-time input transform chain on the device (the step before the path) ----
 * rangedet/core/input.py:14-42,89-229,522-624 (LoadRecord, ProcessMissValue, SepAndClipData, GetUnnormalizedRange,
 * NormData, GetCoordinates, CombineData, PadData, TransposeData, GenerateFPNTarget, TransAndReshape) fused into one
 * kernel: raw record arrays in, the graph's named float32 tensors out.
 * Channel order of clip/mean/sd: range, intensity, elongation, x, y, z, inclination, azimuth (config:269-282; azimuth is
 * not clipped).  sd = sqrt(var) as float.  Level l uses stride 2^l and keeps range in [interval_lo[l], interval_hi[l]). */
typedef struct {
  float clip_lo[7], clip_hi[7];
  float mean[8], sd[8];
  float interval_lo[3], interval_hi[3];
} rd_input_norm_t;
/* range_image (B,H,W,4), pc_vehicle_frame (B,H,W,3), inclination (B,H)  ->  input_data (B,8,Hp,Wp), coord_s1 (B,3,Hp,Wp),
 * pc_vehicle_frame_s{1,2,4} (B,Hp*Wp/s,3), range_image_mask_s{1,2,4} (B,Hp*Wp/s); Hp >= H, Wp >= W, Wp % 4 == 0.
 * norm_host is read on the host at call time. */
int rd_input_transform(const float* range_image, const float* pc_vehicle_frame, const float* inclination,
                       const rd_input_norm_t* norm_host, int B, int H, int W, int Hp, int Wp, float* input_data,
                       float* coord_s1, float* pc_s1, float* pc_s2, float* pc_s4, float* mask_s1, float* mask_s2,
                       float* mask_s4, void* stream);

/* ---- training-time input chain on the device: rd_input_transform + Bbox3dAssigner + GenerateTarget + the training FPN targets ----
 * rangedet/core/input.py:276-320,323-519,522-624 and operator_cxx/src_cxx/assigner.h:11-109 with the training name lists of
 * config/rangedet/rangedet_veh_wo_aug_4_18e.py:72-81,295-305,316-326,336 (one class), for a whole batch in two launches: (1) the box
 * index of every unpadded pixel's post-ProcessMissValue point (the comparisons of rd_assign3d_v2) and the points per box, (2) all
 * named tensors.  Every pointer of rd_train_outputs_t is a device pointer; the struct itself is read on the host at call time.
 * Level l has stride s = 2^l and samples columns s/2, s/2 + s, ...:
 *   input_data (B,8,Hp,Wp), coord_s1 (B,3,Hp,Wp), pc[l] (B,Hp*Wp/s,3): what rd_input_transform writes
 *   mask[l] (B,1,Hp,Wp/s): the fill-propagated validity mask, NOT multiplied by the range interval (config:78-81)
 *   reg_target[l], reg_weight[l], reg_normalize_weight[l] (B,8,Hp,Wp/s) and cls_target[l] (B,1,Hp,Wp/s): each multiplied by the level's
 *     interval mask on the clipped unnormalised range (input.py:582-597).  reg_target of a pixel in a box with (x,y,z,l,w,h,yaw), point p,
 *     az = atan2f(p.y, p.x), r = Rz(-az) (xyz - p): (sign(r.x) sqrt|r.x|, sign(r.y) sqrt|r.y|, log w, log l, cos(yaw - az),
 *     sin(yaw - az), z - h/2, log h) in float32 (input.py:469-503); reg_weight = reg_weight_host there; reg_normalize_weight =
 *     1 / (points in the pixel's box) on all 8 channels (IEEE divide); cls_target = 1.  Zero for pixels without a box and in the padding.
 *   bbox3d_ind (B,H,W) int32: index of the first containing box, -1 for none (Bbox3dAssigner's bbox3d_ind_of_each_pt)
 * Inputs: range_image (B,H,W,4), pc_vehicle_frame (B,H,W,3), inclination (B,H), norm_host as for rd_input_transform;
 * gt_bbox_imu (B,Mmax,24), gt_bbox_center (B,Mmax,3), gt_limits (B,6) = max_x min_x max_y min_y max_z min_z of the frame's boxes,
 * gt_bbox_csa (B,Mmax,7); frame b uses its first num_gt_host[b] boxes (read at call time).  radius and max_dist are compared with SQUARED
 * centre distances like in rd_assign3d_v2 (the reference passes 100 and 20, input.py:299,309).  reg_weight_host: 8 floats.
 * RD_ESHAPE: Wp % 4 != 0, Hp < H, Wp < W, H or W < 3, Mmax < 1, a num_gt outside 1..min(Mmax, 500) (MAX_BOX_NUM, assigner.h:92).
 * RD_EWORKSPACE: ws_bytes < rd_train_transform_workspace_bytes(B) (the workspace is zeroed on the stream). */
typedef struct {
  float *input_data, *coord_s1;
  float *pc[3], *mask[3];
  float *reg_target[3], *reg_weight[3], *reg_normalize_weight[3], *cls_target[3];
  int* bbox3d_ind;
} rd_train_outputs_t;
size_t rd_train_transform_workspace_bytes(int B);
int rd_train_transform(const float* range_image, const float* pc_vehicle_frame, const float* inclination,
                       const rd_input_norm_t* norm_host, const float* gt_bbox_imu, const float* gt_bbox_center,
                       const float* gt_limits, const float* gt_bbox_csa, const int* num_gt_host, int Mmax, float radius,
                       float max_dist, const float* reg_weight_host, int B, int H, int W, int Hp, int Wp,
                       const rd_train_outputs_t* out_host, void* ws, size_t ws_bytes, void* stream);

/* ---- range image from a raw spinning-LiDAR point cloud (the step before rd_input_transform for data that ships no range image) ----
 * datasets/create_range_image_in_kitti.py:107-137 (get_range_image) and :178 (range_image_mask), for B scans of different lengths in one
 * call.  points (sum N_b, 4) float32 x, y, z, intensity, scan b = rows [offsets_host[b], offsets_host[b+1]); incl_host / height_host: H
 * doubles each, the beams' inclinations and sensor heights (read on the host at call time, like offsets_host).  Per point, in the
 * reference's arithmetic:
 *   row    = first arg-min over beams i of |incl[i] - atan2(height[i] - z, xy_norm)| in double, xy_norm = sqrtf(x*x + y*y) (float)
 *   column = float throughout: round-half-even((W - 0.5) - (atan2f(y, x) + pi) / (2 pi) * W), then == W -> W - 1, < 0 -> 0 (the reference
 *            hard-codes W = 2048); atan2f is the C library's (glibc / fdlibm) bit for bit
 *   range  = sqrtf((x*x + y*y) + z*z)
 * The nearest point of a cell wins (the reference writes in order of decreasing range).  TIE RULE: of two points of one cell with the
 * same range the one with the HIGHER index wins -- what a stable argsort gives; the reference's argsort is not stable, so it leaves this
 * open.  A point with a non-finite x, y or z (outside the reference's contract) is skipped; nothing is ever written out of bounds.
 * Outputs: range_image (B,H,W,5) float32 = [range, x, y, z, intensity] of the winning point, five -1 in an empty cell; mask (B,H,W)
 * bytes 0/1 = range_image[..., 0] > -1; point_index (B,H,W) int32 = the winner's index within its scan, -1 = empty (may be NULL).
 * ws: B*H*W*8 bytes of keys, set on the stream in every call (its contents on entry do not matter).  points and range_image must be
 * 16-byte aligned, ws 8-byte aligned.  The result does not depend on the order in which the GPU processes the points.
 * RD_ESHAPE: B < 1, H outside 1..128, W outside 1..2^22, offsets_host not non-decreasing from 0, a scan of 2^31 points or more.
 * RD_EWORKSPACE: ws_bytes < rd_range_image_workspace_bytes(B, H, W).  RD_EINVAL: a null required pointer (points may be NULL only when
 * there is no point at all), a misaligned buffer.  A scan without points is valid: all -1. */
size_t rd_range_image_workspace_bytes(int B, int H, int W);
int rd_range_image_from_points(const float* points, const long long* offsets_host, int B, const double* incl_host,
                               const double* height_host, int H, int W, float* range_image, unsigned char* mask, int* point_index,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- RPN loss head of one pyramid level: IoU target, varifocal loss, normalised smooth-L1 loss and their head gradients ----------
 * RangeRpnHead.get_iou_target / get_vfl_loss / get_normalize_reg_loss (rangedet/symbol/head/builder.py:156-196,350-422, called per level
 * by get_fpn_loss :268-348) with vari_focal_loss (rangedet/symbol/head/loss.py:4-30), one class, iou_type 'bev'.  n = H * Wl, pixel
 * i = h * Wl + w in every layout (builder.py:122-141).  With x = logit, s = IoU target, m = mask, float32:
 *   s         = max over the frame's n_gt boxes of the cleaned (NaN / Inf / > 1 / < 0 -> 0) 8-point IoU of the box decoded from the
 *               pixel's deltas (rd_decode3d_bbox, is_bin = 0) -- for every pixel, the mask does not enter; behind block_grad
 *   norm_cls  = float(sum of mask over the batch) + 1, norm_reg = float(sum of reg_norm_weight over the batch) + 1 (:366,411)
 *   p = 1 / (1 + expf(-x)), Lp = logf(clip(p, 1e-6f, 1 - 1e-6f)), Lm = -x [x >= 0] - log1pf(expf(x - 2 x [x >= 0]))
 *   L0 = -(0.5 s Lp + 0.5 (1 - s) Lm) * 2;  vfl = L0 s (s > 0), L0 alpha |s - p|^gamma (s == 0);  cls_loss = vfl m / norm_cls
 *   x_r = delta - target, sigma = smooth_l1_scalar: sl1 = 0.5 sigma^2 x_r^2 (|x_r| < 1 / sigma^2), else |x_r| - 0.5 / sigma^2; |x_r| with l1
 *   reg_loss  = sl1 reg_weight reg_norm_weight / norm_reg * reg_loss_weight; channel c of pixel i pairs delta[b,i,c] with target[b,c,h,w]
 * and what MakeLoss (grad_scale, :374-378,417-421) sends back, c = [1e-6f <= p <= 1 - 1e-6f], dL0 = -(s c (1 - p) - (1 - s) p):
 *   d_logit   = scale_loss_shift cls_loss_weight m / norm_cls * (s dL0 (s > 0);  alpha (dL0 p^gamma + L0 gamma p^(gamma-1) p (1 - p)) (s == 0))
 *   d_delta   = scale_loss_shift reg_loss_weight reg_weight reg_norm_weight / norm_reg * (sigma^2 x_r inside, sign(x_r) outside or with l1)
 * The loss maps are not scaled by grad_scale (MakeLoss forward is the identity).  The batch strides (in floats) let a level be a slice
 * of the forward's flat (B,N) / (B,N,8) buffers (rd_head_out): pass base + n_off [* 8] and N [* 8].  p_host is read on the host at call
 * time.  stats: 4 floats on the device = norm_cls, norm_reg, sum(cls_loss), sum(reg_loss); every sum is accumulated in double in a fixed
 * order (no atomics), so two calls give the same bits.  All launches go on `stream`, nothing synchronises; the contents of ws on entry
 * do not matter.  d_logit, d_delta, iou_target and boxes10 (the decoded boxes, a diagnostic) may be NULL.
 * RD_ESHAPE: B < 1 or > 65535, H < 1, Wl < 1, n_gt outside 1..256, logit_bstride < n, delta_bstride < 8 n, delta_bstride % 4 != 0.
 * RD_EINVAL: a null required pointer, delta / d_delta not 16-byte aligned, ws not 8-byte aligned, smooth_l1_scalar <= 0.
 * RD_EWORKSPACE: ws_bytes < rd_rpn_loss_workspace_bytes(B, n).  Every check precedes the first launch. */
typedef struct {            /* read on the host at call time */
  float alpha, gamma;                       /* config:123-124 (1, 2) */
  float cls_loss_weight, reg_loss_weight;   /* config:126,125 (10, 8) */
  float smooth_l1_scalar;                   /* config:129 (3); MXNet smooth_l1: sigma = scalar */
  float scale_loss_shift;                   /* config:36,115 with builder.py:97: 128 in fp16 mode, else 1 */
  int l1;                                   /* builder.py:397-401: |x| instead of smooth_l1 */
} rd_loss_param_t;
size_t rd_rpn_loss_workspace_bytes(int B, long n);
int rd_rpn_loss(const float* logit, long logit_bstride, const float* delta, long delta_bstride, const float* pc, const float* gt_bbox,
                int n_gt, const float* mask, const float* reg_target, const float* reg_weight, const float* reg_norm_weight, int B, int H,
                int Wl, const rd_loss_param_t* p_host, float* cls_loss, float* reg_loss, float* d_logit, float* d_delta,
                float* iou_target, float* boxes10, float* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- backward of a head tower: conv weight gradient, output-conv backward, ReLU + norm-scale backward --------------------------------
 * A tower is four  relu(s[c] * conv3x3(x, W) + t[c])  layers at 128 channels and a 1x1 output conv with bias (rangedet/symbol/head/
 * builder.py:221-255: rpn_{cls,reg}_conv_{0..3}_lvl_*, rpn_cls_logit_lvl_* with 1 and rpn_reg_delta_lvl_* with 8 outputs); s, t the folded
 * normalisation.  Weight gradients are float32, as the optimiser keeps them under multi_precision (tools/train.py:358-360); activations
 * and their gradients are RD_BF16 or RD_F16, channels-last with a channel stride and offset like everywhere (both multiples of 8, the
 * tensors 16-byte aligned).  For one layer with z = conv3x3(x, W), y = relu(s z + t) and g = dL/dy:
 *   dz = g [y > 0] s[c]                                                  rd_relu_affine_bwd
 *   dW[co,ci,dh+1,dw+1] = sum_{b,h,w} dz[b,h,w,co] x[b,h+dh,w+dw,ci]      rd_conv3x3_bwd_weight (x zero outside the image)
 *   dx[b,h,w,ci] = sum_{co,dh,dw} dz[b,h-dh,w-dw,co] W[co,ci,dh+1,dw+1]   rd_conv3x3_bn_act_ex (RD_SCALE_FOLDED, no activation, zero shift) on the
 *                                                                        weight with its channel axes swapped and its taps flipped
 * and for the output conv out[b,p,o] = sum_c w[o,c] x[b,p,c] + bias[o] (rd_head_out): rd_head_out_bwd.
 * Every reduction is split over workgroups whose partial sums go to the caller's workspace and are added in index order by a second
 * launch: no atomics, two calls on the same inputs give the same bits, and the bits do not depend on the device's CU count.  All launches
 * go on `stream`, nothing synchronises, the contents of ws on entry do not matter.  Every check precedes the first launch.
 * Training-mode normalisation (batch statistics, the gradients of gamma and beta) is the next section.  The stride-(1,2) 3x3 conv of a
 * down-sampling BasicBlock: weight gradient rd_conv3x3_bwd_weight_ex, data gradient rd_deconv2d_bn_act_all on the weight read as a (3,4)
 * transposed-conv weight with a zero fourth column; its strided 1x1 shortcut runs the 1x1 calls on the pixel-pair view (channel stride
 * 2 cin).  The network's own transposed convs: rd_deconv_bwd_weight and the packers declared with it.  The Meta-Kernel unit
 * with the folded normalisation: rd_meta_kernel_bwd_data and rd_meta_kernel_bwd_params, at the end of this section.  The convs that read the
 * range image itself (res1_unit1's conv1 and projection, the level-0 concat conv): rd_conv_bwd_weight_narrow and
 * rd_conv3x3_bwd_weight_cat below, their device packers with the optimizer's.  The batch-statistics form of the Meta-Kernel's
 * 576-channel BatchNorm and the device re-pack of that unit follow the frozen form: rd_meta_kernel_stats .. rd_pack_meta_dev.
 *
 * rd_relu_affine_bwd: dz = round(float(g) * s[c]) where y > 0, else +0 -- one float32 product, one rounding.  y == NULL: no mask;
 * scale == NULL: 1 (a later normalisation-backward launch then feeds the conv primitives with y = scale = NULL).  C a multiple of 8.
 * dz may be g. */
int rd_relu_affine_bwd(const void* g, int g_cstride, int g_coff, const void* y, int y_cstride, int y_coff, const float* scale, void* dz,
                       int dz_cstride, int dz_coff, int B, int H, int W, int C, int dtype, void* stream);
/* dW (cout, cin, 3, 3) float32 of a stride-1, pad-1 conv with cin, cout in {64, 128} (else RD_ESHAPE), any B, H, W >= 1.  fp32
 * accumulation on the matrix cores over the pixel axis.  split: the most partial sums per output element (= workgroups per tap column
 * and 64 output channels); 0: the library's choice (512 workgroups in all).  The workspace holds split x 9 x cout x cin floats at most:
 * size it with the same split.  RD_EWORKSPACE: ws_bytes below that. */
size_t rd_conv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int cin, int cout, int split);
int rd_conv3x3_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                          int W, int cin, int cout, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
/* dW (cout, cin) float32 of a stride-1 1x1 conv (the projection shortcut of a backbone BasicBlock): dW[co,ci] = sum_{b,h,w} dz[b,h,w,co]
 * x[b,h,w,ci], cin, cout in {64, 128} (else RD_ESHAPE), any B, H, W >= 1; fp32 accumulation on the matrix cores over the flat pixel axis in
 * tiles of 64 pixels.  A workgroup owns all cout x cin outputs and a contiguous run of tiles, so every input byte is read once.  split:
 * the most partial sums per output element (= workgroups); 0: the library's choice, min(512, ceil(tiles / 8)).  The workspace holds
 * split x cout x cin floats at most; split, the absence of atomics and the determinism are those of rd_conv3x3_bwd_weight.  The data
 * gradient of the 1x1 conv is rd_conv2d_bn_act with kh = kw = 1 on the transposed weight packed by rd_pack_conv_weight_host. */
size_t rd_conv1x1_bwd_weight_workspace_bytes(int B, int H, int W, int cin, int cout, int split);
/* rd_conv3x3_bwd_weight with a stride: stride_w 1 gives its bytes with its partial count and workspace size; stride_w 2 is the weight
 * gradient of a 3x3 stride-(1,2) pad-1 conv (conv2 of a down-sampling BasicBlock), x (B, H, Win) and dz (B, H, Win / 2):
 *   dW[co,ci,ky,kx] = sum_{b,h,wo} dz[b,h,wo,co] x[b,h+ky-1,2wo+kx-1,ci]      (x zero outside the image)
 * Win odd with stride_w 2, stride_w outside {1, 2}, cin or cout outside {64, 128}: RD_ESHAPE.  The same kernel: a workgroup owns a tap
 * column and 64 output channels and reads x at twice the pixel stride; chunks, the split and the workspace (split x 9 x cout x cin floats
 * at most) are counted on the dz grid (B, 16-row strips, 64-pixel tiles of Win / stride_w).  No atomics, two calls give the same bytes. */
size_t rd_conv3x3_bwd_weight_ex_workspace_bytes(int B, int H, int Win, int cin, int cout, int stride_w, int split);
int rd_conv3x3_bwd_weight_ex(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                             int Win, int cin, int cout, int stride_w, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
int rd_conv1x1_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                          int W, int cin, int cout, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The weight gradient of the convs that read the range image itself: res1_unit1's conv1 (c -> 64, ksize 3) and projection shortcut
 * (c -> 64, ksize 1), and the range-image columns of the level-0 conv_0 (64 + c -> 128); c = 8 (Waymo) or 5 (KITTI).
 *   dW[co, dw_cin_off + ci, ky, kx] = sum_{b,h,w} dz[b,h,w,co] x[b,h+ky-p,w+kx-p,ci]     ksize 3: p = 1, x zero outside the image; ksize 1: p = 0
 * float32, stride 1.  dW is laid out (cout, dw_cin_stride, ksize, ksize); only channels [dw_cin_off, dw_cin_off + cin) are written, every
 * other element is left untouched.  cin 1..16, cout 64 or 128, ksize 1 or 3 (else RD_ESHAPE).  The kernel reads one 16-channel slot per
 * pixel, exactly as the forward does: x_coff % 8 == 0, x_cstride % 8 == 0, x_coff + 16 <= x_cstride; slot channels at or above cin may
 * hold any finite values, they reach no written element.  16-bit types only (else RD_EINVAL).
 * A different kernel from rd_conv3x3_bwd_weight (csrc/k_convbwd_narrow.h): a workgroup owns all of cout x (taps x slot) and a contiguous
 * run of (frame, 16-row strip, 64-pixel tile) chunks, so dz is read once and x once plus the halo rows of a strip; v_mfma_f32_16x16x32 with
 * one tap's slot as one N tile, fp32 accumulation over the pixel axis.  The reduction has rd_conv3x3_bwd_weight's contract: split is the
 * most partial sums per element (0: the library's choice, min(512, chunks)), partial images (split x ksize^2 x cout x cin floats at most)
 * go to the workspace and a second launch adds them in index order; no atomics, two calls give the same bytes, the bytes do not depend
 * on the CU count; RD_EWORKSPACE when ws_bytes is too small; the contents of ws on entry do not matter. */
size_t rd_conv_bwd_weight_narrow_workspace_bytes(int B, int H, int W, int cin, int cout, int ksize, int split);
int rd_conv_bwd_weight_narrow(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride,
                              int dw_cin_off, int B, int H, int W, int cin, int cout, int ksize, int split, int dtype, void* ws, size_t ws_bytes,
                              void* stream);
/* The weight gradient of the concat conv of rd_conv3x3_bn_act_cat: dW (cout, cin1 + cin2, 3, 3), cin1 64, cin2 1..16, cout 64 or 128 (else
 * RD_ESHAPE).  Channels [0, cin1) are bit for bit what rd_conv3x3_bwd_weight returns for (x1, dz) with the same split -- the same kernel,
 * its reduce writing at the channel stride -- and channels [cin1, cin1 + cin2) bit for bit what rd_conv_bwd_weight_narrow returns for
 * (x2, dz) with ksize 3; x2 is read as a 16-channel slot (x2_coff + 16 <= x2_cstride).  The workspace holds the partial images of both.
 * The data gradient towards x1 is the persistent forward launch on the flipped image of w[:, :cin1] (rd_pack_conv3x3_ex_host(flip(w[:,
 * :cin1]), NULL, cin1, cout, 1, cout, dtype)); the range image takes no gradient. */
size_t rd_conv3x3_bwd_weight_cat_workspace_bytes(int B, int H, int W, int cin1, int cin2, int cout, int split);
int rd_conv3x3_bwd_weight_cat(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                              const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H, int W, int cout, int split, int dtype,
                              void* ws, size_t ws_bytes, void* stream);
/* rd_conv3x3_bwd_weight_cat into a gradient laid out (cout, dw_cin_stride, 3, 3) with dw_cin_stride >= cin1 + cin2 (else RD_ESHAPE): the
 * same bits in channels [0, cin1 + cin2), channels [cin1 + cin2, dw_cin_stride) are never written.  For a master kept at the width the
 * concat forward reads (cin2 rounded up to 8: KITTI's c = 5 in 8), whose zero padding columns then keep a zero gradient.  The workspace is
 * that of rd_conv3x3_bwd_weight_cat. */
int rd_conv3x3_bwd_weight_cat_padded(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                                     const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride, int B, int H, int W, int cout,
                                     int split, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The backward of the network's transposed convs (the `agg` stages of the DLA backbone: Deconvolution -> BatchNorm -> ReLU -> add(skip, .)).
 * x (B, H, Win, cin), W (cin, cout, 3, kw) in MXNet's Deconvolution layout, stride (1, s), pad (1, p) with kw - 2 p == s, so Wout = s Win;
 * dz is the gradient at the output, (B, H, s Win, cout).  The two forms (kw, s, p) = (4, 2, 1) and (8, 4, 2) at the channel pairs of the
 * shipped configs -- (3,8): 128 -> 128 and 128 -> 64; (3,4): 128 -> 64 and 64 -> 64 -- anything else is RD_ESHAPE.
 *   forward   z[b,hi-1+kh,s wi-p+kw,co] += x[b,hi,wi,ci] W[ci,co,kh,kw]                       rd_deconv2d_bn_act_all
 *   dW[ci,co,kh,kw] = sum_{b,hi,wi} x[b,hi,wi,ci] dz[b,hi-1+kh,s wi-p+kw,co]                   rd_deconv_bwd_weight (dz zero outside the image)
 *   dx[b,hi,wi,ci] = sum_{co,kh,kw} dz[b,hi-1+kh,s wi-p+kw,co] W[ci,co,kh,kw]                  rd_conv3x3_bn_act_ex on the s-pixel view
 * rd_deconv_bwd_weight is the kernel of rd_conv3x3_bwd_weight_ex with the two tensors swapped: the deconv input is the narrow tensor and its
 * channels the M axis, dz the wide one, read at pixel stride s with the column offsets kw - p.  A workgroup owns ONE tap column kw and 64
 * input channels; its contract is that of rd_conv3x3_bwd_weight_ex in every respect: fp32 accumulation on the matrix cores over the pixel
 * axis, per-workgroup partial sums in ws added in index order by a second launch, no atomics, two calls give the same bytes.  There are
 * min(split or 512 / (kw cin / 64), chunks) partial sums with chunks = B ceil(H / 16) ceil(Win / 64) counted on the x grid, and the workspace
 * holds that many x 3 kw x cin x cout floats.
 * The data gradient: dense dz [H][s Win][cout] IS [H][Win][s cout] -- view channel e cout + co is output pixel s wv + e -- and
 *   dx = conv3x3(view, Wv),  Wv[ci, e cout + co, kh, dwv + 1] = W[ci,co,kh, s dwv + e + p] where 0 <= s dwv + e + p < kw, else 0
 * a stride-1 rd_conv3x3_bn_act_ex launch with cin = s cout, cout = cin, RD_SCALE_FOLDED, zero shift, no activation (RD_ADD with a residual adds
 * another gradient of x in the epilogue).  rd_pack_deconv_data_grad_host writes its weight image: byte for byte what
 * rd_pack_conv3x3_ex_host(Wv, NULL, cin, s cout, 1, s cout, dtype) writes, rd_conv3x3_ex_packed_bytes(s cout, cin, 1, s cout) bytes.  One
 * third of Wv's (view channel block, tap column) pairs are structurally zero in both forms; the launch multiplies them all the same.
 * rd_pack_deconv_dev: one launch on a device-resident float32 master.  data_grad == 0: the stride_w forward phase images, phase ph at
 * ph * w_phase_bytes (a multiple of 16, at least rd_conv_packed_bytes(6, cin, cout, dtype)), each byte for byte what
 * rd_pack_deconv_weight_folded_host(w, NULL, ..., ph, dtype, .) writes, zero tail included; data_grad != 0: the image above, byte for byte
 * the host one (w_phase_bytes is not read). */
size_t rd_deconv_bwd_weight_workspace_bytes(int B, int H, int Win, int cin, int cout, int kw, int stride_w, int pad_w, int split);
int rd_deconv_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                         int Win, int cin, int cout, int kw, int stride_w, int pad_w, int split, int dtype, void* ws, size_t ws_bytes,
                         void* stream);
int rd_pack_deconv_data_grad_host(const float* w, int cin, int cout, int kw, int stride_w, int pad_w, int dtype, void* out);
int rd_pack_deconv_dev(const float* w_dev, int cin, int cout, int kw, int stride_w, int pad_w, int data_grad, long w_phase_bytes, int dtype,
                       void* out_dev, void* stream);
/* Backward of rd_head_out.  d_out: float32 at d_out[b*out_batch_stride + (n_off + h*W + w)*nout + o], exactly as rd_head_out writes `out`
 * -- so rd_rpn_loss's flat d_logit / d_delta buffers are read in place.  x: the output conv's input (the post-ReLU output of the last
 * tower conv), w (nout, cin) float32.  nout 1..8, cin 64 or 128 (else RD_ESHAPE).
 *   dx[b,p,c] = sum_o d_out[b,p,o] w[o,c]   in the activation type; with relu_mask != 0 times [x > 0], with scale != NULL times scale[c]
 *               (float32, rounded once at the end): with both, dx is the dz of the last tower conv.  dx may be NULL.
 *   dw[o,c] = sum_{b,p} d_out[b,p,o] x[b,p,c],  dbias[o] = sum_{b,p} d_out[b,p,o]   float32 */
size_t rd_head_out_bwd_workspace_bytes(int B, int H, int W, int cin, int nout);
int rd_head_out_bwd(const float* d_out, long out_batch_stride, long n_off, const void* x, int x_cstride, int x_coff, const float* w,
                    int relu_mask, const float* scale, void* dx, int dx_cstride, int dx_coff, float* dw, float* dbias, int B, int H,
                    int W, int cin, int nout, int dtype, void* ws, size_t ws_bytes, void* stream);
/* Backward of the Meta-Kernel unit (rd_meta_kernel_fwd) up to z, with the folded normalisation s1, t1 of its 576-channel BatchNorm:
 * dz = dL/dz comes from rd_relu_affine_bwd(g, y, s2).  RD_BF16 / RD_F16 only (RD_F32: RD_EINVAL).  The packed block of the backward is
 * made on the host from the same nine arrays as rd_pack_meta_host (s2, t2 are not read); the kernels evaluate w_k and r_k under the
 * forward's arithmetic contract (the packer's rounded s1 W1 and A, h rounded to the type, the centre tap's folded constant), so the
 * gradient is that of the function rd_meta_kernel_fwd computes.  csrc/k_metabwd.h lists every 16-bit rounding.
 *   rd_meta_kernel_bwd_data    ddata (B, H, W, 64 at g_coff) in the activation type, rounded once; residual (may be NULL): a tensor of
 *                              the same shape added in float32 before that rounding (the identity shortcut's gradient).  No workspace.
 *   rd_meta_kernel_bwd_params  float32: dA (64, 576) [aggregation_conv1], dW1 (64, 32), db1 (64) [mlp1], dW0 (32, 3), db0 (32) [mlp0],
 *                              dt1 (576) = dL/dt1 and dq1 (576) = sum dr (r - t1) (index c 9 + k; dq1 / gamma is the BatchNorm's dgamma
 *                              under frozen statistics, and both are the sums the batch-statistics form needs).
 * split: the most partial sums per output element, as in rd_conv3x3_bwd_weight (0: the library's choice, 64); the workspace holds
 * split x 9 x 6464 floats at most and only partial sums.  No atomics, two calls give the same bytes, and the bytes do not depend on the
 * CU count.  RD_EINVAL: a null pointer, a misaligned tensor, split < 0; RD_ESHAPE: B, H or W < 1, a channel stride or offset that is no
 * multiple of 8 or coff + 64 > cstride; RD_EWORKSPACE: ws_bytes below rd_meta_kernel_bwd_workspace_bytes(B, H, W, split). */
size_t rd_meta_bwd_packed_bytes(int dtype);
int rd_pack_meta_bwd_host(const float* w0, const float* b0, const float* w1, const float* b1, const float* s1, const float* t1,
                          const float* agg, const float* s2, const float* t2, int dtype, void* packed_host);
int rd_meta_kernel_bwd_data(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                            const void* packed_bwd, const void* residual, int r_cstride, int r_coff, void* ddata, int g_cstride, int g_coff,
                            int B, int H, int W, int dtype, void* stream);
size_t rd_meta_kernel_bwd_workspace_bytes(int B, int H, int W, int split);
int rd_meta_kernel_bwd_params(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                              const void* packed_bwd, float* dA, float* dW1, float* db1, float* dW0, float* db0, float* dt1, float* dq1, int B,
                              int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The Meta-Kernel unit in TRAINING mode: the 576-channel BatchNorm normalises q_k[c] = data[n_k][c] * w_k[c] with the batch's own
 * statistics (use_global_stats = False).  RD_BF16 / RD_F16 only (RD_F32: RD_EINVAL).  Every launch reads the packed blocks made with
 * s1 = s2 = 1, t1 = t2 = 0 -- packed_fwd: rd_pack_meta_host's, packed_bwd: rd_pack_meta_bwd_host's, or both from rd_pack_meta_dev -- so a
 * block depends on the parameters only, and takes the normalisation as float32 device vectors of 576 values, index c 9 + k, however they
 * were computed: a1 = gamma1 rstd1, bb1 = fmaf(-mean1, a1, beta1) (rd_bn_fold with C = 576 on rd_meta_kernel_stats' output), mean1, rstd1,
 * c1 = dbeta1 / n, c2 = dgamma1 / n (n = B H W).  The arithmetic and every 16-bit rounding point: csrc/k_metatrain.h, k_metabwd.h.
 *   rd_meta_kernel_stats             mean1, var1 (biased, 576 each) over all n pixels of q; a padded tap counts with q = 0.  Sums shifted by
 *                                    a per-workgroup pilot, per-workgroup partials, a fixed-order merge launch.
 *   rd_meta_kernel_fwd_train         z (B, H, W, 64 at z_coff) = round(sum A relu(round(fmaf(q, a1, bb1)))): no affine, no ReLU; the second
 *                                    BatchNorm is rd_bn_stats, rd_bn_fold, rd_affine_relu with C = 64 on z.
 *   rd_meta_kernel_bwd_sums          pass A, dz from rd_bn_relu_bwd(g, z, ..): dA (64, 576), dbeta1, dgamma1 (576: the gradients of the
 *                                    BatchNorm's beta and gamma), c1, c2 (576)
 *   rd_meta_kernel_bwd_params_train  pass B: dW1 (64, 32), db1 (64), dW0 (32, 3), db0 (32)
 *   rd_meta_kernel_bwd_data_train    ddata in the activation type, rounded once; residual as in rd_meta_kernel_bwd_data
 *   rd_pack_meta_dev                 both blocks from the device-resident float32 masters w0 (32, 3), b0 (32), w1 (64, 32), b1 (64),
 *                                    agg (64, 576): byte for byte the host packers' output for s1 = s2 = 1, t1 = t2 = 0
 * split as in rd_meta_kernel_bwd_params; the workspaces hold split x 9 x 256 (statistics) and split x 9 x 4224 (pass A and pass B) floats
 * at most, partial sums only.  No atomics, two calls give the same bytes, the bytes do not depend on the CU count.  Status codes as above. */
size_t rd_meta_kernel_stats_workspace_bytes(int B, int H, int W, int split);
int rd_meta_kernel_stats(const void* data, int d_cstride, int d_coff, const float* coord_nchw, const void* packed_bwd, float* mean1,
                         float* var1, int B, int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
int rd_meta_kernel_fwd_train(const void* data, int d_cstride, int d_coff, const float* coord_nchw, const void* packed_fwd,
                             const void* packed_bwd, const float* a1, const float* bb1, void* z, int z_cstride, int z_coff, int B, int H,
                             int W, int dtype, void* stream);
size_t rd_meta_kernel_bwd_train_workspace_bytes(int B, int H, int W, int split);
int rd_meta_kernel_bwd_sums(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                            const void* packed_bwd, const float* a1, const float* bb1, const float* mean1, const float* rstd1, float* dA,
                            float* dbeta1, float* dgamma1, float* c1, float* c2, int B, int H, int W, int split, int dtype, void* ws,
                            size_t ws_bytes, void* stream);
int rd_meta_kernel_bwd_params_train(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff,
                                    const float* coord_nchw, const void* packed_bwd, const float* a1, const float* bb1, const float* mean1,
                                    const float* rstd1, const float* c1, const float* c2, float* dW1, float* db1, float* dW0, float* db0,
                                    int B, int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
int rd_meta_kernel_bwd_data_train(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff,
                                  const float* coord_nchw, const void* packed_bwd, const float* a1, const float* bb1, const float* mean1,
                                  const float* rstd1, const float* c1, const float* c2, const void* residual, int r_cstride, int r_coff,
                                  void* ddata, int g_cstride, int g_coff, int B, int H, int W, int dtype, void* stream);
int rd_pack_meta_dev(const float* w0, const float* b0, const float* w1, const float* b1, const float* agg, void* packed_fwd,
                     void* packed_bwd, int dtype, void* stream);

/* ---- training-mode batch norm of a head-tower layer, forward and backward ----------------------------------------------------------------
 * The reference builds every tower layer with normalizer_factory(type="localbn") (mxnext/complicate.py:26-45): mx.sym.BatchNorm with
 * fix_gamma=False, use_global_stats=False, momentum 0.9, eps 1e-5 + 1e-10, named <conv name>_bn (mxnext/simple.py:502-508,
 * head/builder.py:212-240).  z = conv3x3(x, W) is the unscaled conv output in the activation type (rd_conv3x3_bn_act_ex with RD_SCALE_FOLDED,
 * an unscaled weight image, zero shift, no activation); n = B H W; everything below is float32, and every fused multiply-add is an fmaf:
 * an operation not written fmaf is rounded on its own.  The exact operation order is in rangedet_amd/csrc/k_norm.h.
 *   forward    mean[c], var[c] (biased)                                          rd_bn_stats
 *              rstd = 1 / sqrtf(var + eps), a = gamma rstd, b = fmaf(-mean, a, beta), moving statistics    rd_bn_fold
 *              y = round(max(fmaf(z, a, b), 0))                                  rd_affine_relu
 *   backward   gy = g [fmaf(z, a, b) > 0], zh = (z - mean) rstd, dbeta = sum gy, dgamma = sum gy zh,
 *              dz = round(gamma rstd (gy - dbeta / n - zh dgamma / n))           rd_bn_relu_bwd
 * dz then feeds rd_conv3x3_bwd_weight and the data gradient directly (no rd_relu_affine_bwd).
 * Tensors are RD_BF16 / RD_F16 channels-last with a channel stride and offset (multiples of 8, 16-byte aligned).  C in {8, 16, 32, 64, 128,
 * 256}, else RD_ESHAPE.  Every check precedes the first launch, nothing synchronises, the contents of ws on entry do not matter, there are
 * no atomics: a reduction writes per-workgroup partial sums to ws and a second launch adds them as a tree of fixed shape.  split: the
 * most partial sums per channel; 0: the library's choice (1024).  There are min(split or 1024, ceil(n / 64)) of them, a function of the shape
 * and of split only -- never of the device -- and two calls give the same bytes.  Size the workspace with the same split.
 *
 * rd_bn_stats: one sweep over z.  Each workgroup shifts its sums by a pilot value, the mean of PL = 2048 / C of its pixels spread evenly over
 * its run, and the final launch merges the (pilot, sum, sum of squares) triples about the first workgroup's mean; E[z^2] - E[z]^2 about
 * zero is never formed.  A channel holding one small integer everywhere gives that integer as mean in every bit and var == 0. */
size_t rd_bn_stats_workspace_bytes(int B, int H, int W, int C, int split);
int rd_bn_stats(const void* z, int z_cstride, int z_coff, float* mean, float* var, int B, int H, int W, int C, int split, int dtype, void* ws,
                size_t ws_bytes, void* stream);
/* One launch on C-element float32 device vectors, no host round trip:
 *   rstd = 1.0f / sqrtf(var + eps);  a = gamma * rstd;  b = fmaf(-mean, a, beta)
 *   om = 1.0f - momentum;  moving_mean = fmaf(moving_mean, momentum, mean * om)
 *   vu = unbiased ? var * ((float)n / (float)(n - 1)) : var;  moving_var = fmaf(moving_var, momentum, vu * om)
 * moving_mean / moving_var are updated in place; either may be NULL (left alone).  unbiased != 0 needs n >= 2 (else RD_ESHAPE). */
int rd_bn_fold(const float* mean, const float* var, const float* gamma, const float* beta, float eps, float momentum, long n, int unbiased,
               float* rstd, float* a, float* b, float* moving_mean, float* moving_var, int C, void* stream);
/* y = round(relu ? max(fmaf(z, a[c], b[c]), 0) : fmaf(z, a[c], b[c])): one fused multiply-add, one rounding.  y may be z. */
int rd_affine_relu(const void* z, int z_cstride, int z_coff, const float* a, const float* b, int relu, void* y, int y_cstride, int y_coff,
                   int B, int H, int W, int C, int dtype, void* stream);
/* Three launches: partial sums, their fixed-order sum into dbeta / dgamma, the elementwise dz.  g = dL/dy; a, b, mean, rstd as rd_bn_fold
 * left them.  The ReLU mask is recomputed as [fmaf(z, a, b) > 0] -- y is not read; this differs from a mask on the stored y only where a
 * positive float32 value rounds to zero in the 16-bit type (RD_F16: below 2^-25).  relu == 0: no mask (a and b may then be NULL).
 *   gy = mask ? g : 0;  zh = (z - mean) * rstd;  dbeta = sum gy;  dgamma = sum fmaf(gy, zh, .)
 *   dz = round(gr * fmaf(-zh, c2, gy - c1))  with c1 = dbeta / (float)n, c2 = dgamma / (float)n, gr = gamma * rstd
 * dz may be g. */
size_t rd_bn_relu_bwd_workspace_bytes(int B, int H, int W, int C, int split);
int rd_bn_relu_bwd(const void* g, int g_cstride, int g_coff, const void* z, int z_cstride, int z_coff, const float* a, const float* b,
                   const float* mean, const float* rstd, const float* gamma, int relu, void* dz, int dz_cstride, int dz_coff, float* dgamma,
                   float* dbeta, int B, int H, int W, int C, int split, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The residual form: the second BatchNorm of a backbone BasicBlock (rangedet/symbol/backbone/dla_backbone.py:18-56: conv2 -> BN -> + shortcut
 * -> ReLU).  r is the shortcut in the activation type, a channels-last tensor with its own channel stride and offset: the block input
 * (identity shortcut, ar = br = NULL) or the 16-bit output zs of the 1x1 projection conv, whose own BatchNorm is folded into ar, br
 * (rd_bn_stats and rd_bn_fold on zs).  Per element, float32, every operation not written fmaf rounded on its own:
 *   t = fmaf(z, a, b);  u = ar ? fmaf(r, ar, br) : (float)r;  v = t + u;  y = round(relu ? max(v, 0) : v)
 * y may be z.  C, alignment and the status codes are those of rd_affine_relu; ar without br (or the reverse) is RD_EINVAL. */
int rd_affine_add_relu(const void* z, int z_cstride, int z_coff, const float* a, const float* b, const void* r, int r_cstride, int r_coff,
                       const float* ar, const float* br, int relu, void* y, int y_cstride, int y_coff, int B, int H, int W, int C, int dtype,
                       void* stream);
/* The join of an aggregation stage (dla_backbone.py agg_stage: Deconvolution -> BatchNorm -> ReLU -> add(skip, .)): the ReLU BEFORE the add.
 *   y = round(max(fmaf(z, a[c], b[c]), 0) + (float)r)      one fused multiply-add, one float32 add, one rounding
 * max(t, 0) is t where t > 0 and +0 elsewhere.  r has its own channel stride and offset; y may be z.  C, alignment and the status codes are
 * those of rd_affine_relu.  It needs no backward launch: the up-branch gradient is rd_bn_relu_bwd(g, z, ...), which recomputes the mask
 * [fmaf(z, a, b) > 0] from z, and the skip gradient is g itself. */
int rd_affine_relu_add(const void* z, int z_cstride, int z_coff, const float* a, const float* b, const void* r, int r_cstride, int r_coff,
                       void* y, int y_cstride, int y_coff, int B, int H, int W, int C, int dtype, void* stream);
/* The backward of rd_affine_add_relu, three launches like rd_bn_relu_bwd: ONE sweep over g, z and r gives the two (identity) or three (projection) partial sums
 * per channel, a fixed-tree launch adds them, one elementwise launch writes dz and dr together.  g = dL/dy; a, b, mean, rstd, gamma of the
 * main branch and, for a projection shortcut, ar, br, mean_r, rstd_r, gamma_r of the shortcut's BatchNorm -- these five and the outputs
 * dgamma_r, dbeta_r are all given or all NULL (else RD_EINVAL).
 *   m = [fmaf(z, a, b) + u > 0]   with u and the sum formed exactly as rd_affine_add_relu forms v; y is not read
 *   gy = m ? g : 0;  zh = (z - mean) * rstd;  dbeta = sum gy;  dgamma = sum fmaf(gy, zh, .)
 *   c1 = dbeta / (float)n;  c2 = dgamma / (float)n;  dz = round(gamma * rstd * fmaf(-zh, c2, gy - c1))
 *   identity:    dr = gy                                             (the bits of g, or +0)
 *   projection:  zhr = (r - mean_r) * rstd_r;  dgamma_r = sum fmaf(gy, zhr, .);  dbeta_r = dbeta (the same bytes)
 *                dr = round(gamma_r * rstd_r * fmaf(-zhr, dgamma_r / (float)n, gy - c1))
 * The partial count is that of rd_bn_relu_bwd (min(split or 1024, ceil(n / 64))), the workspace holds 2 or 3 x that x C floats
 * (projection != 0: 3); no atomics, two calls give the same bytes.  dz may be g. */
size_t rd_bn_add_relu_bwd_workspace_bytes(int B, int H, int W, int C, int split, int projection);
int rd_bn_add_relu_bwd(const void* g, int g_cstride, int g_coff, const void* z, int z_cstride, int z_coff, const void* r, int r_cstride,
                       int r_coff, const float* a, const float* b, const float* mean, const float* rstd, const float* gamma, const float* ar,
                       const float* br, const float* mean_r, const float* rstd_r, const float* gamma_r, void* dz, int dz_cstride, int dz_coff,
                       void* dr, int dr_cstride, int dr_coff, float* dgamma, float* dbeta, float* dgamma_r, float* dbeta_r, int B, int H, int W,
                       int C, int split, int dtype, void* ws, size_t ws_bytes, void* stream);

/* ---- the parameter update of the head towers: multi-tensor SGD with momentum, conv weight images re-packed on the device ---------------
 * The reference trains with mx.optimizer `sgd`: momentum, wd, rescale_grad, clip_gradient and, under fp16, multi_precision -- float32
 * master weights and momenta beside the 16-bit weights the network computes with (tools/train.py:306-365; OptimizeParam.optimizer in
 * every config under config/rangedet/: momentum = 0.9, wd = 0.00001, clip_gradient = 35, rangedet_veh_wo_aug_4_18e.py:179-184).  Per
 * element, float32, the arithmetic of MXNet's mp_sgd_mom_update operator as documented (MXNet is not available to this project: not
 * pinned by a run of the reference):
 *   g   = rescale_grad * grad
 *   g   = clip_gradient >= 0 ? (g > clip ? clip : (g < -clip ? -clip : g)) : g
 *   mom = momentum * mom - (lr_t * wd_t) * w - lr_t * g          left to right
 *   w   = w + mom
 * with lr_t = lr * lr_mult and wd_t = wd * wd_mult of the tensor.  Every operation is one float32 rounding in that order, nothing is
 * fused, so the result equals a float32 restatement bit for bit.  A NaN gradient propagates; so does inf when clip_gradient < 0.
 *
 * All tensors of a step are listed in a table that rd_sgd_table_host writes into caller memory of rd_sgd_table_bytes bytes; the caller
 * uploads it once (8-byte aligned) and keeps the host copy, which rd_sgd_mom_update reads for the launch geometry.  The table maps
 * 1024-element chunks to (tensor, offset): one launch of one workgroup per chunk updates every tensor, whatever their number.  weight,
 * grad and mom are float32 device buffers of n elements, 16-byte aligned (else RD_EINVAL; n <= 0: RD_EINVAL).  The scalars of the step
 * are by-value arguments: a new learning rate needs no new table.
 *
 * A tensor that is a (cout, cin, 3, 3) conv weight with cin, cout in {64, 128} (n = 9 cout cin) may name 16-bit weight images, which a
 * second launch over the same table rewrites from the updated weight: pack_fwd, byte for byte what rd_pack_conv3x3_ex_host(w, fold_scale,
 * cout, cin, 1, cin, dtype) writes (fold_scale: cout device floats or NULL; the product is formed in float32, then rounded to nearest
 * even), and pack_bwd, the image of the data gradient -- the same packer on the weight with its channel axes swapped and its taps flipped,
 * no scale.  Each is rd_conv3x3_ex_packed_bytes(cin, cout, 1, cin) bytes, the zero tail included: the step writes all of them.  Other
 * channel counts (the <= 16-channel body form, the 72-channel concat) and the images of other launch forms (stride-2 pair view, M16) are
 * refused with RD_ESHAPE.  A (cout, cin, 1, 1) weight of the same channel counts (n = cout cin: the tap count of an entry follows from n)
 * may name images too: pack_fwd, byte for byte what rd_pack_conv_weight_host(w, cout, cin, 1, 1, dtype) writes (rd_conv_packed_bytes(1, cin,
 * cout, dtype) bytes, zero tail included), and pack_bwd, the same packer on the transposed (cin, cout) weight: what rd_conv2d_bn_act with
 * kh = kw = 1 reads for the conv and for its data gradient.
 * stride_w == 2 on a (C, C, 3, 3) weight, C 64 or 128 (conv2 of a down-sampling BasicBlock; cin != cout or a 1x1 weight: RD_ESHAPE) names
 * the images of the strided launches instead: pack_fwd, byte for byte what rd_pack_conv3x3_ex_host(w, fold_scale, C, C, 2, C, dtype) writes
 * (the pixel-pair view in the body form rd_conv3x3_bn_act_ex takes at stride_w 2; rd_conv3x3_ex_packed_bytes(C, C, 2, C) bytes), and
 * pack_bwd, the two phase images rd_pack_deconv_weight_folded_host(w' , NULL, C, C, 3, 4, 2, 1, phase, dtype, .) writes for w' = w read as
 * (Cin, Cout, 3, 3) with a zero column appended at kx = 3, phase 1 starting rd_conv_packed_bytes(6, C, C, dtype) bytes after phase 0: what
 * rd_deconv2d_bn_act_all reads as the data gradient of the strided conv.  Zero fill and zero tails are written too.  stride_w is the last
 * field: a caller that fills the eleven fields before it and zeroes the rest gets the table it got before.
 * A step is two launches at most; the library allocates nothing and never synchronises; every check precedes
 * the first launch. */
typedef struct {
  void* weight;             /* float32 device buffers of n elements */
  const void* grad;
  void* mom;
  long n;
  float lr_mult, wd_mult;
  int cout, cin;            /* read only when an image is named */
  void* pack_fwd;           /* device images, or NULL */
  void* pack_bwd;
  const float* fold_scale;  /* device, cout values, or NULL; needs pack_fwd */
  int stride_w;             /* 0 or 1: the images above; 2: the images of a (C, C, 3, 3) stride-(1,2) conv, see above */
} rd_sgd_tensor_t;
size_t rd_sgd_table_bytes(const rd_sgd_tensor_t* tensors, int nt);   /* 0: refused (rd_last_error_string says why) */
int rd_sgd_table_host(const rd_sgd_tensor_t* tensors, int nt, int dtype, void* out);   /* dtype: that of the images */
int rd_sgd_mom_update(const void* table_dev, const void* table_host, float lr, float momentum, float wd, float rescale_grad,
                      float clip_gradient, void* stream);
/* One image of a device-resident (cout, cin, 3, 3) float32 weight, cin, cout in {64, 128}: flip == 0 the forward image (fold_scale_dev
 * or NULL), flip != 0 the data-gradient image (fold_scale_dev must be NULL).  One launch, the zero tail included. */
int rd_pack_conv3x3_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin, int flip, int dtype, void* out_dev, void* stream);
/* The launch images of the convs that read the range image, from device-resident float32 masters: one launch each, the zero fill behind
 * the weights and the zero tail included; byte for byte the host packers' images:
 *   rd_pack_conv_narrow_dev, ksize 3    rd_pack_conv3x3_ex_host(w, s, cout, cin, 1, cin, dtype), the <= 16-channel body form (cin 1..16)
 *   rd_pack_conv_narrow_dev, ksize 1    rd_pack_conv_weight_host(w, cout, cin, 1, 1, dtype); fold_scale_dev must be NULL (else RD_EINVAL)
 *   rd_pack_conv3x3_cat_dev, data_grad 0   rd_pack_conv3x3_cat_host(w, s, cout, cin1, cin2, dtype); w (cout, cin1 + cin2, 3, 3), cin1 64, cin2 a
 *                                          multiple of 8 as the forward requires (else RD_ESHAPE)
 *   rd_pack_conv3x3_cat_dev, data_grad 1   rd_pack_conv3x3_ex_host(flip(w[:, :cin1]), NULL, cin1, cout, 1, cout, dtype), the image of the data
 *                                          gradient towards x1 (cin2 1..16 only sets the master's channel stride); fold_scale_dev must be NULL
 * A trap in the host packers: they choose the <= 16-channel and the concat body layouts only when they are given a fold scale, while the
 * forward launches always read those layouts under RD_SCALE_FOLDED.  The unscaled training image is therefore the host packer called with a
 * fold scale of ONES (the product by 1.0f is exact), and these two calls take fold_scale_dev == NULL to mean exactly that. */
int rd_pack_conv_narrow_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin, int ksize, int dtype, void* out_dev, void* stream);
int rd_pack_conv3x3_cat_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin1, int cin2, int data_grad, int dtype,
                            void* out_dev, void* stream);

/* ---- per-kernel timing (HIP events on the launch stream; used by bench.py's roofline block) --------- */
#define RD_PROF_CONV 0
#define RD_PROF_META 1
#define RD_PROF_HEAD_OUT 2
#define RD_PROF_SORT 3
#define RD_PROF_DECODE 4
#define RD_PROF_WNMS 5
#define RD_PROF_LAYOUT 6
#define RD_PROF_CONV3 7 /* the persistent 3x3 stride-1 bf16 kernel (its launches are NOT counted in RD_PROF_CONV) */
#define RD_PROF_BLOCK 8 /* the fused BasicBlock kernel (rd_block64_bn_act) */
#define RD_PROF_NKINDS 9
int rd_prof_enable(int on);
int rd_prof_reset(void);
/* synchronises the recorded events; total_ms / launches per kind */
int rd_prof_get(int kind, double* total_ms, long* launches);

#ifdef __cplusplus
}
#endif
#endif /* RANGEDET_HIP_H_ */
