// librangedet_hip.so -- C ABI (include/rangedet_hip.h) over the hand-written gfx950 kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared rd_api.hip -o librangedet_hip.so
#include "k_conv1.h"
#include "k_block.h"
#include "k_assign.h"
#include "k_input.h"
#include "k_target.h"
#include "k_rangeimg.h"
#include "k_nms3d.h"
#include "k_meta.h"
#include "k_misc.h"
#include "k_riou.h"
#include "k_loss.h"
#include "k_convbwd.h"
#include "k_convbwd_narrow.h"
#include "k_metabwd.h"
#include "k_metatrain.h"
#include "k_norm.h"
#include "k_optim.h"
#include "k_sort.h"
#include "k_wnms.h"

#include <algorithm>
#include <string>
#include <numeric>

using namespace rd;

namespace rd {
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t wnms_ws_bytes(int cap) {
  const size_t nw = (size_t)(cap + 63) / 64;
  return align256((size_t)cap * PREP_F * 4) + 3 * align256((size_t)cap * nw * 8) + 4 * align256((size_t)cap * 4) +
         align256(((size_t)cap + 2) * 8 + 3 * ((size_t)cap / 32 + 2) * 4) + align256(nw * 8) + 256 + align256(sort_ws_bytes(cap)) + 256;
}
inline WnmsWs wnms_ws_carve(void* ws, int cap) {
  WnmsWs w;
  const size_t nw = (size_t)(cap + 63) / 64;
  unsigned char* p = (unsigned char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  w.nwcap = (int)nw;
  w.prep = (float*)p; p += align256((size_t)cap * PREP_F * 4);
  w.thr = (unsigned long long*)p; p += align256((size_t)cap * nw * 8);
  w.vote = (unsigned long long*)p; p += align256((size_t)cap * nw * 8);
  w.snap = (unsigned long long*)p; p += align256((size_t)cap * nw * 8);
  w.keep_q = (int*)p; p += align256((size_t)cap * 4);
  w.order = (int*)p; p += align256((size_t)cap * 4);
  w.alive = (int*)p; p += align256((size_t)cap * 4);
  w.ovf = (int*)p; p += align256((size_t)cap * 4);
  // merge overflow list / tie-order keys (cap + 2 ints + cap + 2 floats, or cap floats + cap ints + a cap-bit map)
  w.scratch = (int*)p; p += align256(((size_t)cap + 2) * 8 + 3 * ((size_t)cap / 32 + 2) * 4);
  w.supp_state = (unsigned long long*)p; p += align256(nw * 8);
  w.nalive = (int*)p; w.novf = (int*)p + 1; p += 256;
  w.sort_ws = p;
  return w;
}
inline void allow_conv_lds() {   // the generic tap kernel (the persistent 3x3 kernel does this per instantiation, k_conv3.h c3_go)
  static std::atomic<unsigned long long> seen{0};
  once_per_device(seen, [] {
    allow_big_lds(conv_taps_kernel<RD_BF16, 4, 3>); allow_big_lds(conv_taps_kernel<RD_BF16, 4, 8>);
    allow_big_lds(conv_taps_kernel<RD_F16, 4, 3>); allow_big_lds(conv_taps_kernel<RD_F16, 4, 8>);
    allow_big_lds(conv_taps_kernel<RD_F32, 4, 8>); allow_big_lds(conv_taps_kernel<RD_F32, 4, 3>);
  });
}
}  // namespace rd

extern "C" {

int rd_version(void) { return 100; }
const char* rd_last_error_string(void) { return rd::err_buf(); }

// ---- layout ---------------------------------------------------------------------------------------------
int rd_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int dst_cstride, int dst_coff,
                    int zero_pad, int dst_dtype, void* stream) {
  RD_REQUIRE(src && dst, RD_EINVAL, "nchw_to_nhwc: null pointer");
  RD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && zero_pad >= 0, RD_ESHAPE, "nchw_to_nhwc: bad shape");
  RD_REQUIRE(dst_coff >= 0 && dst_coff + C + zero_pad <= dst_cstride, RD_ESHAPE, "nchw_to_nhwc: channels exceed stride");
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W, total = (long)B * (C + zero_pad) * HW;
  const int grid = (int)std::min<long>((total + 255) / 256, 8192);
  ProfScope ps(RD_PROF_LAYOUT, st);
  {  // few channels, slot-aligned destination: pixel-per-thread variant with 16-byte stores
    const int ch = ch_per_slot(dst_dtype), ctot = C + zero_pad;
    if ((is_h16(dst_dtype) || dst_dtype == RD_F32) && ctot % ch == 0 && ctot / ch <= 2 && dst_cstride % ch == 0 && dst_coff % ch == 0) {
      const long npix = (long)B * HW;
      const int g2 = (int)std::min<long>((npix + 255) / 256, 8192);
#define RD_PX(DT, NS) hipLaunchKernelGGL((nchw_to_nhwc_px_kernel<DT, NS>), dim3(g2), dim3(256), 0, st, src, dst, C, HW, dst_cstride, dst_coff, npix)
      if (dst_dtype == RD_BF16) { if (ctot / ch == 1) RD_PX(RD_BF16, 1); else RD_PX(RD_BF16, 2); }
      else if (dst_dtype == RD_F16) { if (ctot / ch == 1) RD_PX(RD_F16, 1); else RD_PX(RD_F16, 2); }
      else { if (ctot / ch == 1) RD_PX(RD_F32, 1); else RD_PX(RD_F32, 2); }
#undef RD_PX
      return check_launch("nchw_to_nhwc");
    }
  }
  if (dst_dtype == RD_BF16)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<RD_BF16>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, dst_cstride, dst_coff, zero_pad, total);
  else if (dst_dtype == RD_F16)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<RD_F16>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, dst_cstride, dst_coff, zero_pad, total);
  else if (dst_dtype == RD_F32)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<RD_F32>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, dst_cstride, dst_coff, zero_pad, total);
  else
    return rd::fail(RD_EINVAL, "nchw_to_nhwc: dtype %d", dst_dtype);
  return check_launch("nchw_to_nhwc");
}
int rd_copy_rows(const void* src, long src_row_bytes, void* dst, long dst_row_bytes, long dst_offset_bytes, long bytes,
                 int rows, void* stream) {
  RD_REQUIRE(src && dst, RD_EINVAL, "copy_rows: null pointer");
  RD_REQUIRE(rows > 0 && bytes > 0 && src_row_bytes >= bytes && dst_row_bytes >= dst_offset_bytes + bytes && dst_offset_bytes >= 0,
             RD_ESHAPE, "copy_rows: bad geometry");
  ProfScope ps(RD_PROF_LAYOUT, (hipStream_t)stream);
  if (hipMemcpy2DAsync((char*)dst + dst_offset_bytes, (size_t)dst_row_bytes, src, (size_t)src_row_bytes, (size_t)bytes,
                       (size_t)rows, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return rd::fail(RD_EHIP, "copy_rows: hipMemcpy2DAsync failed");
  return RD_OK;
}
int rd_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int src_cstride, int src_coff,
                    int src_dtype, void* stream) {
  RD_REQUIRE(src && dst, RD_EINVAL, "nhwc_to_nchw: null pointer");
  RD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, RD_ESHAPE, "nhwc_to_nchw: bad shape");
  RD_REQUIRE(src_coff >= 0 && src_coff + C <= src_cstride, RD_ESHAPE, "nhwc_to_nchw: channels exceed stride");
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W, total = (long)B * C * HW;
  const int grid = (int)std::min<long>((total + 255) / 256, 8192);
  ProfScope ps(RD_PROF_LAYOUT, st);
  if (src_dtype == RD_BF16)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<RD_BF16>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, src_cstride, src_coff, total);
  else if (src_dtype == RD_F16)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<RD_F16>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, src_cstride, src_coff, total);
  else if (src_dtype == RD_F32)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<RD_F32>, dim3(grid), dim3(256), 0, st, src, dst, C, HW, src_cstride, src_coff, total);
  else
    return rd::fail(RD_EINVAL, "nhwc_to_nchw: dtype %d", src_dtype);
  return check_launch("nhwc_to_nchw");
}

// ---- packing (host) -------------------------------------------------------------------------------------
size_t rd_conv_packed_bytes(int ntaps, int cin, int cout, int dtype) { return conv_packed_bytes(ntaps, cin, cout, dtype); }
int rd_pack_conv_weight_host(const float* w, int cout, int cin, int kh, int kw, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv: null pointer");
  RD_REQUIRE(dtype == RD_F32 || is_h16(dtype), RD_EINVAL, "pack_conv: dtype");
  RD_REQUIRE(kh * kw >= 1 && kh * kw <= 9 && (kh & 1) && (kw & 1), RD_ESHAPE, "pack_conv: kernel (%d,%d)", kh, kw);
  TapList tl = conv_taps(kh, kw);
  auto get = [&](int co, int ci, int t) { return w[(((size_t)co * cin + ci) * kh + tl.kh[t]) * kw + tl.kw[t]]; };
  memset(out, 0, conv_packed_bytes(tl.n, cin, cout, dtype));     // padding of partial chunks and the zero tail
  if (is_h16(dtype)) pack_taps_frag(tl.n, cin, cout, out, get, dtype);
  else pack_taps(tl.n, cin, cout, dtype, out, get);
  return RD_OK;
}
// A phase whose taps all lie inside the 3x3 window (every transposed conv of the RangeDet graph) is packed and run as a
// tap list in (dh, dw) order; the persistent 3x3 kernel then serves it, writing the phase's pixels of the output viewed
// as [H][Win][stride_w * Cstride].  Tap set 1 / 2: exactly the six taps with dh in {-1,0,1} and dw in {-1,0} / {0,+1}
// (what k(3,8) s4 p2 and k(3,4) s2 p1 phases are) -> 6-step units; anything else inside the window is embedded in
// all nine taps with zero weights.
static bool deconv_embeds_3x3(const TapList& tl) {
  for (int t = 0; t < tl.n; ++t)
    if (tl.dh[t] < -1 || tl.dh[t] > 1 || tl.dw[t] < -1 || tl.dw[t] > 1) return false;
  return tl.n >= 1 && tl.n <= 9;
}
static int deconv_tap_set(const TapList& tl) {   // 1 / 2 as above, else 0
  if (tl.n != 6 || !deconv_embeds_3x3(tl)) return 0;
  for (int ts = 1; ts <= 2; ++ts) {
    bool seen[6] = {false, false, false, false, false, false};
    bool ok = true;
    for (int t = 0; t < 6 && ok; ++t) {
      const int c = tl.dw[t] - (ts == 1 ? -1 : 0);
      if (c < 0 || c > 1) ok = false;
      else seen[(tl.dh[t] + 1) * 2 + c] = true;
    }
    for (int i = 0; i < 6 && ok; ++i) ok = seen[i];
    if (ok) return ts;
  }
  return 0;
}
// the phase's taps in ascending (dh, dw) order: the order the packed image and every kernel use
static TapList deconv_taps_sorted(int kh, int kw, int s, int pad_w, int phase) {
  TapList tl = deconv_taps(kh, kw, s, pad_w, phase);
  if (tl.n > 9) return tl;
  for (int i = 1; i < tl.n; ++i)
    for (int j = i; j > 0 && (tl.dh[j] < tl.dh[j - 1] || (tl.dh[j] == tl.dh[j - 1] && tl.dw[j] < tl.dw[j - 1])); --j) {
      std::swap(tl.dh[j], tl.dh[j - 1]); std::swap(tl.dw[j], tl.dw[j - 1]);
      std::swap(tl.kh[j], tl.kh[j - 1]); std::swap(tl.kw[j], tl.kw[j - 1]);
    }
  return tl;
}
int rd_deconv_phase_taps(int kh, int kw, int stride_w, int pad_w, int phase) {
  if (stride_w < 1 || phase < 0 || phase >= stride_w) return RD_EINVAL;
  TapList tl = deconv_taps(kh, kw, stride_w, pad_w, phase);
  if (tl.n > 9) return RD_ESHAPE;
  return (deconv_embeds_3x3(tl) && !deconv_tap_set(tl)) ? 9 : tl.n;
}
int rd_pack_deconv_weight_host(const float* w, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                               int phase, int dtype, void* out) {
  return rd_pack_deconv_weight_folded_host(w, nullptr, cin, cout, kh, kw, stride_w, pad_w, phase, dtype, out);
}
int rd_pack_deconv_weight_folded_host(const float* w, const float* fold_scale, int cin, int cout, int kh, int kw, int stride_w,
                                      int pad_w, int phase, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_deconv: null pointer");
  RD_REQUIRE(dtype == RD_F32 || is_h16(dtype), RD_EINVAL, "pack_deconv: dtype");
  RD_REQUIRE(stride_w >= 1 && phase >= 0 && phase < stride_w, RD_EINVAL, "pack_deconv: phase");
  TapList tl = deconv_taps_sorted(kh, kw, stride_w, pad_w, phase);
  RD_REQUIRE(tl.n >= 1 && tl.n <= 9, RD_ESHAPE, "pack_deconv: %d taps", tl.n);
  const bool emb = deconv_embeds_3x3(tl) && !deconv_tap_set(tl);
  auto get = [&](int co, int ci, int t) -> float {
    if (emb) {  // t indexes the 3x3 window (dh, dw) = (t/3 - 1, t%3 - 1): the phase's tap there, or zero
      int src = -1;
      for (int u = 0; u < tl.n; ++u)
        if (tl.dh[u] == t / 3 - 1 && tl.dw[u] == t % 3 - 1) src = u;
      if (src < 0) return 0.f;
      t = src;
    }
    return (fold_scale ? fold_scale[co] : 1.f) * w[(((size_t)ci * cout + co) * kh + tl.kh[t]) * kw + tl.kw[t]];
  };
  const int nt = emb ? 9 : tl.n;
  memset(out, 0, conv_packed_bytes(nt, cin, cout, dtype));
  if (is_h16(dtype)) pack_taps_frag(nt, cin, cout, out, get, dtype);
  else pack_taps(nt, cin, cout, dtype, out, get);
  return RD_OK;
}

// ---- conv family ------------------------------------------------------------------------------------------
int rd_conv2d_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale,
                     const float* shift, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                     int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int flags,
                     int dtype, void* stream) {
  RD_REQUIRE(x && w_packed && y, RD_EINVAL, "conv2d: null pointer");
  RD_REQUIRE((kh == 1 && kw == 1) || (kh == 3 && kw == 3), RD_ESHAPE, "conv2d: kernel (%d,%d) not in {1x1,3x3}", kh, kw);
  RD_REQUIRE(stride_w == 1 || stride_w == 2, RD_ESHAPE, "conv2d: stride_w %d", stride_w);
  RD_REQUIRE(y_coff >= 0 && y_coff + cout <= y_cstride, RD_ESHAPE, "conv2d: y channels exceed stride");
  const int pad = (kw - 1) / 2;
  const int Wout = (Win + 2 * pad - kw) / stride_w + 1;  // mx Convolution output size
  RD_REQUIRE(!(flags & RD_SCALE_FOLDED), RD_EINVAL, "conv2d: RD_SCALE_FOLDED is taken by rd_conv3x3_bn_act_ex / rd_conv2d_bn_act_head_out / rd_deconv2d_bn_act");
  TapList tl = conv_taps(kh, kw);
  allow_conv_lds();
  return launch_conv(tl, x, x_cstride, x_coff, w_packed, scale, shift, residual, r_cstride, r_coff, y, y_cstride,
                     y_coff, B, H, Win, Wout, Wout, cin, cout, stride_w, 1, 0, flags, dtype, (hipStream_t)stream);
}
// ---- 3x3 conv of a BasicBlock, extended forms (bf16, persistent kernel) -----------------------------------------------------
// stride (1,2) on the pixel-pair view: x [H][W][cs] with W even IS [H][W/2][2*cs] -- channels [0, cs) of view pixel w2 are
// pixel 2*w2, channels [cs, 2cs) pixel 2*w2+1 -- and  out[w2] = sum_dh ( W[dh,-1].odd[w2-1] + W[dh,0].even[w2] + W[dh,+1].odd[w2] )
// is a stride-1 conv over the view with the six taps dw2 in {-1, 0} (tap set 1): two thirds of the multiply-adds of the
// stride-1-then-drop form and only the stored pixels are computed.
static int ex_view_cin(int cin, int x_cstride, int stride_w) { return stride_w == 2 ? x_cstride + cin : cin; }
size_t rd_conv3x3_ex_packed_bytes(int cin, int cout, int stride_w, int x_cstride) {
  return conv_packed_bytes(stride_w == 2 ? 6 : 9, ex_view_cin(cin, x_cstride, stride_w), cout, RD_BF16);
}
int rd_pack_conv3x3_ex_host(const float* w, const float* fold_scale, int cout, int cin, int stride_w, int x_cstride, int dtype,
                            void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv3x3_ex: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv3x3_ex: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(stride_w == 1 || stride_w == 2, RD_ESHAPE, "pack_conv3x3_ex: stride_w %d", stride_w);
  RD_REQUIRE(cout == 64 || cout == 128, RD_ESHAPE, "pack_conv3x3_ex: cout %d", cout);
  RD_REQUIRE(stride_w == 1 || (x_cstride >= cin && x_cstride % 8 == 0), RD_ESHAPE, "pack_conv3x3_ex: x_cstride %d for cin %d", x_cstride, cin);
  auto wv = [&](int co, int ci, int dh, int dw) {
    return (fold_scale ? fold_scale[co] : 1.f) * w[(((size_t)co * cin + ci) * 3 + (dh + 1)) * 3 + (dw + 1)];
  };
  memset(out, 0, rd_conv3x3_ex_packed_bytes(cin, cout, stride_w, x_cstride));
  // pair view (stride 2): channel c2 < cin is the even pixel (only dw2 = 0 meets it), c2 >= x_cstride the odd one (dw = -1 / +1)
  auto wv2 = [&](int co, int c2, int dh, int dw2) -> float {
    if (c2 < cin) return dw2 == 0 ? wv(co, c2, dh, 0) : 0.f;
    if (c2 >= x_cstride && c2 - x_cstride < cin) return wv(co, c2 - x_cstride, dh, dw2 == -1 ? -1 : 1);
    return 0.f;
  };
  if (stride_w == 1) {
    if (conv3_body_small(cin, fold_scale != nullptr))   // <= 16 input channels: five two-tap steps instead of nine (k_conv3.h c3_body 3)
      pack_body_frag(3, cin, cout, out, [&](int co, int ci, int dh, int dw) { return wv(co, ci, dh - 1, dw - 1); }, dtype);
    else
      pack_taps_frag(9, cin, cout, out, [&](int co, int ci, int t) { return wv(co, ci, t / 3 - 1, t % 3 - 1); }, dtype);
  } else if (conv3_body_s2(cin, x_cstride, fold_scale != nullptr)) {
    // the even pixel's chunks as 3-tap units (no MFMAs on their structurally-zero dw2 = -1 weights): k_conv3.h c3_body 1
    pack_body_frag(1, x_cstride + cin, cout, out, [&](int co, int c2, int dh, int dw) { return wv2(co, c2, dh - 1, dw - 1); }, dtype);
  } else {
    pack_taps_frag(6, x_cstride + cin, cout, out, [&](int co, int c2, int s) -> float { return wv2(co, c2, s / 2 - 1, s % 2 - 1); }, dtype);
  }
  return RD_OK;
}
// the same conv for RD_MFMA16 launches (k_conv3.h M16: v_mfma_f32_16x16x32 fragments): stride 1, cout 128, cin a multiple of 32
int rd_pack_conv3x3_m16_host(const float* w, const float* fold_scale, int cout, int cin, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv3x3_m16: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv3x3_m16: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(cout == 128 && cin >= 32 && cin % 32 == 0, RD_ESHAPE, "pack_conv3x3_m16: cout %d (128), cin %d (a multiple of 32)", cout, cin);
  memset(out, 0, rd_conv3x3_ex_packed_bytes(cin, cout, 1, cin));
  pack_taps_frag16(9, cin, cout, out, [&](int co, int ci, int t) {
    return (fold_scale ? fold_scale[co] : 1.f) * w[(((size_t)co * cin + ci) * 3 + t / 3) * 3 + t % 3];
  }, dtype);
  return RD_OK;
}
int rd_conv3x3_mfma16_ok(int cin, int cout, int stride_w, int W, int fused_output_conv) {
  (void)W; (void)fused_output_conv;   // (the form exists at every width, with or without a fused output conv)
  return conv3_mfma16_ok(cin, cout, stride_w) ? 1 : 0;
}
size_t rd_conv1x1_sc_packed_bytes(int cin, int cout) { return sc_frag_bytes(cin, cout); }
int rd_pack_conv1x1_sc_host(const float* w, const float* fold_scale, int cout, int cin, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv1x1_sc: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv1x1_sc: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE((cout == 64 || cout == 128) && cin >= 1 && cin <= 128, RD_ESHAPE, "pack_conv1x1_sc: cout %d, cin %d (1..128)", cout, cin);
  pack_sc_frag(w, fold_scale, cin, cout, out, dtype);
  return RD_OK;
}
int rd_conv3x3_bn_act_ex(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale, const float* shift,
                         const void* residual, int r_cstride, int r_coff, const void* sc_x, int sc_cstride, int sc_coff,
                         int sc_cin, const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int Win, int cin,
                         int cout, int stride_w, int flags, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed && y, RD_EINVAL, "conv3x3_ex: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv3x3_ex: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(B > 0 && H > 0 && Win > 0 && cin > 0 && (cout == 64 || cout == 128), RD_ESHAPE, "conv3x3_ex: shape / cout %d", cout);
  RD_REQUIRE(stride_w == 1 || (stride_w == 2 && Win % 2 == 0), RD_ESHAPE, "conv3x3_ex: stride_w %d with Win %d (stride 2 needs an even width)", stride_w, Win);
  RD_REQUIRE(y_coff >= 0 && y_coff + cout <= y_cstride, RD_ESHAPE, "conv3x3_ex: y channels exceed stride");
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff + cin_slots(cin, RD_BF16) * 8 <= x_cstride, RD_ESHAPE, "conv3x3_ex: x channel stride/offset");
  RD_REQUIRE(!(sc_x && residual) && !(sc_x && !sc_w_packed), RD_EINVAL, "conv3x3_ex: shortcut conv and residual are exclusive");
  RD_REQUIRE(!((flags & RD_ADD) && !residual && !sc_x), RD_EINVAL, "conv3x3_ex: RD_ADD without residual / shortcut");
  allow_conv_lds();
  const int v = stride_w;                      // pixels per view pixel
  const int Wv = Win / v;
  Conv3Args e;
  memset(&e, 0, sizeof(e));
  int fl = flags;
  if (sc_x) {
    RD_REQUIRE(sc_cin >= 1 && sc_cin <= 128 && sc_cstride % 8 == 0 && sc_coff % 8 == 0 && sc_coff + ((sc_cin + 15) / 16) * 16 <= sc_cstride,
               RD_ESHAPE, "conv3x3_ex: shortcut input channels %d (stride %d, offset %d)", sc_cin, sc_cstride, sc_coff);
    // the shortcut reads the block input at the OUTPUT pixel grid: stride 2 = the even pixel of each pair of the view
    e.sx = (const bf16_t*)sc_x; e.s_cs = sc_cstride * v; e.s_co = sc_coff; e.s_bs = (long)H * Wv * sc_cstride * v;
    e.scw = (const unsigned char*)sc_w_packed; e.s_nks = (sc_cin + 15) / 16;
    fl &= ~RD_ADD;                             // the add happens on the accumulators
    fl |= RD_SCALE_FOLDED;                     // (both scales are in the two weight sets)
  }
  RD_REQUIRE(!(fl & RD_SCALE_FOLDED) || !scale, RD_EINVAL, "conv3x3_ex: folded weights take no scale array");
  const bool m16 = (fl & RD_MFMA16) != 0;
  fl &= ~RD_MFMA16;
  const bool folded = (fl & RD_SCALE_FOLDED) != 0;
  RD_REQUIRE(!m16 || (folded && !sc_x && conv3_mfma16_ok(cin, cout, stride_w)), RD_ESHAPE,
             "conv3x3_ex: RD_MFMA16 takes folded weights of rd_pack_conv3x3_m16_host: stride 1, cout 128, cin a multiple of 32, no fused shortcut (rd_conv3x3_mfma16_ok)");
  const int body = m16 ? C3_BODY_M16 : stride_w == 2 ? conv3_body_s2(cin, x_cstride, folded) : (sc_x ? 0 : conv3_body_small(cin, folded));
  RD_REQUIRE(!(stride_w == 1 && sc_x && conv3_body_small(cin, folded)), RD_ESHAPE, "conv3x3_ex: at most 16 input channels together with a fused shortcut is not a launch form");
  return launch_conv3(x, x_cstride * v, x_coff, w_packed, scale, shift, residual, r_cstride, r_coff, y, y_cstride, y_coff, B, H,
                      Wv, ex_view_cin(cin, x_cstride, stride_w), cout, fl, 1, (hipStream_t)stream, stride_w == 2 ? 1 : 0,
                      sc_x ? &e : nullptr, dtype, nullptr, nullptr, body);
}

// ---- a whole 64-channel BasicBlock in one launch (k_block.h) ------------------------------------------------------------------------
size_t rd_block64_packed_bytes(int cin) { return block64_packed_bytes(cin); }
int rd_pack_block64_host(const float* w1, const float* fold_scale1, const float* w2, const float* fold_scale2, int cin, int dtype, void* out) {
  RD_REQUIRE(w1 && w2 && out, RD_EINVAL, "pack_block64: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_block64: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(cin == 64 || (cin >= 1 && cin <= 16), RD_ESHAPE, "pack_block64: %d input channels (64, or at most 16)", cin);
  pack_block64(w1, fold_scale1, w2, fold_scale2, cin, dtype, out);
  return RD_OK;
}
int rd_block64_bn_act(const void* x, int x_cstride, int x_coff, int cin, const void* w_packed, const float* shift1, const float* shift2,
                      const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed && shift1 && shift2 && y, RD_EINVAL, "block64: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "block64: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(B > 0 && H > 0 && W > 0, RD_ESHAPE, "block64: shape");
  RD_REQUIRE(cin == 64 || (cin >= 1 && cin <= 16), RD_ESHAPE, "block64: %d input channels (64, or at most 16 for the network's first block)", cin);
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff >= 0 && x_coff + cin_slots(cin, RD_BF16) * 8 <= x_cstride, RD_ESHAPE, "block64: x channel stride / offset");
  // (the first block's shortcut epilogue loads a whole 16-channel k-slot of x per pixel -- cin_slots() rounds cin <= 16 up to
  //  exactly that, so an 8-channel pitch is refused above; said once more explicitly so that it survives a change of cin_slots)
  RD_REQUIRE(cin > 16 || x_coff + 16 <= x_cstride, RD_ESHAPE, "block64: the first block reads 16 channels per pixel (x_coff %d + 16 > x_cstride %d)", x_coff, x_cstride);
  RD_REQUIRE(y_cstride % 8 == 0 && y_coff % 8 == 0 && y_coff >= 0 && y_coff + 64 <= y_cstride, RD_ESHAPE, "block64: y channel stride / offset");
  RD_REQUIRE(x != y, RD_EINVAL, "block64: in-place (a tile's halo is another tile's output)");
  return launch_block64(x, x_cstride, x_coff, cin, w_packed, shift1, shift2, sc_w_packed, y, y_cstride, y_coff, B, H, W, dtype, (hipStream_t)stream);
}

// ... in the 16 x 16 x 32 MFMA form (k_block.h M16; 64 input channels): its own weight images, the same results
int rd_pack_block64_m16_host(const float* w1, const float* fold_scale1, const float* w2, const float* fold_scale2, int dtype, void* out) {
  RD_REQUIRE(w1 && w2 && out, RD_EINVAL, "pack_block64_m16: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_block64_m16: dtype %d (RD_BF16 or RD_F16)", dtype);
  pack_block64_m16(w1, fold_scale1, w2, fold_scale2, dtype, out);
  return RD_OK;
}
int rd_pack_conv1x1_sc_m16_host(const float* w, const float* fold_scale, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv1x1_sc_m16: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv1x1_sc_m16: dtype %d (RD_BF16 or RD_F16)", dtype);
  pack_sc_frag16(w, fold_scale, out, dtype);
  return RD_OK;
}
int rd_block64_m16_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* shift1, const float* shift2,
                          const void* sc_w_packed, void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed && shift1 && shift2 && y, RD_EINVAL, "block64_m16: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "block64_m16: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(B > 0 && H > 0 && W > 0, RD_ESHAPE, "block64_m16: shape");
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff >= 0 && x_coff + 64 <= x_cstride, RD_ESHAPE, "block64_m16: x channel stride / offset");
  RD_REQUIRE(y_cstride % 8 == 0 && y_coff % 8 == 0 && y_coff >= 0 && y_coff + 64 <= y_cstride, RD_ESHAPE, "block64_m16: y channel stride / offset");
  RD_REQUIRE(x != y, RD_EINVAL, "block64_m16: in-place (a tile's halo is another tile's output)");
  return launch_block64(x, x_cstride, x_coff, 64, w_packed, shift1, shift2, sc_w_packed, y, y_cstride, y_coff, B, H, W, dtype, (hipStream_t)stream, true);
}

// ---- 3x3 conv over the channel concatenation [x1 | x2] of two tensors that is never materialised (16-bit, folded scales) -----------
// dla_backbone.py:153-154 (concat of the range image with the agg3 feature map) feeding head/builder.py:221-240: w_packed is
// rd_pack_conv3x3_cat_host of the weight whose input channels are laid out [cin1 channels of x1 | cin2 channels of x2].
size_t rd_conv3x3_cat_packed_bytes(int cin1, int cin2, int cout) { return conv_packed_bytes(9, cin1 + cin2, cout, RD_BF16); }
int rd_pack_conv3x3_cat_host(const float* w, const float* fold_scale, int cout, int cin1, int cin2, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_conv3x3_cat: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv3x3_cat: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE((cout == 64 || cout == 128) && cin1 > 0 && cin1 % 32 == 0 && cin2 > 0 && cin2 % 8 == 0, RD_ESHAPE,
             "pack_conv3x3_cat: cout %d, cin1 %d (multiple of 32), cin2 %d (multiple of 8)", cout, cin1, cin2);
  const int cin = cin1 + cin2;
  auto wv = [&](int co, int ci, int dh, int dw) {
    return (fold_scale ? fold_scale[co] : 1.f) * w[(((size_t)co * cin + ci) * 3 + (dh + 1)) * 3 + (dw + 1)];
  };
  memset(out, 0, rd_conv3x3_cat_packed_bytes(cin1, cin2, cout));
  const int body = conv3_body_cat(cin1, cin2, fold_scale != nullptr);
  if (body) pack_body_frag(body, cin, cout, out, [&](int co, int ci, int dh, int dw) { return wv(co, ci, dh - 1, dw - 1); }, dtype);
  else pack_taps_frag(9, cin, cout, out, [&](int co, int ci, int t) { return wv(co, ci, t / 3 - 1, t % 3 - 1); }, dtype);
  return RD_OK;
}
int rd_conv3x3_bn_act_cat(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                          const void* w_packed, const float* shift, void* y, int y_cstride, int y_coff, int B, int H, int W, int cout,
                          int flags, int dtype, void* stream) {
  RD_REQUIRE(x1 && x2 && w_packed && y && shift, RD_EINVAL, "conv3x3_cat: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv3x3_cat: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE((flags & RD_SCALE_FOLDED) && !(flags & RD_ADD), RD_EINVAL, "conv3x3_cat: needs RD_SCALE_FOLDED weights, takes no residual");
  RD_REQUIRE(B > 0 && H > 0 && W > 0 && (cout == 64 || cout == 128), RD_ESHAPE, "conv3x3_cat: shape / cout %d", cout);
  RD_REQUIRE(cin1 > 0 && cin1 % 32 == 0 && cin2 > 0 && cin2 % 8 == 0, RD_ESHAPE, "conv3x3_cat: cin1 %d (multiple of 32), cin2 %d (multiple of 8)", cin1, cin2);
  RD_REQUIRE(y_coff >= 0 && y_coff + cout <= y_cstride, RD_ESHAPE, "conv3x3_cat: y channels exceed stride");
  RD_REQUIRE(x1_cstride % 8 == 0 && x1_coff % 8 == 0 && x1_coff + cin1 <= x1_cstride && x2_cstride % 8 == 0 && x2_coff % 8 == 0 &&
             x2_coff + cin2 <= x2_cstride, RD_ESHAPE, "conv3x3_cat: channel stride/offset");
  allow_conv_lds();
  Conv3Src2 s2;
  s2.x = x2; s2.cs = x2_cstride; s2.co = x2_coff; s2.cin1 = cin1; s2.cin2 = cin2;
  return launch_conv3(x1, x1_cstride, x1_coff, w_packed, nullptr, shift, nullptr, 0, 0, y, y_cstride, y_coff, B, H, W, cin1 + cin2, cout, flags,
                      1, (hipStream_t)stream, 0, nullptr, dtype, nullptr, &s2, conv3_body_cat(cin1, cin2, true));
}

// ---- last tower conv + the tower's 1x1 output conv in one launch (bf16) ---------------------------------------------
size_t rd_head_packed_bytes(void) { return 16384; }
int rd_pack_head_weight_host(const float* w, int nout, int cin, int dtype, void* out_host) {
  RD_REQUIRE(w && out_host, RD_EINVAL, "pack_head_weight: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_head_weight: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(nout >= 1 && nout <= 8 && cin >= 1 && cin <= 128, RD_ESHAPE, "pack_head_weight: nout %d (1..8), cin %d (1..128)", nout, cin);
  pack_head_frag(w, nout, cin, out_host, dtype);
  return RD_OK;
}
// ... for RD_MFMA16 launches (k_conv3.h pack_head_frag16): 8 KB
size_t rd_head_m16_packed_bytes(void) { return 8192; }
int rd_pack_head_weight_m16_host(const float* w, int nout, int cin, int dtype, void* out_host) {
  RD_REQUIRE(w && out_host, RD_EINVAL, "pack_head_weight_m16: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_head_weight_m16: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(nout >= 1 && nout <= 8 && cin >= 1 && cin <= 128, RD_ESHAPE, "pack_head_weight_m16: nout %d (1..8), cin %d (1..128)", nout, cin);
  pack_head_frag16(w, nout, cin, out_host, dtype);
  return RD_OK;
}
int rd_conv2d_bn_act_head_out(const void* x, int x_cstride, int x_coff, const void* w_packed, const float* scale,
                              const float* shift, int B, int H, int W, int cin, int flags, const void* head_w_packed,
                              const float* head_bias, float* out, long out_batch_stride, long n_off, int nout, int dtype,
                              void* stream) {
  RD_REQUIRE(x && w_packed && head_w_packed && head_bias && out, RD_EINVAL, "conv2d_head_out: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv2d_head_out: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(B > 0 && H > 0 && W > 0 && cin > 0 && nout >= 1 && nout <= 8, RD_ESHAPE, "conv2d_head_out: shape / nout %d (1..8)", nout);
  RD_REQUIRE(!(flags & RD_ADD), RD_EINVAL, "conv2d_head_out: no residual in a head tower");
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff + cin_slots(cin, RD_BF16) * 8 <= x_cstride, RD_ESHAPE,
             "conv2d_head_out: x channel stride/offset");
  RD_REQUIRE(!conv3_body_small(cin, (flags & RD_SCALE_FOLDED) != 0), RD_ESHAPE, "conv2d_head_out: cin %d (the packed image of a conv with <= 16 input channels is not this launch form's)", cin);
  const bool m16 = (flags & RD_MFMA16) != 0;
  RD_REQUIRE(!m16 || ((flags & RD_SCALE_FOLDED) && conv3_mfma16_ok(cin, 128, 1)), RD_ESHAPE,
             "conv2d_head_out: RD_MFMA16 (weights of rd_pack_conv3x3_m16_host) is not a launch form for cin %d at width %d (rd_conv3x3_mfma16_ok)", cin, W);
  allow_conv_lds();
  Conv3Args h;
  memset(&h, 0, sizeof(h));
  h.hw = (const unsigned char*)head_w_packed; h.hb = head_bias; h.ho = out; h.ho_bs = out_batch_stride; h.ho_off = n_off; h.hn = nout;
  return launch_conv3(x, x_cstride, x_coff, w_packed, scale, shift, nullptr, 0, 0, nullptr, 128, 0, B, H, W, cin, 128, flags & ~RD_MFMA16, 1,
                      (hipStream_t)stream, 0, &h, dtype, nullptr, nullptr, m16 ? C3_BODY_M16 : 0);
}

int rd_deconv2d_bn_act(const void* x, int x_cstride, int x_coff, const void* w_packed_phase, const float* scale,
                       const float* shift, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                       int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                       int phase, int flags, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed_phase && y, RD_EINVAL, "deconv2d: null pointer");
  RD_REQUIRE(kh == 3, RD_ESHAPE, "deconv2d: kernel height %d (only 3, pad 1, stride 1)", kh);
  RD_REQUIRE(stride_w >= 1 && phase >= 0 && phase < stride_w, RD_EINVAL, "deconv2d: phase %d of stride %d", phase, stride_w);
  RD_REQUIRE(y_coff >= 0 && y_coff + cout <= y_cstride, RD_ESHAPE, "deconv2d: y channels exceed stride");
  const int Wout = (Win - 1) * stride_w - 2 * pad_w + kw;  // mx Deconvolution output size
  RD_REQUIRE(Wout > phase, RD_ESHAPE, "deconv2d: empty phase");
  const int Wq = (Wout - phase + stride_w - 1) / stride_w;
  TapList tl = deconv_taps_sorted(kh, kw, stride_w, pad_w, phase);
  RD_REQUIRE(tl.n >= 1 && tl.n <= 9, RD_ESHAPE, "deconv2d: %d taps per phase unsupported", tl.n);
  allow_conv_lds();
  if (deconv_embeds_3x3(tl)) {
    const int ts = deconv_tap_set(tl);
    if (!ts) tl = conv_taps(3, 3);   // packed as a full 3x3 window with zero weights (rd_pack_deconv_weight_host)
    if (is_h16(dtype) && Wout == stride_w * Win && (cout == 64 || cout == 128) &&
        conv3_has_form(dtype, (flags & RD_SCALE_FOLDED) != 0)) {
      // phase pixels of the output seen as [H][Win][stride_w * Cstride]: channel offset phase * Cstride
      const bf16_t* r = (const bf16_t*)residual;
      return launch_conv3(x, x_cstride, x_coff, w_packed_phase, scale, shift, r, r_cstride * stride_w,
                          r_coff + phase * r_cstride, y, y_cstride * stride_w, y_coff + phase * y_cstride, B, H, Win, cin,
                          cout, flags, 1, (hipStream_t)stream, ts, nullptr, dtype);
    }
  }
  RD_REQUIRE(!(flags & RD_SCALE_FOLDED), RD_ESHAPE, "deconv2d: RD_SCALE_FOLDED needs the persistent 3x3 kernel (bf16, cout 64/128, "
             "taps inside the 3x3 window, Wout == stride_w * Win)");
  return launch_conv(tl, x, x_cstride, x_coff, w_packed_phase, scale, shift, residual, r_cstride, r_coff, y,
                     y_cstride, y_coff, B, H, Win, Wq, Wout, cin, cout, 1, stride_w, phase, flags, dtype,
                     (hipStream_t)stream);
}

// ---- ALL phases of a transposed conv in ONE launch (16-bit, folded scales) -------------------------------------------------------
// w_packed_all = the stride_w phase images of rd_pack_deconv_weight_folded_host one after the other, w_phase_bytes apart.
int rd_deconv2d_all_phases_ok(int kh, int kw, int stride_w, int pad_w, int cout, int dtype) {
  if (!is_h16(dtype) || kh != 3 || stride_w < 2 || stride_w > 8 || !conv3_phases_eligible(cout, RD_SCALE_FOLDED)) return 0;
  if (kw - 2 * pad_w != stride_w) return 0;   // Wout = (Win - 1) * stride_w - 2 * pad_w + kw must equal stride_w * Win
  for (int p = 0; p < stride_w; ++p)
    if (!deconv_tap_set(deconv_taps_sorted(kh, kw, stride_w, pad_w, p))) return 0;
  return 1;
}
int rd_deconv2d_bn_act_all(const void* x, int x_cstride, int x_coff, const void* w_packed_all, long w_phase_bytes,
                           const float* shift, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                           int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                           int flags, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed_all && y, RD_EINVAL, "deconv2d_all: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "deconv2d_all: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(flags & RD_SCALE_FOLDED, RD_EINVAL, "deconv2d_all: needs RD_SCALE_FOLDED weights (rd_pack_deconv_weight_folded_host)");
  RD_REQUIRE(!((flags & RD_ADD) && !residual), RD_EINVAL, "deconv2d_all: RD_ADD without residual");
  RD_REQUIRE(B > 0 && H > 0 && Win > 0 && cin > 0, RD_ESHAPE, "deconv2d_all: shape");
  RD_REQUIRE(y_coff >= 0 && y_coff + cout <= y_cstride, RD_ESHAPE, "deconv2d_all: y channels exceed stride");
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff + cin_slots(cin, RD_BF16) * 8 <= x_cstride, RD_ESHAPE, "deconv2d_all: x channel stride/offset");
  RD_REQUIRE(rd_deconv2d_all_phases_ok(kh, kw, stride_w, pad_w, cout, dtype), RD_ESHAPE,
             "deconv2d_all: kernel (%d,%d) stride %d pad %d cout %d is not a set of two-column 3x2 phases (use rd_deconv2d_bn_act per phase)",
             kh, kw, stride_w, pad_w, cout);
  RD_REQUIRE(w_phase_bytes >= (long)conv_packed_bytes(6, cin, cout, RD_BF16) && w_phase_bytes % 16 == 0, RD_EINVAL, "deconv2d_all: w_phase_bytes");
  allow_conv_lds();
  Conv3Phases ph;
  ph.nph = stride_w; ph.ts_mask = 0; ph.y_pc = y_cstride; ph.r_pc = r_cstride; ph.w_pb = w_phase_bytes;
  for (int p = 0; p < stride_w; ++p)
    if (deconv_tap_set(deconv_taps_sorted(kh, kw, stride_w, pad_w, p)) == 2) ph.ts_mask |= 1 << p;
  return launch_conv3(x, x_cstride, x_coff, w_packed_all, nullptr, shift, residual, r_cstride * stride_w, r_coff, y, y_cstride * stride_w,
                      y_coff, B, H, Win, cin, cout, flags, 1, (hipStream_t)stream, 3, nullptr, dtype, &ph);
}

// ---- phase PAIRS of a transposed conv (cout 64, stride 4: dla_backbone.py:117-127 agg1) ----------------------------------------
// Output phases 2p and 2p+1 of a (3, 2*s) / stride s / pad s/2 transposed conv with s = 4 read the SAME two input columns (tap set 1
// for the pair 0 | 1, tap set 2 for 2 | 3), and in the output seen as [H][Win][s * C] their channels are neighbours: a pair is ONE
// 3 x 2-tap conv with 2 * cout = 128 output channels.  It runs the cout-128 form of the persistent kernel (every pixel fragment read
// from LDS feeds four MFMAs instead of two, half as many tile passes and epilogues) with bit-identical results: the K order of every
// output element is unchanged.  Needs a dense cout-channel output / residual (y_cstride == r_cstride == cout, offsets 0).
int rd_deconv2d_phase_pairs_ok(int kh, int kw, int stride_w, int pad_w, int cout, int dtype) {
  if (!rd_deconv2d_all_phases_ok(kh, kw, stride_w, pad_w, cout, dtype) || cout != 64 || stride_w % 2) return 0;
  if (!rd_deconv2d_all_phases_ok(kh, kw, stride_w, pad_w, 128, dtype)) return 0;    // (the cout-128 form of the kernel is available)
  for (int p = 0; p < stride_w; p += 2)
    if (deconv_tap_set(deconv_taps_sorted(kh, kw, stride_w, pad_w, p)) != deconv_tap_set(deconv_taps_sorted(kh, kw, stride_w, pad_w, p + 1))) return 0;
  return 1;
}
// pair image = the two phase images of rd_pack_deconv_weight_folded_host interleaved per (chunk, tap, k-step): [A: 2 KB | B: 2 KB]
int rd_pack_deconv_phase_pair_host(const void* phase_a, const void* phase_b, int cin, int dtype, void* out) {
  RD_REQUIRE(phase_a && phase_b && out, RD_EINVAL, "pack_deconv_pair: null pointer");
  RD_REQUIRE(is_h16(dtype) && cin > 0, RD_EINVAL, "pack_deconv_pair: dtype %d / cin %d", dtype, cin);
  const size_t body = conv_packed_body_bytes(6, cin, 64, RD_BF16), blocks = body / 2048;    // (chunk, tap, k-step) blocks of 2 x 1 KB
  for (size_t i = 0; i < blocks; ++i) {
    memcpy((unsigned char*)out + i * 4096, (const unsigned char*)phase_a + i * 2048, 2048);
    memcpy((unsigned char*)out + i * 4096 + 2048, (const unsigned char*)phase_b + i * 2048, 2048);
  }
  memset((unsigned char*)out + 2 * body, 0, 2 * RD_CONV_TAIL);    // the zero tail the kernel's padding DMA reads (k_conv.h RD_CONV_TAIL)
  return RD_OK;
}
// w_packed_pairs: stride_w / 2 pair images, w_pair_bytes apart; shift2: 2 * cout values (the layer's shift twice)
int rd_deconv2d_bn_act_pairs(const void* x, int x_cstride, int x_coff, const void* w_packed_pairs, long w_pair_bytes,
                             const float* shift2, const void* residual, int r_cstride, int r_coff, void* y, int y_cstride,
                             int y_coff, int B, int H, int Win, int cin, int cout, int kh, int kw, int stride_w, int pad_w,
                             int flags, int dtype, void* stream) {
  RD_REQUIRE(x && w_packed_pairs && y && shift2, RD_EINVAL, "deconv2d_pairs: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "deconv2d_pairs: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(flags & RD_SCALE_FOLDED, RD_EINVAL, "deconv2d_pairs: needs RD_SCALE_FOLDED weights (rd_pack_deconv_weight_folded_host)");
  RD_REQUIRE(!((flags & RD_ADD) && !residual), RD_EINVAL, "deconv2d_pairs: RD_ADD without residual");
  RD_REQUIRE(B > 0 && H > 0 && Win > 0 && cin > 0, RD_ESHAPE, "deconv2d_pairs: shape");
  RD_REQUIRE(x_cstride % 8 == 0 && x_coff % 8 == 0 && x_coff + cin_slots(cin, RD_BF16) * 8 <= x_cstride, RD_ESHAPE, "deconv2d_pairs: x channel stride/offset");
  RD_REQUIRE(rd_deconv2d_phase_pairs_ok(kh, kw, stride_w, pad_w, cout, dtype), RD_ESHAPE,
             "deconv2d_pairs: kernel (%d,%d) stride %d pad %d cout %d has no phase pairs (use rd_deconv2d_bn_act_all)", kh, kw, stride_w, pad_w, cout);
  RD_REQUIRE(y_cstride == cout && y_coff == 0 && (!residual || (r_cstride == cout && r_coff == 0)), RD_ESHAPE,
             "deconv2d_pairs: the output / residual must be dense %d-channel tensors (two phases are one 128-channel write)", cout);
  RD_REQUIRE(w_pair_bytes >= (long)conv_packed_bytes(6, cin, 2 * cout, RD_BF16) && w_pair_bytes % 16 == 0, RD_EINVAL, "deconv2d_pairs: w_pair_bytes");
  allow_conv_lds();
  Conv3Phases ph;
  ph.nph = stride_w / 2; ph.ts_mask = 0; ph.y_pc = 2 * cout; ph.r_pc = 2 * cout; ph.w_pb = w_pair_bytes;
  for (int p = 0; p < stride_w; p += 2)
    if (deconv_tap_set(deconv_taps_sorted(kh, kw, stride_w, pad_w, p)) == 2) ph.ts_mask |= 1 << (p / 2);
  return launch_conv3(x, x_cstride, x_coff, w_packed_pairs, nullptr, shift2, residual, r_cstride * stride_w, r_coff, y, y_cstride * stride_w,
                      y_coff, B, H, Win, cin, 2 * cout, flags, 1, (hipStream_t)stream, 3, nullptr, dtype, &ph);
}

int rd_head_out(const void* x, int x_cstride, int x_coff, const float* w, const float* bias, float* out,
                long out_batch_stride, long n_off, int B, int H, int W, int cin, int nout, int dtype, void* stream) {
  RD_REQUIRE(x && w && bias && out, RD_EINVAL, "head_out: null pointer");
  RD_REQUIRE(cin % 8 == 0 && cin <= 128 && cin > 0, RD_ESHAPE, "head_out: cin %d (multiple of 8, <= 128)", cin);
  RD_REQUIRE(nout == 1 || nout == 7 || nout == 8, RD_ESHAPE, "head_out: nout %d not in {1,7,8}", nout);
  RD_REQUIRE(dtype == RD_F32 || is_h16(dtype), RD_EINVAL, "head_out: dtype");
  hipStream_t st = (hipStream_t)stream;
  const long HW = (long)H * W;
  dim3 grid((unsigned)std::min<long>((HW + 31) / 32, 4096), B);
  ProfScope ps(RD_PROF_HEAD_OUT, st);
  if (is_h16(dtype) && nout > 1 && cin % 16 == 0 && x_cstride % 8 == 0 && x_coff % 8 == 0) {   // matrix-core streaming variant
    dim3 g2((unsigned)std::min<long>((HW + 127) / 128, 2048), B);
#define RD_HOM(NO, DT_) hipLaunchKernelGGL((head_out_mfma_kernel<NO, DT_>), g2, dim3(256), 0, st, (const bf16_t*)x, x_cstride, x_coff, w, bias, out, out_batch_stride, n_off, HW, cin)
    if (dtype == RD_F16) { if (nout == 7) RD_HOM(7, RD_F16); else RD_HOM(8, RD_F16); }
    else { if (nout == 7) RD_HOM(7, RD_BF16); else RD_HOM(8, RD_BF16); }
#undef RD_HOM
    return check_launch("head_out");
  }
#define RD_HO(DT, NO) hipLaunchKernelGGL((head_out_kernel<DT, NO>), grid, dim3(256), 0, st, x, x_cstride, x_coff, w, bias, out, out_batch_stride, n_off, HW, cin)
  if (dtype == RD_BF16) { if (nout == 1) RD_HO(RD_BF16, 1); else if (nout == 7) RD_HO(RD_BF16, 7); else RD_HO(RD_BF16, 8); }
  else if (dtype == RD_F16) { if (nout == 1) RD_HO(RD_F16, 1); else if (nout == 7) RD_HO(RD_F16, 7); else RD_HO(RD_F16, 8); }
  else { if (nout == 1) RD_HO(RD_F32, 1); else if (nout == 7) RD_HO(RD_F32, 7); else RD_HO(RD_F32, 8); }
#undef RD_HO
  return check_launch("head_out");
}

// ---- Meta-Kernel ---------------------------------------------------------------------------------------------
size_t rd_meta_packed_bytes(int dtype) { return meta_layout(dtype).total; }
int rd_pack_meta_host(const float* w0, const float* b0, const float* w1, const float* b1, const float* s1,
                      const float* t1, const float* agg, const float* s2, const float* t2, int dtype, void* out) {
  RD_REQUIRE(w0 && b0 && w1 && b1 && s1 && t1 && agg && s2 && t2 && out, RD_EINVAL, "pack_meta: null pointer");
  RD_REQUIRE(dtype == RD_F32 || is_h16(dtype), RD_EINVAL, "pack_meta: dtype");
  pack_meta(w0, b0, w1, b1, s1, t1, agg, s2, t2, dtype, out);
  return RD_OK;
}
int rd_meta_kernel_fwd(const void* data, int d_cstride, int d_coff, const float* coord_nchw, const void* packed,
                       void* y, int y_cstride, int y_coff, int B, int H, int W, int dtype, void* stream) {
  RD_REQUIRE(data && coord_nchw && packed && y, RD_EINVAL, "meta_kernel: null pointer");
  RD_REQUIRE(B > 0 && H > 0 && W > 0, RD_ESHAPE, "meta_kernel: empty shape");
  RD_REQUIRE(dtype == RD_F32 || is_h16(dtype), RD_EINVAL, "meta_kernel: dtype");
  const int ch = ch_per_slot(dtype);
  RD_REQUIRE(d_cstride % ch == 0 && d_coff % ch == 0 && y_cstride % ch == 0 && y_coff % ch == 0, RD_ESHAPE,
             "meta_kernel: channel strides/offsets must be 16-byte multiples");
  RD_REQUIRE(d_coff + 64 <= d_cstride && y_coff + 64 <= y_cstride, RD_ESHAPE, "meta_kernel: needs 64 channels");
  return launch_meta(data, d_cstride, d_coff, coord_nchw, packed, y, y_cstride, y_coff, B, H, W, dtype, (hipStream_t)stream);
}

// ---- post-processing -------------------------------------------------------------------------------------------
size_t rd_sorted_foreground_workspace_bytes(long N, long k) { (void)k; return (sort_ws_bytes(N) + 256 + 255) & ~(size_t)255; }
int rd_sorted_foreground(const float* cls_score, const float* bbox_delta, const float* pc, const float* mask, int B,
                         long N, long k, int D, int apply_sigmoid, float* out_score, float* out_delta, float* out_pc,
                         int* out_idx, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(cls_score && bbox_delta && pc && out_score && out_delta && out_pc && ws, RD_EINVAL, "sorted_foreground: null pointer");
  RD_REQUIRE(B > 0 && N > 0 && k > 0 && D > 0, RD_ESHAPE, "sorted_foreground: empty shape");
  RD_REQUIRE(N >= k, RD_ESHAPE, "sorted_foreground: N (%ld) < num_fgs (%ld)", N, k);  // get_sorted_foreground.py:65
  RD_REQUIRE(N < (1L << 31), RD_ESHAPE, "sorted_foreground: N too large");
  RD_REQUIRE(ws_bytes >= rd_sorted_foreground_workspace_bytes(N, k), RD_EWORKSPACE, "sorted_foreground: workspace %zu < %zu",
             ws_bytes, rd_sorted_foreground_workspace_bytes(N, k));
  hipStream_t st = (hipStream_t)stream;
  void* wsa = (void*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  SortWs s = sort_ws_carve(wsa, N);
  ProfScope ps(RD_PROF_SORT, st);
  // the B batch elements are independent sorts: side by side (blockIdx.y) when the workspace holds B problems,
  // otherwise one after the other in a single-problem workspace
  const size_t per = rd_sorted_foreground_workspace_bytes(N, k);
  const bool wide = ws_bytes >= per * (size_t)B;
  const long stride = wide ? (long)(per / 4) : 0;
  const int nb = wide ? B : 1;
  for (int b0 = 0; b0 < B; b0 += nb) {
    hipLaunchKernelGGL(sort_keygen_kernel, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, st, cls_score + (size_t)b0 * N,
                       mask ? mask + (size_t)b0 * N : nullptr, N, apply_sigmoid, s.keysA, s.idxA, stride);
    unsigned *rk, *ri;
    int rc = radix_topk_pairs(s, N, k, st, nb, stride, &rk, &ri);
    if (rc != RD_OK) return rc;
    hipLaunchKernelGGL(sort_gather_kernel, dim3((unsigned)((k + 255) / 256), nb), dim3(256), 0, st, rk, ri, k, D,
                       bbox_delta + (size_t)b0 * N * D, pc + (size_t)b0 * N * 3, out_score + (size_t)b0 * k,
                       out_delta + (size_t)b0 * k * D, out_pc + (size_t)b0 * k * 3, out_idx ? out_idx + (size_t)b0 * k : nullptr,
                       stride, N);
  }
  return check_launch("sorted_foreground");
}

int rd_decode3d_bbox(const float* bbox_delta, const float* pc, float* out, int B, long N, int box_type, int is_bin,
                     void* stream) {
  RD_REQUIRE(bbox_delta && pc && out, RD_EINVAL, "decode3d: null pointer");
  RD_REQUIRE(B > 0 && N > 0, RD_ESHAPE, "decode3d: empty shape");
  RD_REQUIRE((is_bin && box_type == 7) || (!is_bin && box_type == 8), RD_ESHAPE,
             "decode3d: box_type %d with is_bin=%d (8 for regular, 7 for bin)", box_type, is_bin);
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)B * N;
  ProfScope ps(RD_PROF_DECODE, st);
  hipLaunchKernelGGL(decode3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bbox_delta, pc, out, n, box_type, is_bin);
  return check_launch("decode3d");
}

size_t rd_score_filter_workspace_bytes(long n) { return (size_t)((n + 255) / 256 + 8) * 4 + 256; }
int rd_score_filter_dets_batched(const float* scores, long scores_bstride, const float* boxes10, long boxes_bstride,
                                 long n, float min_score, float* dets, long dets_bstride, int* d_count, void* ws,
                                 size_t ws_bytes, int B, void* stream) {
  RD_REQUIRE(scores && boxes10 && dets && d_count && ws, RD_EINVAL, "score_filter: null pointer");
  RD_REQUIRE(n > 0 && B > 0, RD_ESHAPE, "score_filter: empty input");
  const size_t per = rd_score_filter_workspace_bytes(n);
  RD_REQUIRE(ws_bytes >= per * (size_t)B, RD_EWORKSPACE, "score_filter: workspace %zu < %zu", ws_bytes, per * (size_t)B);
  hipStream_t st = (hipStream_t)stream;
  int* blk = (int*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  const int nblk = (int)((n + 255) / 256);
  const long blk_bs = nblk + 8;                  // per-frame block-count arrays (ints apart)
  ProfScope ps(RD_PROF_WNMS, st);
  hipLaunchKernelGGL(filter_count_kernel, dim3(nblk, B), dim3(256), 0, st, scores, n, min_score, blk, scores_bstride, blk_bs);
  hipLaunchKernelGGL(filter_scan_kernel, dim3(B), dim3(256), 0, st, blk, nblk, d_count, blk_bs);
  hipLaunchKernelGGL(filter_scatter_kernel, dim3(nblk, B), dim3(256), 0, st, scores, boxes10, n, min_score, blk, dets,
                     scores_bstride, boxes_bstride, blk_bs, dets_bstride);
  return check_launch("score_filter");
}
int rd_score_filter_dets(const float* scores, const float* boxes10, long n, float min_score, float* dets, int* d_count,
                         void* ws, size_t ws_bytes, void* stream) {
  return rd_score_filter_dets_batched(scores, 0, boxes10, 0, n, min_score, dets, 0, d_count, ws, ws_bytes, 1, stream);
}

size_t rd_wnms_workspace_bytes(int Kcap) { return Kcap > 0 ? wnms_ws_bytes(Kcap) : 0; }
int rd_wnms_4c_batched(const float* dets, long dets_bstride, int Kcap, const int* d_count, const int* order,
                       long order_bstride, int tie_order, float thresh, float thresh_vote, int is3d, int hash_scale,
                       float* out_dets, long out_bstride, int* keep, long keep_bstride, int* d_nkeep, void* ws,
                       size_t ws_bytes, int B, void* stream) {
  RD_REQUIRE(dets && out_dets && keep && d_nkeep && ws, RD_EINVAL, "wnms_4c: null pointer");
  RD_REQUIRE(Kcap > 0 && Kcap <= RD_WNMS_MAX_K, RD_ESHAPE, "wnms_4c: Kcap %d not in [1, %d]", Kcap, RD_WNMS_MAX_K);
  RD_REQUIRE(B > 0, RD_ESHAPE, "wnms_4c: batch %d", B);
  // diagnostic bits of tie_order (include/rangedet_hip.h RD_WNMS_DIAG_*): per-call test aids, results do not depend on them
  const int diag = tie_order & ~0xff;
  tie_order &= 0xff;
  RD_REQUIRE(tie_order == RD_TIE_STABLE || tie_order == RD_TIE_REFERENCE, RD_EINVAL, "wnms_4c: tie_order %d", tie_order);
  RD_REQUIRE(!(diag & ~(RD_WNMS_DIAG_NO_SKIP | (0xff << 16) | (0x7f << 24))), RD_EINVAL, "wnms_4c: unknown diagnostic bits 0x%x", diag);
  const size_t per = rd_wnms_workspace_bytes(Kcap);
  RD_REQUIRE(ws_bytes >= per * (size_t)B, RD_EWORKSPACE, "wnms_4c: workspace %zu < %zu", ws_bytes, per * (size_t)B);
  RD_REQUIRE(order || B == 1 || tie_order == RD_TIE_REFERENCE, RD_EINVAL,
             "wnms_4c: the batched call needs an explicit processing order or RD_TIE_REFERENCE");
  hipStream_t st = (hipStream_t)stream;
  // (every kernel of the chain that may take more than 64 KB of dynamic LDS, once per device: no runtime-API call besides the launches
  //  themselves is left on the path, so the whole chain can be captured into a hipGraph -- pipeline.RangeDetPipeline(graph=True))
  static std::atomic<unsigned long long> seen_lds{0};
  once_per_device(seen_lds, [] {
    allow_big_lds(wnms_tie_order_kernel); allow_big_lds(wnms_scan_kernel); allow_big_lds(wnms_scan4_kernel); allow_big_lds(wnms_merge_kernel);
  });
  WnmsWs w = wnms_ws_carve(ws, Kcap);
  ProfScope ps(RD_PROF_WNMS, st);
  // consecutive frames use consecutive `per`-byte workspaces (per is a multiple of 256), so every carved array of
  // frame b sits b * per bytes after frame 0's
  WnmsBatch bs;
  bs.dets = dets_bstride; bs.order = order_bstride; bs.prep = (long)(per / 4); bs.words = (long)(per / 8);
  bs.ints = (long)(per / 4); bs.keep = keep_bstride; bs.out = out_bstride;
  const int* ord = order;
  if (!ord && tie_order == RD_TIE_REFERENCE) {   // the reference's own order: std::sort replayed on the device
    const size_t lds = TIE_STACK_BYTES + (Kcap <= TIE_LDS_K ? (size_t)Kcap * 8 + 3 * ((size_t)Kcap / 32 + 2) * 4 : 0);
    hipLaunchKernelGGL(wnms_tie_order_kernel, dim3(1, 1, B), dim3(256), lds, st, dets, Kcap, d_count, w.order, bs, (long)(per / 4),
                       w.scratch);
    ord = w.order;
    bs.order = (long)(per / 4);
  } else if (!ord) {  // device ordering: score descending, ties by row index ascending
    void* swa = (void*)(((uintptr_t)w.sort_ws + 255) & ~(uintptr_t)255);
    SortWs s = sort_ws_carve(swa, Kcap);
    hipLaunchKernelGGL(sort_keygen_dets_kernel, dim3((Kcap + 255) / 256), dim3(256), 0, st, dets, Kcap, d_count, s.keysA, s.idxA);
    int rc = radix_sort_pairs(s, Kcap, st);
    if (rc != RD_OK) return rc;
    if (hipMemcpyAsync(w.order, s.idxA, (size_t)Kcap * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return rd::fail(RD_EHIP, "wnms_4c: order copy");
    ord = w.order;
    bs.order = 0;
  }
  const int nb = (Kcap + 63) / 64;
  hipLaunchKernelGGL(wnms_prep_kernel, dim3((Kcap + 255) / 256, 1, B), dim3(256), 0, st, dets, ord, Kcap, d_count, w.prep, bs,
                     (float)hash_scale, w.novf);
  // RD_WNMS_DIAG_TILE_W(n) / RD_WNMS_DIAG_MERGE_LDS(n): per-call test aids that force the column-chunked scan and the merge overflow
  // path at small K (environment variables until round 5)
  const int e_tw = (diag >> 16) & 0xff, e_ml = (diag >> 24) & 0x7f;
  const int tile_w = std::min(w.nwcap, e_tw ? std::max(1, e_tw) : 256);
  const size_t scan_lds = ((size_t)w.nwcap + (size_t)64 * tile_w) * 8;
  // Two rounds.  The greedy scan only ever reads the thr / vote rows of boxes it KEEPS, and the highest-scoring boxes
  // suppress most of the rest: round 1 evaluates the pairs of the first R1 rows and scans them; round 2 evaluates pairs
  // only for the later rows that are still unsuppressed (compacted list) and resumes the scan.  Results are identical
  // to the one-round form -- the skipped rows are exactly the ones whose bits nobody reads.
  const int R1 = 256, nb1 = R1 / 64;
  const bool two = Kcap >= 4 * R1;
  // pair tiles are strided over a fixed number of single-wave workgroups per frame: one tile each at the pipeline's typical K
  // (1 - 2 k rows: <= 2048 tiles per round), grid-strided beyond that -- so the launch size does not grow with the capacity
  // (8 columns per pair tile, k_wnms.h: 8 tiles per mask word)
  const int pgrid = std::min(2048, std::max(64, nb * 8 * std::min(nb, 16)));
  // the rejection test of the pair kernel (k_wnms.h w_pair_skippable) is only sound for thresholds far above the noise the
  // reference's clipper returns on disjoint boxes (<= 4.2e-7 inside the test's domain, profiles/r04_nms_spurious_study.txt), and it
  // was characterised on the BEV value only: in 3-D mode the reference divides the clipped area x height overlap by a volume sum
  // that non-positive or cancelling heights can make arbitrarily small (nms.h:234-246), so there every pair is clipped.
  // RD_WNMS_DIAG_NO_SKIP (per call): every pair clipped (A/B)
  const int allow_skip = thresh >= 1e-3f && thresh_vote >= 1e-3f && !is3d && !(diag & RD_WNMS_DIAG_NO_SKIP);
  auto pairs = [&](const int* rows, const int* nrows, const unsigned long long* supp, int rb_end) {
    hipLaunchKernelGGL(wnms_pairs_kernel, dim3(pgrid, 1, B), dim3(64), 0, st, w.prep, Kcap, d_count, thresh, thresh_vote, is3d, w.thr, w.vote,
                       w.nwcap, bs, rows, nrows, supp, 0, rb_end, allow_skip);
  };
  pairs(nullptr, nullptr, nullptr, two ? nb1 : nb);
  // capacities up to 8 192 rows: the four-wave scan with grouped staging (a forced tile width: the single-wave form)
  const bool scan4 = w.nwcap <= 128 && !e_tw;
  const int tile_words = 64 * 128;
  const size_t scan4_lds = ((size_t)w.nwcap + tile_words) * 8;
  auto scan = [&](int c_begin, int c_end, unsigned long long* state) {
    if (scan4)
      hipLaunchKernelGGL(wnms_scan4_kernel, dim3(1, 1, B), dim3(256), scan4_lds, st, w.thr, w.snap, Kcap, d_count, w.nwcap, ord,
                         w.keep_q, keep, d_nkeep, bs, c_begin, c_end, state, tile_words);
    else
      hipLaunchKernelGGL(wnms_scan_kernel, dim3(1, 1, B), dim3(64), scan_lds, st, w.thr, w.snap, Kcap, d_count, w.nwcap, ord,
                         w.keep_q, keep, d_nkeep, bs, c_begin, c_end, state, tile_w);
  };
  scan(0, two ? nb1 : nb, two ? w.supp_state : (unsigned long long*)nullptr);
  if (two) {
    hipLaunchKernelGGL(wnms_alive_kernel, dim3(1, 1, B), dim3(256), 0, st, w.supp_state, Kcap, d_count, R1, w.alive, w.nalive, bs);
    pairs((const int*)w.alive, (const int*)w.nalive, (const unsigned long long*)w.supp_state, 0);
    scan(nb1, nb, w.supp_state);
  }
  // neighbourhood list of a kept row: 2 048 entries (16 KB) in LDS -- the lists are a few dozen entries long; a frame with more
  // candidates than that counts each row's list first and sends the rare longer one through the global-scratch kernel.  (With the
  // former 16 384 entries every single-wave workgroup asked for 65 KB: in the pipeline, where the conv workgroups hold 2 x 80 KB
  // per CU, the merge took 80 us instead of 21; +0.3 % frames/s)
  const int lds_cap = std::min(Kcap + 2, e_ml ? std::max(4, e_ml) : 2048);
  hipLaunchKernelGGL(wnms_merge_kernel, dim3(std::min(Kcap, 4096), 1, B), dim3(64), (size_t)lds_cap * 8, st, dets, ord, w.vote,
                     w.snap, Kcap, d_count, w.nwcap, w.keep_q, d_nkeep, out_dets, bs, lds_cap, w.ovf, w.novf);
  if (Kcap + 2 > lds_cap)
    hipLaunchKernelGGL(wnms_merge_big_kernel, dim3(1, 1, B), dim3(64), 0, st, dets, ord, w.vote, w.snap, Kcap, d_count, w.nwcap,
                       w.keep_q, out_dets, bs, (const int*)w.ovf, (const int*)w.novf, w.scratch);
  return check_launch("wnms_4c");
}
int rd_wnms_4c(const float* dets, int Kcap, const int* d_count, const int* order, int tie_order, float thresh,
               float thresh_vote, int is3d, int hash_scale, float* out_dets, int* keep, int* d_nkeep, void* ws,
               size_t ws_bytes, void* stream) {
  return rd_wnms_4c_batched(dets, 0, Kcap, d_count, order, 0, tie_order, thresh, thresh_vote, is3d, hash_scale, out_dets, 0,
                            keep, 0, d_nkeep, ws, ws_bytes, 1, stream);
}
int rd_single_overlap(const float* dets_a, const float* dets_b, long n, int is3d, float* out, void* stream) {
  RD_REQUIRE(n >= 0 && (n == 0 || (dets_a && dets_b && out)), RD_EINVAL, "single_overlap: bad arguments");
  if (n == 0) return RD_OK;
  hipLaunchKernelGGL(single_overlap_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dets_a, dets_b, n,
                     is3d, out);
  return check_launch("single_overlap");
}
int rd_wnms_pair_skippable(const float* dets_a, const float* dets_b, long n, unsigned char* out, void* stream) {
  RD_REQUIRE(dets_a && dets_b && out && n >= 0, RD_EINVAL, "wnms_pair_skippable: null pointer");
  if (n == 0) return RD_OK;
  hipLaunchKernelGGL(pair_skippable_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dets_a, dets_b, n, out);
  return check_launch("wnms_pair_skippable");
}
namespace rd {
__global__ void atan2f_kernel(const float* y, const float* x, long n, float* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fdlibm_atan2f(y[i], x[i]);
}
}  // namespace rd
int rd_edge_atan2f(const float* y, const float* x, long n, float* out, void* stream) {
  RD_REQUIRE(y && x && out && n >= 0, RD_EINVAL, "edge_atan2f: null pointer");
  if (n == 0) return RD_OK;
  hipLaunchKernelGGL(atan2f_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, x, n, out);
  return check_launch("edge_atan2f");
}
int rd_wnms_order_host(const float* dets_host, int K, int* order_host) {
  RD_REQUIRE(K >= 0 && (K == 0 || (dets_host && order_host)), RD_EINVAL, "wnms_order_host: bad arguments");
  // the reference's ordering, literally (nms.h:786-792): std::sort is unstable, so equal scores come out in
  // libstdc++ introsort order -- reproduced by running the same call on the host.
  std::iota(order_host, order_host + K, 0);
  std::sort(order_host, order_host + K, [&](int i, int j) { return dets_host[i * 12 + 11] > dets_host[j * 12 + 11]; });
  return RD_OK;
}

int rd_dets12_to_8_batched(const float* dets12, long dets12_bstride, int Mcap, const int* d_count, float* out8,
                           long out8_bstride, int B, void* stream) {
  RD_REQUIRE(dets12 && out8, RD_EINVAL, "dets12_to_8: null pointer");
  RD_REQUIRE(Mcap > 0 && B > 0, RD_ESHAPE, "dets12_to_8: empty input");
  hipLaunchKernelGGL(dets12_to_8_kernel, dim3((Mcap + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, dets12, Mcap, d_count,
                     out8, dets12_bstride, out8_bstride);
  return check_launch("dets12_to_8");
}
int rd_dets12_to_8(const float* dets12, int Mcap, const int* d_count, float* out8, void* stream) {
  return rd_dets12_to_8_batched(dets12, 0, Mcap, d_count, out8, 0, 1, stream);
}

int rd_gather_keep_scores(const float* score, long score_bstride, int k, const int* keep_idx, int max_keep, float* out, int B,
                          void* stream) {
  RD_REQUIRE(score && keep_idx && out, RD_EINVAL, "gather_keep_scores: null pointer");
  RD_REQUIRE(k > 0 && max_keep > 0 && B > 0, RD_ESHAPE, "gather_keep_scores: empty input");
  hipLaunchKernelGGL(gather_keep_scores_kernel, dim3((max_keep + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, score,
                     score_bstride, k, keep_idx, max_keep, out);
  return check_launch("gather_keep_scores");
}

int rd_rotated_iou_8pt(const float* boxes1, const float* boxes2, float* ious, long n1, long n2, void* stream) {
  RD_REQUIRE(boxes1 && boxes2 && ious, RD_EINVAL, "rotated_iou: null pointer");
  RD_REQUIRE(n1 > 0 && n2 > 0, RD_ESHAPE, "rotated_iou: empty input");
  hipLaunchKernelGGL(riou8_kernel, dim3((unsigned)((n1 * n2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes1, boxes2, ious, n1, n2);
  return check_launch("rotated_iou_8pt");
}
int rd_batch_rotated_iou(const float* proposal, int p_stride, const float* gt_bbox, float* iou_map, int* argmax, int B, long N,
                         int n_gt, void* stream) {
  RD_REQUIRE(proposal && gt_bbox && iou_map, RD_EINVAL, "batch_rotated_iou: null pointer");
  RD_REQUIRE(B > 0 && B <= 65535 && N > 0 && n_gt > 0 && n_gt <= 256 && p_stride >= 8, RD_ESHAPE,
             "batch_rotated_iou: B %d, N %ld, n_gt %d (<= 256), proposal row %d floats (>= 8)", B, N, n_gt, p_stride);
  hipLaunchKernelGGL(batch_riou_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, proposal, p_stride,
                     N * (long)p_stride, gt_bbox, (long)n_gt * 8, iou_map, argmax, N, n_gt);
  return check_launch("batch_rotated_iou");
}
int rd_rotated_iou_7(const float* boxes1, const float* boxes2, float* ious, long n1, long n2, void* stream) {
  RD_REQUIRE(boxes1 && boxes2 && ious, RD_EINVAL, "rotated_iou_7: null pointer");
  if (n1 * n2 == 0) return RD_OK;
  hipLaunchKernelGGL(riou7_kernel, dim3((unsigned)((n1 * n2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes1, boxes2, ious, n1, n2);
  return check_launch("rotated_iou_7");
}
int rd_batch_rotated_iou_3d(const float* proposal, int p_stride, const float* gt_bbox7, float* iou_map, int* argmax, int B, long N,
                            int n_gt, void* stream) {
  RD_REQUIRE(proposal && gt_bbox7 && iou_map, RD_EINVAL, "batch_rotated_iou_3d: null pointer");
  RD_REQUIRE(B > 0 && N > 0 && p_stride >= 10, RD_ESHAPE, "batch_rotated_iou_3d: proposal rows need the 8 corners + z0, z1 (stride %d)", p_stride);
  RD_REQUIRE(n_gt >= 1 && n_gt <= 256, RD_ESHAPE, "batch_rotated_iou_3d: n_gt %d (1..256; the config pads to 200)", n_gt);
  ProfScope ps(RD_PROF_DECODE, (hipStream_t)stream);
  hipLaunchKernelGGL(batch_riou3d_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, proposal, p_stride,
                     (long)N * p_stride, gt_bbox7, (long)n_gt * 7, iou_map, argmax, N, n_gt);
  return check_launch("batch_rotated_iou_3d");
}
int rd_batch_max_iou(const float* proposals, int p_stride, const float* gt8, float* out, long n, int n_gt, void* stream) {
  return rd_batch_rotated_iou(proposals, p_stride, gt8, out, nullptr, 1, n, n_gt, stream);
}

// ---- greedy 3-D NMS (_contrib_NMS3D) ----------------------------------------------------------------------------------
size_t rd_nms3d_workspace_bytes(long N, int B) {
  if (N <= 0 || N > (1 << 18) || B <= 0) return 0;
  return nms3d_frame_bytes((int)N) * (size_t)B;
}
int rd_nms3d(const float* boxes, int B, long N, float iou_thres, int max_keep, int normal_iou, int* keep_idx,
             float* bbox_after_nms, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(boxes && keep_idx && bbox_after_nms && ws, RD_EINVAL, "nms3d: null pointer");
  RD_REQUIRE(B > 0 && B <= 65535 && N > 0 && N <= (1 << 18) && max_keep > 0, RD_ESHAPE, "nms3d: B %d, N %ld (<= 262144), max_keep %d", B, N, max_keep);
  RD_REQUIRE(ws_bytes >= rd_nms3d_workspace_bytes(N, B), RD_EWORKSPACE, "nms3d: workspace %zu < %zu bytes", ws_bytes, rd_nms3d_workspace_bytes(N, B));
  RD_REQUIRE(((uintptr_t)ws & 7) == 0, RD_EINVAL, "nms3d: workspace must be 8-byte aligned");
  Nms3dArgs a;
  a.boxes = boxes; a.ws = (unsigned char*)ws; a.ws_frame = nms3d_frame_bytes((int)N);
  a.keep = keep_idx; a.out = bbox_after_nms;
  a.N = (int)N; a.ncw = (int)((N + 63) / 64); a.max_keep = max_keep; a.normal_iou = normal_iou ? 1 : 0; a.thresh = iou_thres;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(RD_PROF_WNMS, st);
  const int gi = (std::max(std::max(a.ncw, max_keep), 2) + 255) / 256;
  hipLaunchKernelGGL(nms3d_init_kernel, dim3(gi, B), dim3(256), 0, st, a);
  for (int r0 = 0, blk = 64; r0 < a.N; r0 += blk, blk = std::min(2 * blk, NMS3D_RB)) {
    const int rows = std::min(blk, a.N - r0);
    hipLaunchKernelGGL(nms3d_pairs_kernel, dim3((a.N + NMS3D_SEG - 1) / NMS3D_SEG, rows, B), dim3(256), 0, st, a, r0);
    hipLaunchKernelGGL(nms3d_scan_kernel, dim3(B), dim3(256), (size_t)a.ncw * 8, st, a, r0, blk);
  }
  return check_launch("nms3d");
}

// ---- target assignment (processing_cxx.assign3D_v2 / get_point_num) --------------------------------------------------
int rd_assign3d_v2(const float* pc, const float* bbox, const float* bbox_center, const float* bbox_radius, const float* mask,
                   const float* is_in_nlz, long N, int M, float max_x, float min_x, float max_y, float min_y, float max_z,
                   float min_z, float max_dist, int* out, void* stream) {
  RD_REQUIRE(pc && bbox && bbox_center && bbox_radius && mask && is_in_nlz && out, RD_EINVAL, "assign3d_v2: null pointer");
  RD_REQUIRE(N > 0 && M > 0 && M <= ASSIGN_MAX_BOXES, RD_ESHAPE, "assign3d_v2: N %ld, M %d (1..%d)", N, M, ASSIGN_MAX_BOXES);
  AssignArgs a;
  a.pc = pc; a.bbox = bbox; a.center = bbox_center; a.radius = bbox_radius; a.mask = mask; a.nlz = is_in_nlz; a.out = out;
  a.N = N; a.M = M;
  a.max_x = max_x; a.min_x = min_x; a.max_y = max_y; a.min_y = min_y; a.max_z = max_z; a.min_z = min_z; a.max_dist = max_dist;
  hipLaunchKernelGGL(assign3d_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), (size_t)M * ASSIGN_BOX_F * 4, (hipStream_t)stream, a);
  return check_launch("assign3d_v2");
}
size_t rd_get_point_num_workspace_bytes(void) { return POINT_NUM_MAX_BOXES * sizeof(int); }
int rd_get_point_num(const float* bbox_inds, long N, float* out, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(bbox_inds && out && ws, RD_EINVAL, "get_point_num: null pointer");
  RD_REQUIRE(N > 0, RD_ESHAPE, "get_point_num: N %ld", N);
  RD_REQUIRE(ws_bytes >= rd_get_point_num_workspace_bytes(), RD_EWORKSPACE, "get_point_num: workspace %zu < %zu bytes", ws_bytes,
             rd_get_point_num_workspace_bytes());
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, rd_get_point_num_workspace_bytes(), st) != hipSuccess) return fail(RD_EHIP, "get_point_num: memset failed");
  const unsigned g = (unsigned)std::min<long>((N + 255) / 256, 1024);
  hipLaunchKernelGGL(point_num_count_kernel, dim3(g), dim3(256), 0, st, bbox_inds, N, (int*)ws);
  hipLaunchKernelGGL(point_num_gather_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, bbox_inds, N, (const int*)ws, out);
  return check_launch("get_point_num");
}

// ---- input transform chain ----------------------------------------------------------------------------------------
int rd_input_transform(const float* range_image, const float* pc_vehicle_frame, const float* inclination,
                       const rd_input_norm_t* norm_host, int B, int H, int W, int Hp, int Wp, float* input_data,
                       float* coord_s1, float* pc_s1, float* pc_s2, float* pc_s4, float* mask_s1, float* mask_s2,
                       float* mask_s4, void* stream) {
  RD_REQUIRE(range_image && pc_vehicle_frame && inclination && norm_host && input_data && coord_s1 && pc_s1 && pc_s2 && pc_s4 &&
                 mask_s1 && mask_s2 && mask_s4, RD_EINVAL, "input_transform: null pointer");
  RD_REQUIRE(B > 0 && H > 2 && W > 2 && Hp >= H && Wp >= W && Wp % 4 == 0, RD_ESHAPE,
             "input_transform: shape (%d,%d,%d) -> (%d,%d)", B, H, W, Hp, Wp);
  InputArgs a;
  a.ri = range_image; a.pc = pc_vehicle_frame; a.incl = inclination;
  a.data = input_data; a.coord = coord_s1;
  a.pcs[0] = pc_s1; a.pcs[1] = pc_s2; a.pcs[2] = pc_s4;
  a.msk[0] = mask_s1; a.msk[1] = mask_s2; a.msk[2] = mask_s4;
  a.B = B; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp;
  a.n = *norm_host;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(RD_PROF_LAYOUT, st);
  hipLaunchKernelGGL(input_transform_kernel, dim3((unsigned)(((long)Hp * Wp + 255) / 256), B), dim3(256), 0, st, a);
  return check_launch("input_transform");
}

// ---- training-time input chain (k_target.h) --------------------------------------------------------------------------
size_t rd_train_transform_workspace_bytes(int B) { return B > 0 ? (size_t)B * POINT_NUM_MAX_BOXES * sizeof(int) : 0; }
int rd_train_transform(const float* range_image, const float* pc_vehicle_frame, const float* inclination,
                       const rd_input_norm_t* norm_host, const float* gt_bbox_imu, const float* gt_bbox_center,
                       const float* gt_limits, const float* gt_bbox_csa, const int* num_gt_host, int Mmax, float radius,
                       float max_dist, const float* reg_weight_host, int B, int H, int W, int Hp, int Wp,
                       const rd_train_outputs_t* out_host, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(range_image && pc_vehicle_frame && inclination && norm_host && gt_bbox_imu && gt_bbox_center && gt_limits && gt_bbox_csa &&
                 num_gt_host && reg_weight_host && out_host && ws, RD_EINVAL, "train_transform: null pointer");
  const rd_train_outputs_t& o = *out_host;
  bool all = o.input_data && o.coord_s1 && o.bbox3d_ind;
  for (int l = 0; l < 3; ++l)
    all = all && o.pc[l] && o.mask[l] && o.reg_target[l] && o.reg_weight[l] && o.reg_normalize_weight[l] && o.cls_target[l];
  RD_REQUIRE(all, RD_EINVAL, "train_transform: null output pointer");
  RD_REQUIRE(B > 0 && H > 2 && W > 2 && Hp >= H && Wp >= W && Wp % 4 == 0, RD_ESHAPE,
             "train_transform: shape (%d,%d,%d) -> (%d,%d)", B, H, W, Hp, Wp);
  RD_REQUIRE(Mmax >= 1, RD_ESHAPE, "train_transform: Mmax %d", Mmax);
  for (int b = 0; b < B; ++b)
    RD_REQUIRE(num_gt_host[b] >= 1 && num_gt_host[b] <= std::min(Mmax, POINT_NUM_MAX_BOXES), RD_ESHAPE,
               "train_transform: num_gt[%d] = %d (1..%d)", b, num_gt_host[b], std::min(Mmax, POINT_NUM_MAX_BOXES));
  RD_REQUIRE(ws_bytes >= rd_train_transform_workspace_bytes(B), RD_EWORKSPACE, "train_transform: workspace %zu < %zu bytes", ws_bytes,
             rd_train_transform_workspace_bytes(B));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, rd_train_transform_workspace_bytes(B), st) != hipSuccess) return fail(RD_EHIP, "train_transform: memset failed");
  TrainArgs a;
  a.ri = range_image; a.pc = pc_vehicle_frame; a.incl = inclination;
  a.gt_imu = gt_bbox_imu; a.gt_center = gt_bbox_center; a.gt_limits = gt_limits; a.gt_csa = gt_bbox_csa;
  a.ind = o.bbox3d_ind; a.counts = (int*)ws; a.o = o;
  a.Mmax = Mmax; a.radius = radius; a.max_dist = max_dist;
  for (int c = 0; c < 8; ++c) a.reg_weight[c] = reg_weight_host[c];
  a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp;
  a.n = *norm_host;
  ProfScope ps(RD_PROF_LAYOUT, st);
  // the counts of a frame are complete when pass 1 of its chunk has finished: same stream, so pass 2 of the chunk may follow directly
  for (int b0 = 0; b0 < B; b0 += TRAIN_FRAMES_PER_LAUNCH) {
    const int nb = std::min(TRAIN_FRAMES_PER_LAUNCH, B - b0);
    int mmax = 0;
    for (int i = 0; i < TRAIN_FRAMES_PER_LAUNCH; ++i) {
      a.num_gt[i] = i < nb ? num_gt_host[b0 + i] : 0;
      mmax = std::max(mmax, a.num_gt[i]);
    }
    a.b0 = b0;
    hipLaunchKernelGGL(train_assign_kernel, dim3((unsigned)(((long)H * W + 255) / 256), nb), dim3(256), (size_t)mmax * ASSIGN_BOX_F * 4, st, a);
    hipLaunchKernelGGL(train_write_kernel, dim3((unsigned)(((long)Hp * Wp + 255) / 256), nb), dim3(256), 0, st, a);
  }
  return check_launch("train_transform");
}

// ---- range image from a raw point cloud (k_rangeimg.h) ------------------------------------------------------------------
size_t rd_range_image_workspace_bytes(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 ? (size_t)B * H * W * sizeof(unsigned long long) : 0;
}
int rd_range_image_from_points(const float* points, const long long* offsets_host, int B, const double* incl_host,
                               const double* height_host, int H, int W, float* range_image, unsigned char* mask, int* point_index,
                               void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(offsets_host && incl_host && height_host && range_image && mask && ws, RD_EINVAL, "range_image_from_points: null pointer");
  RD_REQUIRE(B >= 1 && H >= 1 && H <= RI_MAX_BEAMS && W >= 1 && W <= RI_MAX_WIDTH, RD_ESHAPE,
             "range_image_from_points: B %d, H %d (1..%d), W %d (1..%d)", B, H, RI_MAX_BEAMS, W, RI_MAX_WIDTH);
  RD_REQUIRE(offsets_host[0] == 0, RD_ESHAPE, "range_image_from_points: offsets[0] = %lld, not 0", offsets_host[0]);
  for (int b = 0; b < B; ++b) {
    const long long n = offsets_host[b + 1] - offsets_host[b];
    RD_REQUIRE(n >= 0 && n < (1LL << 31), RD_ESHAPE, "range_image_from_points: scan %d has %lld points (0..2^31-1)", b, n);
  }
  RD_REQUIRE(points || offsets_host[B] == 0, RD_EINVAL, "range_image_from_points: null points");
  RD_REQUIRE(((uintptr_t)points | (uintptr_t)range_image) % 16 == 0 && (uintptr_t)ws % 8 == 0, RD_EINVAL,
             "range_image_from_points: points and range_image must be 16-byte aligned, the workspace 8-byte aligned");
  const size_t need = rd_range_image_workspace_bytes(B, H, W);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "range_image_from_points: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0xFF, need, st) != hipSuccess) return fail(RD_EHIP, "range_image_from_points: memset failed");   // every key = RI_EMPTY
  RangeImgArgs a;
  a.points = points; a.key = (unsigned long long*)ws;
  a.range_image = range_image; a.mask = mask; a.point_index = point_index;
  a.H = H; a.W = W;
  for (int r = 0; r < RI_MAX_BEAMS; ++r) { a.incl[r] = r < H ? incl_host[r] : 0.0; a.height[r] = r < H ? height_host[r] : 0.0; }
  ProfScope ps(RD_PROF_LAYOUT, st);
  const unsigned cell_blocks = (unsigned)(((long long)H * W + 255) / 256);
  for (int b0 = 0; b0 < B; b0 += RI_SCANS_PER_LAUNCH) {
    const int nb = std::min(RI_SCANS_PER_LAUNCH, B - b0);
    long long nchunk = 0;
    for (int i = 0; i <= RI_SCANS_PER_LAUNCH; ++i) a.off[i] = offsets_host[b0 + std::min(i, nb)];
    for (int i = 0; i < nb; ++i) nchunk = std::max(nchunk, a.off[i + 1] - a.off[i]);
    a.b0 = b0;
    if (nchunk > 0)
      hipLaunchKernelGGL(range_image_project_kernel, dim3((unsigned)((nchunk + 255) / 256), nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(range_image_resolve_kernel, dim3(cell_blocks, nb), dim3(256), 0, st, a);
  }
  return check_launch("range_image_from_points");
}

// ---- RPN loss head of one level (k_loss.h) -------------------------------------------------------------------------------
size_t rd_rpn_loss_workspace_bytes(int B, long n) { return B > 0 && B <= 65535 && n > 0 ? loss_ws_bytes(B, n) : 0; }
int rd_rpn_loss(const float* logit, long logit_bstride, const float* delta, long delta_bstride, const float* pc, const float* gt_bbox,
                int n_gt, const float* mask, const float* reg_target, const float* reg_weight, const float* reg_norm_weight, int B, int H,
                int Wl, const rd_loss_param_t* p_host, float* cls_loss, float* reg_loss, float* d_logit, float* d_delta,
                float* iou_target, float* boxes10, float* stats, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(logit && delta && pc && gt_bbox && mask && reg_target && reg_weight && reg_norm_weight && p_host && cls_loss && reg_loss &&
                 stats && ws, RD_EINVAL, "rpn_loss: null pointer");
  RD_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && Wl >= 1, RD_ESHAPE, "rpn_loss: B %d (1..65535), H %d, Wl %d", B, H, Wl);
  RD_REQUIRE(n_gt >= 1 && n_gt <= 256, RD_ESHAPE, "rpn_loss: n_gt %d (1..256; the config pads to 200)", n_gt);
  const long n = (long)H * Wl;
  RD_REQUIRE(logit_bstride >= n && delta_bstride >= 8 * n && delta_bstride % 4 == 0, RD_ESHAPE,
             "rpn_loss: batch strides %ld (>= %ld) and %ld (>= %ld, a multiple of 4)", logit_bstride, n, delta_bstride, 8 * n);
  RD_REQUIRE(((uintptr_t)delta | (uintptr_t)d_delta) % 16 == 0 && (uintptr_t)ws % 8 == 0, RD_EINVAL,
             "rpn_loss: delta and d_delta must be 16-byte aligned, the workspace 8-byte aligned");
  RD_REQUIRE(p_host->smooth_l1_scalar > 0.f, RD_EINVAL, "rpn_loss: smooth_l1_scalar %g (> 0)", (double)p_host->smooth_l1_scalar);
  const size_t need = rd_rpn_loss_workspace_bytes(B, n);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "rpn_loss: workspace %zu < %zu bytes", ws_bytes, need);
  LossArgs a;
  a.logit = logit; a.delta = delta; a.pc = pc; a.gt = gt_bbox; a.mask = mask;
  a.reg_target = reg_target; a.reg_weight = reg_weight; a.reg_norm_weight = reg_norm_weight;
  a.logit_bs = logit_bstride; a.delta_bs = delta_bstride; a.n = n; a.B = B; a.ngt = n_gt;
  a.p = *p_host;
  a.cls_loss = cls_loss; a.reg_loss = reg_loss; a.d_logit = d_logit; a.d_delta = d_delta; a.iou_target = iou_target; a.boxes10 = boxes10;
  a.stats = stats;
  a.norm_blocks = loss_norm_blocks(B, n);
  const long npix = loss_pixel_blocks(B, n);
  a.part_mask = (double*)ws; a.part_nw = a.part_mask + a.norm_blocks;
  a.part_cls = a.part_nw + a.norm_blocks; a.part_reg = a.part_cls + npix;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_norm_kernel, dim3(a.norm_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, a.part_mask, a.part_nw, (long)a.norm_blocks, 1.0f, stats);
  hipLaunchKernelGGL(loss_pixel_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, a.part_cls, a.part_reg, npix, 0.0f, stats + 2);
  return check_launch("rpn_loss");
}

// ---- backward of the head towers (k_convbwd.h) ------------------------------------------------------------------------------
static bool nhwc16_ok(int cs, int co, int C) { return cs > 0 && cs % 8 == 0 && co >= 0 && co % 8 == 0 && co + C <= cs; }
static bool bhw_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1; }
int rd_relu_affine_bwd(const void* g, int g_cstride, int g_coff, const void* y, int y_cstride, int y_coff, const float* scale, void* dz,
                       int dz_cstride, int dz_coff, int B, int H, int W, int C, int dtype, void* stream) {
  RD_REQUIRE(g && dz, RD_EINVAL, "relu_affine_bwd: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "relu_affine_bwd: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(bhw_ok(B, H, W) && C >= 8 && C % 8 == 0, RD_ESHAPE, "relu_affine_bwd: B %d, H %d, W %d, C %d (a multiple of 8)", B, H, W, C);
  RD_REQUIRE(nhwc16_ok(g_cstride, g_coff, C) && nhwc16_ok(dz_cstride, dz_coff, C) && (!y || nhwc16_ok(y_cstride, y_coff, C)), RD_ESHAPE,
             "relu_affine_bwd: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)g | (uintptr_t)y | (uintptr_t)dz) % 16 == 0, RD_EINVAL, "relu_affine_bwd: the tensors must be 16-byte aligned");
  const long npix = (long)B * H * W, nthreads = npix * (C / 8);
  RD_REQUIRE((nthreads + 255) / 256 <= 0x7fffffffL, RD_ESHAPE, "relu_affine_bwd: %ld pixels", npix);
  const dim3 grid((unsigned)((nthreads + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  RD_LAUNCH_H16(dtype, (relu_affine_bwd_kernel<DT>), grid, dim3(256), st, (const unsigned short*)g, g_cstride, g_coff, (const unsigned short*)y,
                y_cstride, y_coff, scale, (unsigned short*)dz, dz_cstride, dz_coff, npix, C);
  return check_launch("relu_affine_bwd");
}

size_t rd_conv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int cin, int cout, int split) {
  return bhw_ok(B, H, W) && split >= 0 && bw_weight_shape_ok(cin, cout) ? bw_weight_ws_bytes(B, H, W, cin, cout, split) : 0;
}
int rd_conv3x3_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                          int W, int cin, int cout, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(x && dz && dW && ws, RD_EINVAL, "conv3x3_bwd_weight: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv3x3_bwd_weight: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "conv3x3_bwd_weight: split %d (0: the library's choice)", split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "conv3x3_bwd_weight: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(bw_weight_shape_ok(cin, cout), RD_ESHAPE, "conv3x3_bwd_weight: cin %d, cout %d (each 64 or 128; stride 1, pad 1)", cin, cout);
  RD_REQUIRE(nhwc16_ok(x_cstride, x_coff, cin) && nhwc16_ok(dz_cstride, dz_coff, cout), RD_ESHAPE,
             "conv3x3_bwd_weight: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dz) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)dW) % 4 == 0, RD_EINVAL,
             "conv3x3_bwd_weight: x and dz must be 16-byte aligned, dW and the workspace 4-byte aligned");
  const size_t need = bw_weight_ws_bytes(B, H, W, cin, cout, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "conv3x3_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  const long S = bw_split(B, H, W, cout, split);
  RD_REQUIRE(S <= 0x7fffffffL, RD_ESHAPE, "conv3x3_bwd_weight: split %ld", S);
  BwdWArgs a;
  a.x = (const unsigned short*)x; a.dz = (const unsigned short*)dz;
  a.x_cs = x_cstride; a.x_co = x_coff; a.dz_cs = dz_cstride; a.dz_co = dz_coff;
  a.B = B; a.H = H; a.W = W; a.nwt = (W + BW_PT - 1) / BW_PT; a.nhs = (H + BW_RH - 1) / BW_RH;
  a.nchunks = bw_chunks(B, H, W);
  a.part = (float*)ws;
  a.Wz = W;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S, 3, cout / BW_COB);
  if (cin == 128 && cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 128, 128>), grid, dim3(256), st, a);
  else if (cin == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 128, 64>), grid, dim3(256), st, a);
  else if (cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 128>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 64>), grid, dim3(256), st, a);
  hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((9 * cout * cin + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cout, cin, dW, 9);
  return check_launch("conv3x3_bwd_weight");
}
// ---- backward of the Meta-Kernel unit (k_metabwd.h) ---------------------------------------------------------------------------------
size_t rd_meta_bwd_packed_bytes(int dtype) { return is_h16(dtype) ? meta_bwd_layout().total : 0; }
int rd_pack_meta_bwd_host(const float* w0, const float* b0, const float* w1, const float* b1, const float* s1, const float* t1,
                          const float* agg, const float* s2, const float* t2, int dtype, void* packed_host) {
  RD_REQUIRE(w0 && b0 && w1 && b1 && s1 && t1 && agg && s2 && t2 && packed_host, RD_EINVAL, "pack_meta_bwd: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_meta_bwd: dtype %d (RD_BF16 or RD_F16)", dtype);
  pack_meta_bwd(w0, b0, w1, b1, s1, t1, agg, dtype, packed_host);   // (s2, t2 act behind z: rd_relu_affine_bwd)
  return RD_OK;
}
static int meta_bwd_checks(const char* what, const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff,
                           const float* coord, const void* packed, int B, int H, int W, int dtype, MetaBwdArgs& a) {
  RD_REQUIRE(dz && data && coord && packed, RD_EINVAL, "%s: null pointer", what);
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "%s: dtype %d (RD_BF16 or RD_F16)", what, dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "%s: B %d, H %d, W %d", what, B, H, W);
  RD_REQUIRE(nhwc16_ok(dz_cstride, dz_coff, 64) && nhwc16_ok(d_cstride, d_coff, 64), RD_ESHAPE,
             "%s: channel strides and offsets are multiples of 8 with coff + 64 <= cstride", what);
  RD_REQUIRE(((uintptr_t)dz | (uintptr_t)data | (uintptr_t)packed) % 16 == 0 && (uintptr_t)coord % 4 == 0, RD_EINVAL,
             "%s: dz, data and the packed block must be 16-byte aligned, coord 4-byte aligned", what);
  a.dz = (const unsigned short*)dz; a.z_cs = dz_cstride; a.z_co = dz_coff;
  a.data = (const unsigned short*)data; a.d_cs = d_cstride; a.d_co = d_coff;
  a.coord = coord; a.packed = (const unsigned char*)packed;
  a.res = nullptr; a.r_cs = a.r_co = 0; a.ddata = nullptr; a.g_cs = a.g_co = 0; a.part = nullptr;
  a.B = B; a.H = H; a.W = W;
  return RD_OK;
}
int rd_meta_kernel_bwd_data(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                            const void* packed_bwd, const void* residual, int r_cstride, int r_coff, void* ddata, int g_cstride, int g_coff,
                            int B, int H, int W, int dtype, void* stream) {
  MetaBwdArgs a;
  const int rc = meta_bwd_checks("meta_kernel_bwd_data", dz, dz_cstride, dz_coff, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W, dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(ddata, RD_EINVAL, "meta_kernel_bwd_data: null pointer");
  RD_REQUIRE(nhwc16_ok(g_cstride, g_coff, 64) && (!residual || nhwc16_ok(r_cstride, r_coff, 64)), RD_ESHAPE,
             "meta_kernel_bwd_data: channel strides and offsets are multiples of 8 with coff + 64 <= cstride");
  RD_REQUIRE(((uintptr_t)ddata | (uintptr_t)residual) % 16 == 0, RD_EINVAL, "meta_kernel_bwd_data: ddata and residual must be 16-byte aligned");
  a.res = (const unsigned short*)residual; a.r_cs = r_cstride; a.r_co = r_coff;
  a.ddata = (unsigned short*)ddata; a.g_cs = g_cstride; a.g_co = g_coff;
  return launch_meta_bwd_data(a, dtype, (hipStream_t)stream);
}
size_t rd_meta_kernel_bwd_workspace_bytes(int B, int H, int W, int split) { return bhw_ok(B, H, W) && split >= 0 ? mb_ws_bytes(B, H, W, split) : 0; }
int rd_meta_kernel_bwd_params(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                              const void* packed_bwd, float* dA, float* dW1, float* db1, float* dW0, float* db0, float* dt1, float* dq1, int B,
                              int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  MetaBwdArgs a;
  const int rc = meta_bwd_checks("meta_kernel_bwd_params", dz, dz_cstride, dz_coff, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W, dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(dA && dW1 && db1 && dW0 && db0 && dt1 && dq1 && ws, RD_EINVAL, "meta_kernel_bwd_params: null pointer");
  RD_REQUIRE(split >= 0, RD_EINVAL, "meta_kernel_bwd_params: split %d (0: the library's choice)", split);
  RD_REQUIRE(((uintptr_t)dA | (uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)dW0 | (uintptr_t)db0 | (uintptr_t)dt1 | (uintptr_t)dq1 | (uintptr_t)ws) % 4 == 0,
             RD_EINVAL, "meta_kernel_bwd_params: the gradients and the workspace must be 4-byte aligned");
  const size_t need = mb_ws_bytes(B, H, W, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "meta_kernel_bwd_params: workspace %zu < %zu bytes", ws_bytes, need);
  a.part = (float*)ws;
  const MetaBwdOut out{dA, dW1, db1, dW0, db0, dt1, dq1};
  return launch_meta_bwd_params(a, out, split, dtype, (hipStream_t)stream);
}
// ---- the Meta-Kernel unit in training mode (k_metatrain.h) ------------------------------------------------------------------------------
// data, coord, the backward block, shape and type of every training entry; dz where the entry reads it
static int meta_train_checks(const char* what, bool has_dz, const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride,
                             int d_coff, const float* coord, const void* packed, int B, int H, int W, int dtype, MetaTrainArgs& a) {
  RD_REQUIRE((!has_dz || dz) && data && coord && packed, RD_EINVAL, "%s: null pointer", what);
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "%s: dtype %d (RD_BF16 or RD_F16)", what, dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "%s: B %d, H %d, W %d", what, B, H, W);
  RD_REQUIRE((!has_dz || nhwc16_ok(dz_cstride, dz_coff, 64)) && nhwc16_ok(d_cstride, d_coff, 64), RD_ESHAPE,
             "%s: channel strides and offsets are multiples of 8 with coff + 64 <= cstride", what);
  RD_REQUIRE(((uintptr_t)dz | (uintptr_t)data | (uintptr_t)packed) % 16 == 0 && (uintptr_t)coord % 4 == 0, RD_EINVAL,
             "%s: the tensors and the packed block must be 16-byte aligned, coord 4-byte aligned", what);
  a = MetaTrainArgs{};
  a.dz = (const unsigned short*)dz; a.z_cs = dz_cstride; a.z_co = dz_coff;
  a.data = (const unsigned short*)data; a.d_cs = d_cstride; a.d_co = d_coff;
  a.coord = coord; a.packed = (const unsigned char*)packed;
  a.B = B; a.H = H; a.W = W;
  return RD_OK;
}
static bool f32_ok(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!p || (uintptr_t)p % 4 != 0) return false;
  return true;
}
size_t rd_meta_kernel_stats_workspace_bytes(int B, int H, int W, int split) {
  return bhw_ok(B, H, W) && split >= 0 ? mt_stats_ws_bytes(B, H, W, split) : 0;
}
int rd_meta_kernel_stats(const void* data, int d_cstride, int d_coff, const float* coord_nchw, const void* packed_bwd, float* mean1,
                         float* var1, int B, int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  MetaTrainArgs a;
  const int rc = meta_train_checks("meta_kernel_stats", false, nullptr, 0, 0, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W, dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(f32_ok({mean1, var1, ws}), RD_EINVAL, "meta_kernel_stats: mean1, var1 and the workspace: non-null, 4-byte aligned");
  RD_REQUIRE(split >= 0, RD_EINVAL, "meta_kernel_stats: split %d (0: the library's choice)", split);
  const size_t need = mt_stats_ws_bytes(B, H, W, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "meta_kernel_stats: workspace %zu < %zu bytes", ws_bytes, need);
  a.part = (float*)ws;
  return launch_meta_stats(a, mean1, var1, split, dtype, (hipStream_t)stream);
}
int rd_meta_kernel_fwd_train(const void* data, int d_cstride, int d_coff, const float* coord_nchw, const void* packed_fwd,
                             const void* packed_bwd, const float* a1, const float* bb1, void* z, int z_cstride, int z_coff, int B, int H,
                             int W, int dtype, void* stream) {
  MetaTrainArgs a;
  const int rc = meta_train_checks("meta_kernel_fwd_train", false, nullptr, 0, 0, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W, dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(packed_fwd && z && f32_ok({a1, bb1}) && ((uintptr_t)packed_fwd | (uintptr_t)z) % 16 == 0, RD_EINVAL,
             "meta_kernel_fwd_train: packed_fwd, z (16-byte aligned), a1, bb1 (4-byte aligned): non-null");
  RD_REQUIRE(nhwc16_ok(z_cstride, z_coff, 64), RD_ESHAPE, "meta_kernel_fwd_train: channel strides and offsets are multiples of 8 with coff + 64 <= cstride");
  a.packed_fwd = (const unsigned char*)packed_fwd; a.a1 = a1; a.bb1 = bb1;
  a.ddata = (unsigned short*)z; a.g_cs = z_cstride; a.g_co = z_coff;
  return launch_meta_fwd_train(a, dtype, (hipStream_t)stream);
}
size_t rd_meta_kernel_bwd_train_workspace_bytes(int B, int H, int W, int split) {
  return bhw_ok(B, H, W) && split >= 0 ? mt_bwd_ws_bytes(B, H, W, split) : 0;
}
int rd_meta_kernel_bwd_sums(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff, const float* coord_nchw,
                            const void* packed_bwd, const float* a1, const float* bb1, const float* mean1, const float* rstd1, float* dA,
                            float* dbeta1, float* dgamma1, float* c1, float* c2, int B, int H, int W, int split, int dtype, void* ws,
                            size_t ws_bytes, void* stream) {
  MetaTrainArgs a;
  const int rc = meta_train_checks("meta_kernel_bwd_sums", true, dz, dz_cstride, dz_coff, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W, dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(f32_ok({a1, bb1, mean1, rstd1, dA, dbeta1, dgamma1, c1, c2, ws}), RD_EINVAL,
             "meta_kernel_bwd_sums: the tables, the gradients and the workspace: non-null, 4-byte aligned");
  RD_REQUIRE(split >= 0, RD_EINVAL, "meta_kernel_bwd_sums: split %d (0: the library's choice)", split);
  const size_t need = mt_bwd_ws_bytes(B, H, W, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "meta_kernel_bwd_sums: workspace %zu < %zu bytes", ws_bytes, need);
  a.a1 = a1; a.bb1 = bb1; a.mean1 = mean1; a.rstd1 = rstd1; a.part = (float*)ws;
  const MetaTrainSumsOut out{dA, dbeta1, dgamma1, c1, c2};
  return launch_meta_train_sums(a, out, split, dtype, (hipStream_t)stream);
}
int rd_meta_kernel_bwd_params_train(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff,
                                    const float* coord_nchw, const void* packed_bwd, const float* a1, const float* bb1, const float* mean1,
                                    const float* rstd1, const float* c1, const float* c2, float* dW1, float* db1, float* dW0, float* db0,
                                    int B, int H, int W, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  MetaTrainArgs a;
  const int rc = meta_train_checks("meta_kernel_bwd_params_train", true, dz, dz_cstride, dz_coff, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W,
                                   dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(f32_ok({a1, bb1, mean1, rstd1, c1, c2, dW1, db1, dW0, db0, ws}), RD_EINVAL,
             "meta_kernel_bwd_params_train: the tables, the gradients and the workspace: non-null, 4-byte aligned");
  RD_REQUIRE(split >= 0, RD_EINVAL, "meta_kernel_bwd_params_train: split %d (0: the library's choice)", split);
  const size_t need = mt_bwd_ws_bytes(B, H, W, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "meta_kernel_bwd_params_train: workspace %zu < %zu bytes", ws_bytes, need);
  a.a1 = a1; a.bb1 = bb1; a.mean1 = mean1; a.rstd1 = rstd1; a.c1 = c1; a.c2 = c2; a.part = (float*)ws;
  const MetaTrainParamsOut out{dW1, db1, dW0, db0};
  return launch_meta_train_params(a, out, split, dtype, (hipStream_t)stream);
}
int rd_meta_kernel_bwd_data_train(const void* dz, int dz_cstride, int dz_coff, const void* data, int d_cstride, int d_coff,
                                  const float* coord_nchw, const void* packed_bwd, const float* a1, const float* bb1, const float* mean1,
                                  const float* rstd1, const float* c1, const float* c2, const void* residual, int r_cstride, int r_coff,
                                  void* ddata, int g_cstride, int g_coff, int B, int H, int W, int dtype, void* stream) {
  MetaTrainArgs a;
  const int rc = meta_train_checks("meta_kernel_bwd_data_train", true, dz, dz_cstride, dz_coff, data, d_cstride, d_coff, coord_nchw, packed_bwd, B, H, W,
                                   dtype, a);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(ddata && f32_ok({a1, bb1, mean1, rstd1, c1, c2}), RD_EINVAL, "meta_kernel_bwd_data_train: ddata and the tables (4-byte aligned): non-null");
  RD_REQUIRE(nhwc16_ok(g_cstride, g_coff, 64) && (!residual || nhwc16_ok(r_cstride, r_coff, 64)), RD_ESHAPE,
             "meta_kernel_bwd_data_train: channel strides and offsets are multiples of 8 with coff + 64 <= cstride");
  RD_REQUIRE(((uintptr_t)ddata | (uintptr_t)residual) % 16 == 0, RD_EINVAL, "meta_kernel_bwd_data_train: ddata and residual must be 16-byte aligned");
  a.a1 = a1; a.bb1 = bb1; a.mean1 = mean1; a.rstd1 = rstd1; a.c1 = c1; a.c2 = c2;
  a.res = (const unsigned short*)residual; a.r_cs = r_cstride; a.r_co = r_coff;
  a.ddata = (unsigned short*)ddata; a.g_cs = g_cstride; a.g_co = g_coff;
  return launch_meta_train_data(a, dtype, (hipStream_t)stream);
}
int rd_pack_meta_dev(const float* w0, const float* b0, const float* w1, const float* b1, const float* agg, void* packed_fwd,
                     void* packed_bwd, int dtype, void* stream) {
  RD_REQUIRE(f32_ok({w0, b0, w1, b1, agg}) && packed_fwd && packed_bwd, RD_EINVAL, "pack_meta_dev: null or misaligned pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_meta_dev: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(((uintptr_t)packed_fwd | (uintptr_t)packed_bwd) % 16 == 0, RD_EINVAL, "pack_meta_dev: the packed blocks must be 16-byte aligned");
  const MetaPackDevArgs a{w0, b0, w1, b1, agg, (unsigned char*)packed_fwd, (unsigned char*)packed_bwd};
  return launch_meta_pack_dev(a, dtype, (hipStream_t)stream);
}
// the same with a stride: stride_w 1 forwards to the entry above (its bytes, its partial count, its workspace); stride_w 2 is the weight
// gradient of a 3x3 stride-(1,2) pad-1 conv, x (B, H, Win) against dz (B, H, Win / 2): chunks and the split are counted on the dz grid
static bool bw_ex_shape_ok(int B, int H, int Win, int cin, int cout, int stride_w) {
  return bhw_ok(B, H, Win) && bw_weight_shape_ok(cin, cout) && (stride_w == 1 || (stride_w == 2 && Win % 2 == 0));
}
size_t rd_conv3x3_bwd_weight_ex_workspace_bytes(int B, int H, int Win, int cin, int cout, int stride_w, int split) {
  return split >= 0 && bw_ex_shape_ok(B, H, Win, cin, cout, stride_w) ? bw_weight_ws_bytes(B, H, Win / stride_w, cin, cout, split) : 0;
}
int rd_conv3x3_bwd_weight_ex(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                             int Win, int cin, int cout, int stride_w, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(x && dz && dW && ws, RD_EINVAL, "conv3x3_bwd_weight_ex: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv3x3_bwd_weight_ex: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "conv3x3_bwd_weight_ex: split %d (0: the library's choice)", split);
  RD_REQUIRE(stride_w == 1 || stride_w == 2, RD_ESHAPE, "conv3x3_bwd_weight_ex: stride_w %d (1 or 2)", stride_w);
  RD_REQUIRE(bhw_ok(B, H, Win), RD_ESHAPE, "conv3x3_bwd_weight_ex: B %d, H %d, Win %d", B, H, Win);
  RD_REQUIRE(Win % stride_w == 0, RD_ESHAPE, "conv3x3_bwd_weight_ex: Win %d with stride_w 2 (an even width)", Win);
  RD_REQUIRE(bw_weight_shape_ok(cin, cout), RD_ESHAPE, "conv3x3_bwd_weight_ex: cin %d, cout %d (each 64 or 128; pad 1)", cin, cout);
  RD_REQUIRE(nhwc16_ok(x_cstride, x_coff, cin) && nhwc16_ok(dz_cstride, dz_coff, cout), RD_ESHAPE,
             "conv3x3_bwd_weight_ex: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dz) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)dW) % 4 == 0, RD_EINVAL,
             "conv3x3_bwd_weight_ex: x and dz must be 16-byte aligned, dW and the workspace 4-byte aligned");
  const int Wo = Win / stride_w;
  const size_t need = bw_weight_ws_bytes(B, H, Wo, cin, cout, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "conv3x3_bwd_weight_ex: workspace %zu < %zu bytes", ws_bytes, need);
  const long S = bw_split(B, H, Wo, cout, split);
  RD_REQUIRE(S <= 0x7fffffffL, RD_ESHAPE, "conv3x3_bwd_weight_ex: split %ld", S);
  if (stride_w == 1)
    return rd_conv3x3_bwd_weight(x, x_cstride, x_coff, dz, dz_cstride, dz_coff, dW, B, H, Win, cin, cout, split, dtype, ws, ws_bytes, stream);
  BwdWArgs a;
  a.x = (const unsigned short*)x; a.dz = (const unsigned short*)dz;
  a.x_cs = x_cstride; a.x_co = x_coff; a.dz_cs = dz_cstride; a.dz_co = dz_coff;
  a.B = B; a.H = H; a.W = Win; a.Wz = Wo; a.nwt = (Wo + BW_PT - 1) / BW_PT; a.nhs = (H + BW_RH - 1) / BW_RH;
  a.nchunks = bw_chunks(B, H, Wo);
  a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S, 3, cout / BW_COB);
  if (cin == 128 && cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 128, 128, 2>), grid, dim3(256), st, a);
  else if (cin == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 128, 64, 2>), grid, dim3(256), st, a);
  else if (cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 128, 2>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 64, 2>), grid, dim3(256), st, a);
  hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((9 * cout * cin + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cout, cin, dW, 9);
  return check_launch("conv3x3_bwd_weight_ex");
}
// the weight gradient of a transposed conv (k_convbwd.h): the same kernel with the deconv input as the narrow tensor and dz as the wide one
size_t rd_deconv_bwd_weight_workspace_bytes(int B, int H, int Win, int cin, int cout, int kw, int stride_w, int pad_w, int split) {
  return split >= 0 && bhw_ok(B, H, Win) && bw_deconv_form_ok(kw, stride_w, pad_w) && bw_deconv_shape_ok(cin, cout, kw)
             ? bw_deconv_ws_bytes(B, H, Win, cin, cout, kw, split) : 0;
}
int rd_deconv_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                         int Win, int cin, int cout, int kw, int stride_w, int pad_w, int split, int dtype, void* ws, size_t ws_bytes,
                         void* stream) {
  RD_REQUIRE(x && dz && dW && ws, RD_EINVAL, "deconv_bwd_weight: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "deconv_bwd_weight: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "deconv_bwd_weight: split %d (0: the library's choice)", split);
  RD_REQUIRE(bw_deconv_form_ok(kw, stride_w, pad_w), RD_ESHAPE,
             "deconv_bwd_weight: kernel (3,%d), stride (1,%d), pad (1,%d) -- (3,4) / 2 / 1 or (3,8) / 4 / 2", kw, stride_w, pad_w);
  RD_REQUIRE(bhw_ok(B, H, Win) && (long)Win * stride_w <= 0x7fffffffL, RD_ESHAPE, "deconv_bwd_weight: B %d, H %d, Win %d", B, H, Win);
  RD_REQUIRE(bw_deconv_shape_ok(cin, cout, kw), RD_ESHAPE,
             "deconv_bwd_weight: %d -> %d channels with kernel (3,%d) -- (3,8): 128 -> 128 or 128 -> 64; (3,4): 128 -> 64 or 64 -> 64", cin, cout, kw);
  RD_REQUIRE(nhwc16_ok(x_cstride, x_coff, cin) && nhwc16_ok(dz_cstride, dz_coff, cout), RD_ESHAPE,
             "deconv_bwd_weight: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dz) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)dW) % 4 == 0, RD_EINVAL,
             "deconv_bwd_weight: x and dz must be 16-byte aligned, dW and the workspace 4-byte aligned");
  const size_t need = bw_deconv_ws_bytes(B, H, Win, cin, cout, kw, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "deconv_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  const long S = bw_deconv_split(B, H, Win, cin, kw, split);
  RD_REQUIRE(S <= 0x7fffffffL, RD_ESHAPE, "deconv_bwd_weight: split %ld", S);
  BwdWArgs a;   // the kernel's dz is the narrow tensor (the deconv input), its x the wide one (the gradient at the deconv output)
  a.x = (const unsigned short*)dz; a.dz = (const unsigned short*)x;
  a.x_cs = dz_cstride; a.x_co = dz_coff; a.dz_cs = x_cstride; a.dz_co = x_coff;
  a.B = B; a.H = H; a.W = Win * stride_w; a.Wz = Win; a.nwt = (Win + BW_PT - 1) / BW_PT; a.nhs = (H + BW_RH - 1) / BW_RH;
  a.nchunks = bw_chunks(B, H, Win);
  a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S, kw, cin / BW_COB);
  if (kw == 8 && cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 128, 128, 4, 8, 2>), grid, dim3(256), st, a);
  else if (kw == 8) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 128, 4, 8, 2>), grid, dim3(256), st, a);
  else if (cin == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 128, 2, 4, 1>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 64, 2, 4, 1>), grid, dim3(256), st, a);
  hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((3 * kw * cin * cout + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cin, cout, dW,
                     3 * kw);
  return check_launch("deconv_bwd_weight");
}

size_t rd_conv1x1_bwd_weight_workspace_bytes(int B, int H, int W, int cin, int cout, int split) {
  return bhw_ok(B, H, W) && split >= 0 && bw_weight_shape_ok(cin, cout) ? bw1_weight_ws_bytes(B, H, W, cin, cout, split) : 0;
}
int rd_conv1x1_bwd_weight(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H,
                          int W, int cin, int cout, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(x && dz && dW && ws, RD_EINVAL, "conv1x1_bwd_weight: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "conv1x1_bwd_weight: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "conv1x1_bwd_weight: split %d (0: the library's choice)", split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "conv1x1_bwd_weight: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(bw_weight_shape_ok(cin, cout), RD_ESHAPE, "conv1x1_bwd_weight: cin %d, cout %d (each 64 or 128; stride 1)", cin, cout);
  RD_REQUIRE(nhwc16_ok(x_cstride, x_coff, cin) && nhwc16_ok(dz_cstride, dz_coff, cout), RD_ESHAPE,
             "conv1x1_bwd_weight: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dz) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)dW) % 4 == 0, RD_EINVAL,
             "conv1x1_bwd_weight: x and dz must be 16-byte aligned, dW and the workspace 4-byte aligned");
  const size_t need = bw1_weight_ws_bytes(B, H, W, cin, cout, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "conv1x1_bwd_weight: workspace %zu < %zu bytes", ws_bytes, need);
  const long S = bw1_split(B, H, W, split);
  RD_REQUIRE(S <= 0x7fffffffL, RD_ESHAPE, "conv1x1_bwd_weight: split %ld", S);
  BwdW1Args a;
  a.x = (const unsigned short*)x; a.dz = (const unsigned short*)dz;
  a.x_cs = x_cstride; a.x_co = x_coff; a.dz_cs = dz_cstride; a.dz_co = dz_coff;
  a.npix = (long)B * H * W; a.nchunks = bw1_chunks(B, H, W);
  a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S);
  if (cin == 128 && cout == 128) RD_LAUNCH_H16(dtype, (conv1_bwd_weight_kernel<DT, 128, 128>), grid, dim3(256), st, a);
  else if (cin == 128) RD_LAUNCH_H16(dtype, (conv1_bwd_weight_kernel<DT, 128, 64>), grid, dim3(256), st, a);
  else if (cout == 128) RD_LAUNCH_H16(dtype, (conv1_bwd_weight_kernel<DT, 64, 128>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv1_bwd_weight_kernel<DT, 64, 64>), grid, dim3(256), st, a);
  hipLaunchKernelGGL(bwd1_weight_reduce_kernel, dim3((cout * cin + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cout * cin, dW);
  return check_launch("conv1x1_bwd_weight");
}

// ---- weight gradient of the convs that read the range image (k_convbwd_narrow.h) ----------------------------------------------------------
static bool nw_slot_ok(int cs, int co) { return cs > 0 && cs % 8 == 0 && co >= 0 && co % 8 == 0 && co + NW_SLOT <= cs; }
// the checks of rd_conv_bwd_weight_narrow, all of them before any launch (the concat call runs them for its x2 half first)
static int nw_check(const char* what, const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, const float* dW,
                    int dw_cin_stride, int dw_cin_off, int B, int H, int W, int cin, int cout, int ksize, int split, int dtype, const void* ws,
                    size_t ws_bytes) {
  RD_REQUIRE(x && dz && dW && ws, RD_EINVAL, "%s: null pointer", what);
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "%s: dtype %d (RD_BF16 or RD_F16)", what, dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "%s: split %d (0: the library's choice)", what, split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "%s: B %d, H %d, W %d", what, B, H, W);
  RD_REQUIRE(ksize == 1 || ksize == 3, RD_ESHAPE, "%s: ksize %d (1 or 3)", what, ksize);
  RD_REQUIRE(nw_shape_ok(cin, cout, ksize), RD_ESHAPE, "%s: cin %d (1 .. 16), cout %d (64 or 128)", what, cin, cout);
  RD_REQUIRE(nw_slot_ok(x_cstride, x_coff) && nhwc16_ok(dz_cstride, dz_coff, cout), RD_ESHAPE,
             "%s: channel strides and offsets are multiples of 8 with x_coff + 16 <= x_cstride (the whole slot is read) and dz_coff + cout <= "
             "dz_cstride", what);
  RD_REQUIRE(dw_cin_off >= 0 && dw_cin_off + cin <= dw_cin_stride, RD_ESHAPE, "%s: dW channels [%d, %d) of %d", what, dw_cin_off, dw_cin_off + cin,
             dw_cin_stride);
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dz) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)dW) % 4 == 0, RD_EINVAL,
             "%s: x and dz must be 16-byte aligned, dW and the workspace 4-byte aligned", what);
  const size_t need = nw_ws_bytes(B, H, W, cin, cout, ksize, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
  RD_REQUIRE(nw_split(B, H, W, split) <= 0x7fffffffL, RD_ESHAPE, "%s: split %ld", what, nw_split(B, H, W, split));
  return RD_OK;
}
static void nw_launch(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride,
                      int dw_cin_off, int B, int H, int W, int cin, int cout, int ksize, int split, int dtype, void* ws, hipStream_t st) {
  const long S = nw_split(B, H, W, split);
  NarrowWArgs a;
  a.x = (const unsigned short*)x; a.dz = (const unsigned short*)dz;
  a.x_cs = x_cstride; a.x_co = x_coff; a.dz_cs = dz_cstride; a.dz_co = dz_coff;
  a.B = B; a.H = H; a.W = W; a.nwt = (W + NW_PT - 1) / NW_PT; a.nhs = (H + NW_RH - 1) / NW_RH; a.cin = cin;
  a.nchunks = nw_chunks(B, H, W);
  a.part = (float*)ws;
  const dim3 grid((unsigned)S);
  if (ksize == 3 && cout == 128) RD_LAUNCH_H16(dtype, (conv_bwd_weight_narrow_kernel<DT, 128, 3>), grid, dim3(256), st, a);
  else if (ksize == 3) RD_LAUNCH_H16(dtype, (conv_bwd_weight_narrow_kernel<DT, 64, 3>), grid, dim3(256), st, a);
  else if (cout == 128) RD_LAUNCH_H16(dtype, (conv_bwd_weight_narrow_kernel<DT, 128, 1>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv_bwd_weight_narrow_kernel<DT, 64, 1>), grid, dim3(256), st, a);
  const int nt = ksize * ksize;
  hipLaunchKernelGGL(bwd_weight_reduce_strided_kernel, dim3((nt * cout * cin + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cout, cin,
                     dW, nt, dw_cin_stride, dw_cin_off);
}
size_t rd_conv_bwd_weight_narrow_workspace_bytes(int B, int H, int W, int cin, int cout, int ksize, int split) {
  return bhw_ok(B, H, W) && split >= 0 && nw_shape_ok(cin, cout, ksize) ? nw_ws_bytes(B, H, W, cin, cout, ksize, split) : 0;
}
int rd_conv_bwd_weight_narrow(const void* x, int x_cstride, int x_coff, const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride,
                              int dw_cin_off, int B, int H, int W, int cin, int cout, int ksize, int split, int dtype, void* ws, size_t ws_bytes,
                              void* stream) {
  const int rc = nw_check("conv_bwd_weight_narrow", x, x_cstride, x_coff, dz, dz_cstride, dz_coff, dW, dw_cin_stride, dw_cin_off, B, H, W, cin, cout,
                          ksize, split, dtype, ws, ws_bytes);
  if (rc != RD_OK) return rc;
  nw_launch(x, x_cstride, x_coff, dz, dz_cstride, dz_coff, dW, dw_cin_stride, dw_cin_off, B, H, W, cin, cout, ksize, split, dtype, ws,
            (hipStream_t)stream);
  return check_launch("conv_bwd_weight_narrow");
}

// The weight gradient of the concat conv [x1 | x2] -> cout (the level-0 conv_0): channels [0, cin1) are rd_conv3x3_bwd_weight's kernel on
// (x1, dz) with its reduce writing at the channel stride cin1 + cin2, channels [cin1, cin1 + cin2) the narrow kernel on (x2, dz).  The
// workspace holds the partial images of the first, then those of the second.
size_t rd_conv3x3_bwd_weight_cat_workspace_bytes(int B, int H, int W, int cin1, int cin2, int cout, int split) {
  if (!(bhw_ok(B, H, W) && split >= 0 && cin1 == 64 && nw_shape_ok(cin2, cout, 3))) return 0;
  return bw_weight_ws_bytes(B, H, W, cin1, cout, split) + nw_ws_bytes(B, H, W, cin2, cout, 3, split);
}
static int bw_cat_run(const char* what, const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff,
                      int cin2, const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride, int B, int H, int W, int cout, int split,
                      int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(x1 && x2 && dz && dW && ws, RD_EINVAL, "%s: null pointer", what);
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "%s: dtype %d (RD_BF16 or RD_F16)", what, dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "%s: split %d (0: the library's choice)", what, split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "%s: B %d, H %d, W %d", what, B, H, W);
  RD_REQUIRE(cin1 == 64, RD_ESHAPE, "%s: cin1 %d (64: the agg3 feature map)", what, cin1);
  RD_REQUIRE(nw_shape_ok(cin2, cout, 3), RD_ESHAPE, "%s: cin2 %d (1 .. 16), cout %d (64 or 128)", what, cin2, cout);
  const size_t need1 = bw_weight_ws_bytes(B, H, W, cin1, cout, split), need = need1 + nw_ws_bytes(B, H, W, cin2, cout, 3, split);
  RD_REQUIRE(nhwc16_ok(x1_cstride, x1_coff, cin1), RD_ESHAPE, "%s: x1 channel stride and offset are multiples of 8 with coff + 64 <= cstride", what);
  RD_REQUIRE((uintptr_t)x1 % 16 == 0, RD_EINVAL, "%s: x1 must be 16-byte aligned", what);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, need);
  void* ws2 = (char*)ws + need1;
  const int rc = nw_check(what, x2, x2_cstride, x2_coff, dz, dz_cstride, dz_coff, dW, dw_cin_stride, cin1, B, H, W, cin2, cout, 3, split, dtype, ws2,
                          ws_bytes - need1);
  if (rc != RD_OK) return rc;
  const long S = bw_split(B, H, W, cout, split);
  RD_REQUIRE(S <= 0x7fffffffL, RD_ESHAPE, "%s: split %ld", what, S);
  BwdWArgs a;
  a.x = (const unsigned short*)x1; a.dz = (const unsigned short*)dz;
  a.x_cs = x1_cstride; a.x_co = x1_coff; a.dz_cs = dz_cstride; a.dz_co = dz_coff;
  a.B = B; a.H = H; a.W = W; a.nwt = (W + BW_PT - 1) / BW_PT; a.nhs = (H + BW_RH - 1) / BW_RH;
  a.nchunks = bw_chunks(B, H, W);
  a.part = (float*)ws;
  a.Wz = W;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)S, 3, cout / BW_COB);
  if (cout == 128) RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 128>), grid, dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (conv3_bwd_weight_kernel<DT, 64, 64>), grid, dim3(256), st, a);
  hipLaunchKernelGGL(bwd_weight_reduce_strided_kernel, dim3((9 * cout * cin1 + 255) / 256), dim3(256), 0, st, (const float*)ws, (int)S, cout, cin1,
                     dW, 9, dw_cin_stride, 0);
  nw_launch(x2, x2_cstride, x2_coff, dz, dz_cstride, dz_coff, dW, dw_cin_stride, cin1, B, H, W, cin2, cout, 3, split, dtype, ws2, st);
  return check_launch(what);
}
int rd_conv3x3_bwd_weight_cat(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                              const void* dz, int dz_cstride, int dz_coff, float* dW, int B, int H, int W, int cout, int split, int dtype,
                              void* ws, size_t ws_bytes, void* stream) {
  return bw_cat_run("conv3x3_bwd_weight_cat", x1, x1_cstride, x1_coff, cin1, x2, x2_cstride, x2_coff, cin2, dz, dz_cstride, dz_coff, dW, cin1 + cin2, B,
                    H, W, cout, split, dtype, ws, ws_bytes, stream);
}
// the same into a gradient whose channel stride is wider than cin1 + cin2 (a master padded to the width the forward reads): channels
// [cin1 + cin2, dw_cin_stride) are never written
int rd_conv3x3_bwd_weight_cat_padded(const void* x1, int x1_cstride, int x1_coff, int cin1, const void* x2, int x2_cstride, int x2_coff, int cin2,
                                     const void* dz, int dz_cstride, int dz_coff, float* dW, int dw_cin_stride, int B, int H, int W, int cout,
                                     int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  return bw_cat_run("conv3x3_bwd_weight_cat_padded", x1, x1_cstride, x1_coff, cin1, x2, x2_cstride, x2_coff, cin2, dz, dz_cstride, dz_coff, dW,
                    dw_cin_stride, B, H, W, cout, split, dtype, ws, ws_bytes, stream);
}

size_t rd_head_out_bwd_workspace_bytes(int B, int H, int W, int cin, int nout) {
  return bhw_ok(B, H, W) && (cin == 64 || cin == 128) && nout >= 1 && nout <= 8 ? hob_ws_bytes((long)B * H * W, cin) : 0;
}
int rd_head_out_bwd(const float* d_out, long out_batch_stride, long n_off, const void* x, int x_cstride, int x_coff, const float* w,
                    int relu_mask, const float* scale, void* dx, int dx_cstride, int dx_coff, float* dw, float* dbias, int B, int H,
                    int W, int cin, int nout, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(d_out && x && w && dw && dbias && ws, RD_EINVAL, "head_out_bwd: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "head_out_bwd: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "head_out_bwd: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(cin == 64 || cin == 128, RD_ESHAPE, "head_out_bwd: cin %d (64 or 128)", cin);
  RD_REQUIRE(nout >= 1 && nout <= 8, RD_ESHAPE, "head_out_bwd: nout %d (1..8)", nout);
  const long HW = (long)H * W, total = (long)B * HW;
  RD_REQUIRE(n_off >= 0 && out_batch_stride >= (n_off + HW) * nout, RD_ESHAPE, "head_out_bwd: batch stride %ld < (n_off %ld + %ld) * %d",
             out_batch_stride, n_off, HW, nout);
  RD_REQUIRE(nhwc16_ok(x_cstride, x_coff, cin) && (!dx || nhwc16_ok(dx_cstride, dx_coff, cin)), RD_ESHAPE,
             "head_out_bwd: channel strides and offsets are multiples of 8 with coff + cin <= cstride");
  RD_REQUIRE(((uintptr_t)x | (uintptr_t)dx) % 16 == 0 && ((uintptr_t)ws | (uintptr_t)d_out | (uintptr_t)dw | (uintptr_t)dbias) % 4 == 0, RD_EINVAL,
             "head_out_bwd: x and dx must be 16-byte aligned, the float buffers 4-byte aligned");
  const size_t need = hob_ws_bytes(total, cin);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "head_out_bwd: workspace %zu < %zu bytes", ws_bytes, need);
  HobArgs a;
  a.d_out = d_out; a.obs = out_batch_stride; a.n_off = n_off; a.HW = HW; a.total = total;
  const int nb = hob_blocks(total);
  a.per_block = (total + nb - 1) / nb;
  a.x = (const unsigned short*)x; a.x_cs = x_cstride; a.x_co = x_coff;
  a.w = w; a.scale = scale; a.relu_mask = relu_mask ? 1 : 0; a.nout = nout;
  a.dx = (unsigned short*)dx; a.dx_cs = dx_cstride; a.dx_co = dx_coff;
  a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (cin == 128) RD_LAUNCH_H16(dtype, (head_out_bwd_kernel<DT, 128>), dim3(nb), dim3(256), st, a);
  else RD_LAUNCH_H16(dtype, (head_out_bwd_kernel<DT, 64>), dim3(nb), dim3(256), st, a);
  hipLaunchKernelGGL(head_out_bwd_reduce_kernel, dim3((nout * cin + nout + 255) / 256), dim3(256), 0, st, (const float*)ws, nb, cin, nout, dw, dbias);
  return check_launch("head_out_bwd");
}

// ---- training-mode batch norm of a head-tower layer (k_norm.h) ---------------------------------------------------------------
size_t rd_bn_stats_workspace_bytes(int B, int H, int W, int C, int split) {
  return bhw_ok(B, H, W) && nm_channels_ok(C) && split >= 0 ? (size_t)nm_parts((long)B * H * W, split) * 3 * C * sizeof(float) : 0;
}
int rd_bn_stats(const void* z, int z_cstride, int z_coff, float* mean, float* var, int B, int H, int W, int C, int split, int dtype, void* ws,
                size_t ws_bytes, void* stream) {
  RD_REQUIRE(z && mean && var && ws, RD_EINVAL, "bn_stats: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "bn_stats: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "bn_stats: split %d (0: the library's choice)", split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "bn_stats: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "bn_stats: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(z_cstride, z_coff, C), RD_ESHAPE, "bn_stats: channel stride and offset are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE((uintptr_t)z % 16 == 0 && ((uintptr_t)mean | (uintptr_t)var | (uintptr_t)ws) % 4 == 0, RD_EINVAL,
             "bn_stats: z must be 16-byte aligned, the float buffers 4-byte aligned");
  const size_t need = rd_bn_stats_workspace_bytes(B, H, W, C, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "bn_stats: workspace %zu < %zu bytes", ws_bytes, need);
  NmStatsArgs a;
  a.z = (const unsigned short*)z; a.cs = z_cstride; a.co = z_coff; a.C = C;
  a.npix = (long)B * H * W; a.P = (int)nm_parts(a.npix, split); a.part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  RD_LAUNCH_H16(dtype, (bn_stats_partial_kernel<DT>), dim3(a.P), dim3(256), st, a);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C / 8), dim3(256), 0, st, (const float*)ws, a.P, C, a.npix, mean, var);
  return check_launch("bn_stats");
}

int rd_bn_fold(const float* mean, const float* var, const float* gamma, const float* beta, float eps, float momentum, long n, int unbiased,
               float* rstd, float* a, float* b, float* moving_mean, float* moving_var, int C, void* stream) {
  RD_REQUIRE(mean && var && gamma && beta && rstd && a && b, RD_EINVAL, "bn_fold: null pointer");
  RD_REQUIRE(C >= 1 && n >= 1 && (!unbiased || n >= 2), RD_ESHAPE, "bn_fold: C %d, n %ld (at least 2 for the unbiased moving variance)", C, n);
  RD_REQUIRE(((uintptr_t)mean | (uintptr_t)var | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)rstd | (uintptr_t)a | (uintptr_t)b |
              (uintptr_t)moving_mean | (uintptr_t)moving_var) % 4 == 0, RD_EINVAL, "bn_fold: the float buffers must be 4-byte aligned");
  NmFoldArgs f;
  f.mean = mean; f.var = var; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
  f.nratio = unbiased ? (float)n / (float)(n - 1) : 0.f;
  f.rstd = rstd; f.a = a; f.b = b; f.mmean = moving_mean; f.mvar = moving_var; f.C = C;
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, f);
  return check_launch("bn_fold");
}

int rd_affine_relu(const void* z, int z_cstride, int z_coff, const float* a, const float* b, int relu, void* y, int y_cstride, int y_coff,
                   int B, int H, int W, int C, int dtype, void* stream) {
  RD_REQUIRE(z && a && b && y, RD_EINVAL, "affine_relu: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "affine_relu: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "affine_relu: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "affine_relu: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(z_cstride, z_coff, C) && nhwc16_ok(y_cstride, y_coff, C), RD_ESHAPE,
             "affine_relu: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)z | (uintptr_t)y) % 16 == 0 && ((uintptr_t)a | (uintptr_t)b) % 4 == 0, RD_EINVAL,
             "affine_relu: the tensors must be 16-byte aligned, a and b 4-byte aligned");
  NmAffineArgs f;
  f.z = (const unsigned short*)z; f.z_cs = z_cstride; f.z_co = z_coff; f.a = a; f.b = b; f.relu = relu ? 1 : 0;
  f.y = (unsigned short*)y; f.y_cs = y_cstride; f.y_co = y_coff; f.C = C; f.npix = (long)B * H * W;
  const long nb = nm_ew_blocks(f.npix, C);
  RD_REQUIRE(nb <= 0x7fffffffL, RD_ESHAPE, "affine_relu: %ld pixels", f.npix);
  hipStream_t st = (hipStream_t)stream;
  RD_LAUNCH_H16(dtype, (affine_relu_kernel<DT>), dim3((unsigned)nb), dim3(256), st, f);
  return check_launch("affine_relu");
}

size_t rd_bn_relu_bwd_workspace_bytes(int B, int H, int W, int C, int split) {
  return bhw_ok(B, H, W) && nm_channels_ok(C) && split >= 0 ? (size_t)nm_parts((long)B * H * W, split) * 2 * C * sizeof(float) : 0;
}
int rd_bn_relu_bwd(const void* g, int g_cstride, int g_coff, const void* z, int z_cstride, int z_coff, const float* a, const float* b,
                   const float* mean, const float* rstd, const float* gamma, int relu, void* dz, int dz_cstride, int dz_coff, float* dgamma,
                   float* dbeta, int B, int H, int W, int C, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(g && z && mean && rstd && gamma && dz && dgamma && dbeta && ws && (!relu || (a && b)), RD_EINVAL, "bn_relu_bwd: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "bn_relu_bwd: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "bn_relu_bwd: split %d (0: the library's choice)", split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "bn_relu_bwd: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "bn_relu_bwd: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(g_cstride, g_coff, C) && nhwc16_ok(z_cstride, z_coff, C) && nhwc16_ok(dz_cstride, dz_coff, C), RD_ESHAPE,
             "bn_relu_bwd: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)g | (uintptr_t)z | (uintptr_t)dz) % 16 == 0 &&
             ((uintptr_t)a | (uintptr_t)b | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gamma | (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)ws) % 4 == 0,
             RD_EINVAL, "bn_relu_bwd: the tensors must be 16-byte aligned, the float buffers 4-byte aligned");
  const size_t need = rd_bn_relu_bwd_workspace_bytes(B, H, W, C, split);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "bn_relu_bwd: workspace %zu < %zu bytes", ws_bytes, need);
  NmBwdArgs f;
  f.g = (const unsigned short*)g; f.z = (const unsigned short*)z; f.g_cs = g_cstride; f.g_co = g_coff; f.z_cs = z_cstride; f.z_co = z_coff;
  f.a = a; f.b = b; f.mean = mean; f.rstd = rstd; f.gamma = gamma; f.relu = relu ? 1 : 0;
  f.dz = (unsigned short*)dz; f.dz_cs = dz_cstride; f.dz_co = dz_coff; f.C = C;
  f.npix = (long)B * H * W; f.P = (int)nm_parts(f.npix, split); f.part = (float*)ws; f.dgamma = dgamma; f.dbeta = dbeta;
  const long nb = nm_ew_blocks(f.npix, C);
  RD_REQUIRE(nb <= 0x7fffffffL, RD_ESHAPE, "bn_relu_bwd: %ld pixels", f.npix);
  hipStream_t st = (hipStream_t)stream;
  RD_LAUNCH_H16(dtype, (bn_bwd_partial_kernel<DT>), dim3(f.P), dim3(256), st, f);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C / 8, 2), dim3(256), 0, st, (const float*)ws, f.P, C, dbeta, dgamma);
  RD_LAUNCH_H16(dtype, (bn_bwd_dz_kernel<DT>), dim3((unsigned)nb), dim3(256), st, f);
  return check_launch("bn_relu_bwd");
}

// the residual form: the second BatchNorm of a backbone BasicBlock, + shortcut, ReLU
int rd_affine_add_relu(const void* z, int z_cstride, int z_coff, const float* a, const float* b, const void* r, int r_cstride, int r_coff,
                       const float* ar, const float* br, int relu, void* y, int y_cstride, int y_coff, int B, int H, int W, int C, int dtype,
                       void* stream) {
  RD_REQUIRE(z && a && b && r && y, RD_EINVAL, "affine_add_relu: null pointer");
  RD_REQUIRE(!ar == !br, RD_EINVAL, "affine_add_relu: ar and br go together (both NULL: an identity shortcut)");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "affine_add_relu: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "affine_add_relu: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "affine_add_relu: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(z_cstride, z_coff, C) && nhwc16_ok(r_cstride, r_coff, C) && nhwc16_ok(y_cstride, y_coff, C), RD_ESHAPE,
             "affine_add_relu: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)z | (uintptr_t)r | (uintptr_t)y) % 16 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)ar | (uintptr_t)br) % 4 == 0,
             RD_EINVAL, "affine_add_relu: the tensors must be 16-byte aligned, the float vectors 4-byte aligned");
  NmAddArgs f;
  f.z = (const unsigned short*)z; f.z_cs = z_cstride; f.z_co = z_coff; f.r = (const unsigned short*)r; f.r_cs = r_cstride; f.r_co = r_coff;
  f.a = a; f.b = b; f.ar = ar; f.br = br; f.relu = relu ? 1 : 0;
  f.y = (unsigned short*)y; f.y_cs = y_cstride; f.y_co = y_coff; f.C = C; f.npix = (long)B * H * W;
  const long nb = nm_ew_blocks(f.npix, C);
  RD_REQUIRE(nb <= 0x7fffffffL, RD_ESHAPE, "affine_add_relu: %ld pixels", f.npix);
  hipStream_t st = (hipStream_t)stream;
  if (ar) RD_LAUNCH_H16(dtype, (affine_add_relu_kernel<DT, true>), dim3((unsigned)nb), dim3(256), st, f);
  else RD_LAUNCH_H16(dtype, (affine_add_relu_kernel<DT, false>), dim3((unsigned)nb), dim3(256), st, f);
  return check_launch("affine_add_relu");
}

// the join of an aggregation stage: the ReLU before the add
int rd_affine_relu_add(const void* z, int z_cstride, int z_coff, const float* a, const float* b, const void* r, int r_cstride, int r_coff,
                       void* y, int y_cstride, int y_coff, int B, int H, int W, int C, int dtype, void* stream) {
  RD_REQUIRE(z && a && b && r && y, RD_EINVAL, "affine_relu_add: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "affine_relu_add: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "affine_relu_add: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "affine_relu_add: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(z_cstride, z_coff, C) && nhwc16_ok(r_cstride, r_coff, C) && nhwc16_ok(y_cstride, y_coff, C), RD_ESHAPE,
             "affine_relu_add: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)z | (uintptr_t)r | (uintptr_t)y) % 16 == 0 && ((uintptr_t)a | (uintptr_t)b) % 4 == 0, RD_EINVAL,
             "affine_relu_add: the tensors must be 16-byte aligned, a and b 4-byte aligned");
  NmAddArgs f;
  f.z = (const unsigned short*)z; f.z_cs = z_cstride; f.z_co = z_coff; f.r = (const unsigned short*)r; f.r_cs = r_cstride; f.r_co = r_coff;
  f.a = a; f.b = b; f.ar = nullptr; f.br = nullptr; f.relu = 1;
  f.y = (unsigned short*)y; f.y_cs = y_cstride; f.y_co = y_coff; f.C = C; f.npix = (long)B * H * W;
  const long nb = nm_ew_blocks(f.npix, C);
  RD_REQUIRE(nb <= 0x7fffffffL, RD_ESHAPE, "affine_relu_add: %ld pixels", f.npix);
  hipStream_t st = (hipStream_t)stream;
  RD_LAUNCH_H16(dtype, (affine_relu_add_kernel<DT>), dim3((unsigned)nb), dim3(256), st, f);
  return check_launch("affine_relu_add");
}

size_t rd_bn_add_relu_bwd_workspace_bytes(int B, int H, int W, int C, int split, int projection) {
  return bhw_ok(B, H, W) && nm_channels_ok(C) && split >= 0 ? (size_t)nm_parts((long)B * H * W, split) * (projection ? 3 : 2) * C * sizeof(float) : 0;
}
int rd_bn_add_relu_bwd(const void* g, int g_cstride, int g_coff, const void* z, int z_cstride, int z_coff, const void* r, int r_cstride,
                       int r_coff, const float* a, const float* b, const float* mean, const float* rstd, const float* gamma, const float* ar,
                       const float* br, const float* mean_r, const float* rstd_r, const float* gamma_r, void* dz, int dz_cstride, int dz_coff,
                       void* dr, int dr_cstride, int dr_coff, float* dgamma, float* dbeta, float* dgamma_r, float* dbeta_r, int B, int H, int W,
                       int C, int split, int dtype, void* ws, size_t ws_bytes, void* stream) {
  RD_REQUIRE(g && z && r && a && b && mean && rstd && gamma && dz && dr && dgamma && dbeta && ws, RD_EINVAL, "bn_add_relu_bwd: null pointer");
  const bool proj = ar != nullptr;
  RD_REQUIRE(proj ? (br && mean_r && rstd_r && gamma_r && dgamma_r && dbeta_r) : (!br && !mean_r && !rstd_r && !gamma_r && !dgamma_r && !dbeta_r),
             RD_EINVAL, "bn_add_relu_bwd: ar, br, mean_r, rstd_r, gamma_r, dgamma_r and dbeta_r go together (all NULL: an identity shortcut)");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "bn_add_relu_bwd: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(split >= 0, RD_EINVAL, "bn_add_relu_bwd: split %d (0: the library's choice)", split);
  RD_REQUIRE(bhw_ok(B, H, W), RD_ESHAPE, "bn_add_relu_bwd: B %d, H %d, W %d", B, H, W);
  RD_REQUIRE(nm_channels_ok(C), RD_ESHAPE, "bn_add_relu_bwd: C %d (8, 16, 32, 64, 128 or 256)", C);
  RD_REQUIRE(nhwc16_ok(g_cstride, g_coff, C) && nhwc16_ok(z_cstride, z_coff, C) && nhwc16_ok(r_cstride, r_coff, C) &&
             nhwc16_ok(dz_cstride, dz_coff, C) && nhwc16_ok(dr_cstride, dr_coff, C), RD_ESHAPE,
             "bn_add_relu_bwd: channel strides and offsets are multiples of 8 with coff + C <= cstride");
  RD_REQUIRE(((uintptr_t)g | (uintptr_t)z | (uintptr_t)r | (uintptr_t)dz | (uintptr_t)dr) % 16 == 0 &&
             ((uintptr_t)a | (uintptr_t)b | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gamma | (uintptr_t)ar | (uintptr_t)br | (uintptr_t)mean_r |
              (uintptr_t)rstd_r | (uintptr_t)gamma_r | (uintptr_t)dgamma | (uintptr_t)dbeta | (uintptr_t)dgamma_r | (uintptr_t)dbeta_r | (uintptr_t)ws) % 4 == 0,
             RD_EINVAL, "bn_add_relu_bwd: the tensors must be 16-byte aligned, the float buffers 4-byte aligned");
  const size_t need = rd_bn_add_relu_bwd_workspace_bytes(B, H, W, C, split, proj);
  RD_REQUIRE(ws_bytes >= need, RD_EWORKSPACE, "bn_add_relu_bwd: workspace %zu < %zu bytes", ws_bytes, need);
  NmAddBwdArgs f;
  f.g = (const unsigned short*)g; f.z = (const unsigned short*)z; f.r = (const unsigned short*)r;
  f.g_cs = g_cstride; f.g_co = g_coff; f.z_cs = z_cstride; f.z_co = z_coff; f.r_cs = r_cstride; f.r_co = r_coff;
  f.a = a; f.b = b; f.mean = mean; f.rstd = rstd; f.gamma = gamma;
  f.ar = ar; f.br = br; f.mean_r = mean_r; f.rstd_r = rstd_r; f.gamma_r = gamma_r;
  f.dz = (unsigned short*)dz; f.dz_cs = dz_cstride; f.dz_co = dz_coff; f.dr = (unsigned short*)dr; f.dr_cs = dr_cstride; f.dr_co = dr_coff; f.C = C;
  f.npix = (long)B * H * W; f.P = (int)nm_parts(f.npix, split); f.part = (float*)ws;
  f.dbeta = dbeta; f.dgamma = dgamma; f.dgamma_r = dgamma_r;
  const long nb = nm_ew_blocks(f.npix, C);
  RD_REQUIRE(nb <= 0x7fffffffL, RD_ESHAPE, "bn_add_relu_bwd: %ld pixels", f.npix);
  hipStream_t st = (hipStream_t)stream;
  if (proj) RD_LAUNCH_H16(dtype, (bn_add_bwd_partial_kernel<DT, true>), dim3(f.P), dim3(256), st, f);
  else RD_LAUNCH_H16(dtype, (bn_add_bwd_partial_kernel<DT, false>), dim3(f.P), dim3(256), st, f);
  hipLaunchKernelGGL(bn_add_bwd_final_kernel, dim3(C / 8, proj ? 3 : 2), dim3(256), 0, st, (const float*)ws, f.P, C, dbeta, dgamma, dbeta_r, dgamma_r);
  if (proj) RD_LAUNCH_H16(dtype, (bn_add_bwd_dzdr_kernel<DT, true>), dim3((unsigned)nb), dim3(256), st, f);
  else RD_LAUNCH_H16(dtype, (bn_add_bwd_dzdr_kernel<DT, false>), dim3((unsigned)nb), dim3(256), st, f);
  return check_launch("bn_add_relu_bwd");
}

// ---- SGD with momentum over a table of tensors, and the conv weight images re-packed on the device (k_optim.h) ----------------------
static int sgd_table_count(const rd_sgd_tensor_t* t, int nt, long* n_chunks, long* n_pack) {
  RD_REQUIRE(t && nt > 0, RD_EINVAL, "sgd_table: no tensors");
  *n_chunks = *n_pack = 0;
  for (int i = 0; i < nt; ++i) {
    const int rc = sgd_check_tensor(t[i], i);
    if (rc != RD_OK) return rc;
    *n_chunks += sgd_tensor_chunks(t[i]);
    *n_pack += sgd_tensor_pack_chunks(t[i]);
  }
  RD_REQUIRE(*n_chunks <= 0x7fffffffL && *n_pack <= 0x7fffffffL && sgd_table_size(nt, *n_chunks, *n_pack) <= 0x7fffffffUL, RD_ESHAPE,
             "sgd_table: %ld element chunks and %ld image chunks exceed one launch", *n_chunks, *n_pack);
  return RD_OK;
}
size_t rd_sgd_table_bytes(const rd_sgd_tensor_t* tensors, int nt) {
  long nc, np;
  return sgd_table_count(tensors, nt, &nc, &np) == RD_OK ? sgd_table_size(nt, nc, np) : 0;
}
int rd_sgd_table_host(const rd_sgd_tensor_t* tensors, int nt, int dtype, void* out) {
  RD_REQUIRE(out, RD_EINVAL, "sgd_table: null pointer");
  long nc, np;
  const int rc = sgd_table_count(tensors, nt, &nc, &np);
  if (rc != RD_OK) return rc;
  RD_REQUIRE(np == 0 || is_h16(dtype), RD_EINVAL, "sgd_table: dtype %d of the images (RD_BF16 or RD_F16)", dtype);
  sgd_table_build(tensors, nt, dtype, nc, np, out);
  return RD_OK;
}
int rd_sgd_mom_update(const void* table_dev, const void* table_host, float lr, float momentum, float wd, float rescale_grad,
                      float clip_gradient, void* stream) {
  RD_REQUIRE(table_dev && table_host, RD_EINVAL, "sgd_mom_update: null pointer");
  RD_REQUIRE((uintptr_t)table_dev % 8 == 0, RD_EINVAL, "sgd_mom_update: the device table must be 8-byte aligned");
  SgdHeader h;
  memcpy(&h, table_host, sizeof(h));
  RD_REQUIRE(h.magic == SGD_MAGIC && h.nt > 0 && h.n_chunks > 0 && h.n_pack >= 0 && h.bytes == sgd_table_size(h.nt, h.n_chunks, h.n_pack) &&
             (h.n_pack == 0 || is_h16(h.dtype)), RD_EINVAL, "sgd_mom_update: table_host is not a table of rd_sgd_table_host");
  hipStream_t st = (hipStream_t)stream;
  const SgdStep s{lr, momentum, wd, rescale_grad, clip_gradient};
  hipLaunchKernelGGL(sgd_mom_kernel, dim3((unsigned)h.n_chunks), dim3(256), 0, st, (const unsigned char*)table_dev, s);
  if (h.n_pack > 0) RD_LAUNCH_H16(h.dtype, (sgd_pack_kernel<DT>), dim3((unsigned)h.n_pack), dim3(256), st, (const unsigned char*)table_dev);
  return check_launch("sgd_mom_update");
}
int rd_pack_conv3x3_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin, int flip, int dtype, void* out_dev, void* stream) {
  RD_REQUIRE(w_dev && out_dev, RD_EINVAL, "pack_conv3x3_dev: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv3x3_dev: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(sgd_pack_shape_ok(cout, cin), RD_ESHAPE, "pack_conv3x3_dev: %d -> %d channels (64 or 128 on either side)", cin, cout);
  RD_REQUIRE(!(flip && fold_scale_dev), RD_EINVAL, "pack_conv3x3_dev: the data-gradient image takes no fold scale");
  RD_REQUIRE((uintptr_t)out_dev % 16 == 0 && ((uintptr_t)w_dev | (uintptr_t)fold_scale_dev) % 4 == 0, RD_EINVAL,
             "pack_conv3x3_dev: the image must be 16-byte aligned, the float buffers 4-byte aligned");
  const unsigned grid = (unsigned)((sgd_image_slots(cout, cin) + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS);
  RD_LAUNCH_H16(dtype, (pack_conv3x3_dev_kernel<DT>), dim3(grid), dim3(256), (hipStream_t)stream, w_dev, fold_scale_dev, cout, cin, flip ? 1 : 0,
                (unsigned short*)out_dev);
  return check_launch("pack_conv3x3_dev");
}

// ---- launch images of the narrow-input convs from device-resident masters (k_convbwd_narrow.h) ------------------------------------------
static int nwp_launch(const char* what, const float* w_dev, const float* fold_scale_dev, int cout, int cin, int mode, int dtype, void* out_dev,
                      void* stream) {
  RD_REQUIRE((uintptr_t)out_dev % 16 == 0 && ((uintptr_t)w_dev | (uintptr_t)fold_scale_dev) % 4 == 0, RD_EINVAL,
             "%s: the image must be 16-byte aligned, the float buffers 4-byte aligned", what);
  const long body = nwp_body_slots(mode, cout), total = nwp_total_slots(mode, cout, cin, dtype);
  RD_LAUNCH_H16(dtype, (pack_narrow_dev_kernel<DT>), dim3((unsigned)((total + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS)), dim3(256), (hipStream_t)stream,
                w_dev, fold_scale_dev, cout, cin, mode, body, total, (unsigned short*)out_dev);
  return check_launch(what);
}
int rd_pack_conv_narrow_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin, int ksize, int dtype, void* out_dev, void* stream) {
  RD_REQUIRE(w_dev && out_dev, RD_EINVAL, "pack_conv_narrow_dev: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv_narrow_dev: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(ksize == 1 || ksize == 3, RD_ESHAPE, "pack_conv_narrow_dev: ksize %d (1 or 3)", ksize);
  RD_REQUIRE(nw_shape_ok(cin, cout, ksize), RD_ESHAPE, "pack_conv_narrow_dev: cin %d (1 .. 16), cout %d (64 or 128)", cin, cout);
  RD_REQUIRE(!(ksize == 1 && fold_scale_dev), RD_EINVAL, "pack_conv_narrow_dev: the 1x1 image takes no fold scale");
  return nwp_launch("pack_conv_narrow_dev", w_dev, fold_scale_dev, cout, cin, ksize == 3 ? NWP_NARROW3 : NWP_NARROW1, dtype, out_dev, stream);
}
int rd_pack_conv3x3_cat_dev(const float* w_dev, const float* fold_scale_dev, int cout, int cin1, int cin2, int data_grad, int dtype,
                            void* out_dev, void* stream) {
  RD_REQUIRE(w_dev && out_dev, RD_EINVAL, "pack_conv3x3_cat_dev: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_conv3x3_cat_dev: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(cin1 == NWP_CIN1, RD_ESHAPE, "pack_conv3x3_cat_dev: cin1 %d (64: the agg3 feature map)", cin1);
  RD_REQUIRE(nw_shape_ok(cin2, cout, 3), RD_ESHAPE, "pack_conv3x3_cat_dev: cin2 %d (1 .. 16), cout %d (64 or 128)", cin2, cout);
  RD_REQUIRE(data_grad || cin2 % 8 == 0, RD_ESHAPE, "pack_conv3x3_cat_dev: cin2 %d (the forward reads a multiple of 8)", cin2);
  RD_REQUIRE(!(data_grad && fold_scale_dev), RD_EINVAL, "pack_conv3x3_cat_dev: the data-gradient image takes no fold scale");
  return nwp_launch("pack_conv3x3_cat_dev", w_dev, fold_scale_dev, cout, cin1 + cin2, data_grad ? NWP_CAT_BWD : NWP_CAT_FWD, dtype, out_dev, stream);
}

// the data gradient of a transposed conv as a 3x3 stride-1 conv over dz read as [H][Win][s Cout]: its weight image, host and device
static bool deconv_train_ok(int cin, int cout, int kw, int stride_w, int pad_w) {
  return bw_deconv_form_ok(kw, stride_w, pad_w) && bw_deconv_shape_ok(cin, cout, kw);
}
int rd_pack_deconv_data_grad_host(const float* w, int cin, int cout, int kw, int stride_w, int pad_w, int dtype, void* out) {
  RD_REQUIRE(w && out, RD_EINVAL, "pack_deconv_data_grad: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_deconv_data_grad: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(deconv_train_ok(cin, cout, kw, stride_w, pad_w), RD_ESHAPE,
             "pack_deconv_data_grad: %d -> %d channels, kernel (3,%d), stride (1,%d), pad (1,%d) -- the four transposed convs of the network",
             cin, cout, kw, stride_w, pad_w);
  const int cv = stride_w * cout;
  std::vector<float> wv((size_t)cin * cv * 9, 0.f);   // Wv[ci][e cout + co][kh][dwv + 1] = W[ci][co][kh][s dwv + e + p]
  for (int ci = 0; ci < cin; ++ci)
    for (int c2 = 0; c2 < cv; ++c2)
      for (int kh = 0; kh < 3; ++kh)
        for (int d = 0; d < 3; ++d) {
          const int kx = stride_w * (d - 1) + c2 / cout + pad_w;
          if (kx >= 0 && kx < kw) wv[(((size_t)ci * cv + c2) * 3 + kh) * 3 + d] = w[(((size_t)ci * cout + c2 % cout) * 3 + kh) * kw + kx];
        }
  return rd_pack_conv3x3_ex_host(wv.data(), nullptr, cin, cv, 1, cv, dtype, out);
}
int rd_pack_deconv_dev(const float* w_dev, int cin, int cout, int kw, int stride_w, int pad_w, int data_grad, long w_phase_bytes, int dtype,
                       void* out_dev, void* stream) {
  RD_REQUIRE(w_dev && out_dev, RD_EINVAL, "pack_deconv_dev: null pointer");
  RD_REQUIRE(is_h16(dtype), RD_EINVAL, "pack_deconv_dev: dtype %d (RD_BF16 or RD_F16)", dtype);
  RD_REQUIRE(deconv_train_ok(cin, cout, kw, stride_w, pad_w), RD_ESHAPE,
             "pack_deconv_dev: %d -> %d channels, kernel (3,%d), stride (1,%d), pad (1,%d) -- the four transposed convs of the network", cin, cout,
             kw, stride_w, pad_w);
  RD_REQUIRE((uintptr_t)out_dev % 16 == 0 && (uintptr_t)w_dev % 4 == 0, RD_EINVAL,
             "pack_deconv_dev: the image must be 16-byte aligned, the weight 4-byte aligned");
  const long per = data_grad ? deconv_dgrad_slots(cin, cout, stride_w) : deconv_phase_slots(cin, cout);
  RD_REQUIRE(data_grad || (w_phase_bytes >= per * 16 && w_phase_bytes % 16 == 0), RD_EINVAL,
             "pack_deconv_dev: w_phase_bytes %ld (a multiple of 16, at least the %ld bytes of a phase image)", w_phase_bytes, per * 16);
  const long total = data_grad ? per : per * stride_w;
  RD_LAUNCH_H16(dtype, (pack_deconv_dev_kernel<DT>), dim3((unsigned)((total + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS)), dim3(256),
                (hipStream_t)stream, w_dev, cin, cout, kw, stride_w, pad_w, data_grad ? 1 : 0, data_grad ? 0L : w_phase_bytes / 2,
                (unsigned short*)out_dev);
  return check_launch("pack_deconv_dev");
}

// ---- profiling -------------------------------------------------------------------------------------------------
// dev only (not part of include/rangedet_hip.h): the phase trace of the conv kernels.  rd_dev_conv_trace_set registers a
// caller-owned, zeroed device buffer of at least 2^20 64-bit words (nullptr: tracing off); rd_dev_conv_trace_read copies the first n
// words of it to the host.
int rd_dev_conv_trace_set(unsigned long long* device_buf, long nwords) {
  if (device_buf && nwords < (long)CONV_TRACE_CAP) return RD_EINVAL;
  conv_trace_slot() = device_buf;
  return RD_OK;
}
int rd_dev_conv_trace_read(unsigned long long* out, long n) {
  if (!conv_trace_buf() || n > (long)CONV_TRACE_CAP) return RD_EINVAL;
  return hipMemcpy(out, conv_trace_buf(), n * 8, hipMemcpyDeviceToHost) == hipSuccess ? RD_OK : RD_EHIP;
}
int rd_prof_enable(int on) {
  Prof& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  p.on = on != 0;
  return RD_OK;
}
int rd_prof_reset(void) {
  Prof& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  p.drain();
  for (int k = 0; k < RD_PROF_NKINDS; ++k) { p.total[k] = 0; p.count[k] = 0; }
  return RD_OK;
}
int rd_prof_get(int kind, double* total_ms, long* launches) {
  RD_REQUIRE(kind >= 0 && kind < RD_PROF_NKINDS && total_ms && launches, RD_EINVAL, "prof_get: bad arguments");
  Prof& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  p.drain();
  *total_ms = p.total[kind];
  *launches = p.count[kind];
  return RD_OK;
}

}  // extern "C"
