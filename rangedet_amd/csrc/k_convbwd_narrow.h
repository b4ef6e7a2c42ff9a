// Weight gradient of the convs that read the range image itself (16-bit activations, float32 gradient): res1_unit1's conv1 (c -> 64,
// 3x3) and projection shortcut (c -> 64, 1x1), and the range-image columns of the level-0 conv_0 (64 + c -> 128, 3x3).  c is 8 (Waymo) or
// 5 (KITTI); the image lives in a zero-padded 16-channel slot, and the kernel reads that slot per pixel, exactly as the forward does.
//   conv_bwd_weight_narrow_kernel   dW[co][ci][ky][kx] = sum over pixels of dz[pix][co] * x[pix + (ky - p, kx - p)][ci], partial sums per
//                                   workgroup in the workspace;  bwd_weight_reduce_strided_kernel adds them in index order and writes the
//                                   channels [cin_off, cin_off + cin) of a (cout, cin_stride, k, k) gradient, nothing else
// No atomics: every sum has a fixed order, two calls give the same bits, and the split never looks at the device.
//
// Why not k_convbwd.h's kernel on a zero-padded image: it is built for 64 or 128 channels on the x side (a 32-wide N tile per wave) and a
// workgroup owns ONE tap column, so dz is read three times; at 16 real channels that is four times the MFMA work on zeros and three times
// the bytes.  Here the bytes decide: a pixel is 32 bytes of x and 2 cout bytes of dz against 2 * 144 * cout multiply-adds, so a workgroup
// owns ALL of cout x (taps x slot) and a contiguous run of pixel chunks: dz is read exactly once, x once plus the halo rows of a strip.
//
// The GEMM: M = cout (A = dz transposed), N = taps x 16 slot channels (B = x), K = pixels.  The MFMA is v_mfma_f32_16x16x32: one tap's
// 16-channel slot is exactly one N tile, so no lane computes a channel that does not exist in the slot (with 32x32x16 half of every tile
// would be a second tap's slot or zeros, and a k-step would be 16 pixels instead of 32).  Lane l holds k = 8 (l >> 4) .. + 8 of row
// l & 15 in both operands; D[m][n] sits in lane n + 16 (m / 4), register m % 4.
// Both operands run along the pixel axis and memory is channels-last, so both go through k_convbwd.h's register transpose (bw_load, an
// 8 pixel x 8 channel block per thread, and bw_store_t into [channel][pixel] rows of 64 + 8 pixels).  The x slot is only 16 rows, so
// the KS column-shifted copies of an x row (x[w + dw] at column w, zeros outside the image) are all kept: every fragment read is an
// aligned 16-byte row read, and the three tap rows are a ring of three x rows while the workgroup walks down a strip of NW_RH rows.  The
// shifted copies are loaded by three groups of sixteen threads from the same lines (the second and third are cache hits).
// Wave w owns the output channels [cout / 4 * w, + cout / 4) -- MT = cout / 64 M tiles -- and all KS * KS N tiles: 9 MT accumulators of four
// registers.  ksize 1 is the same kernel with one tap: no halo rows, no ring, no shifted copies.
// Slot channels at or above cin are multiplied like the others (they are finite) and dropped when the partial image is written.
#pragma once
#include "k_convbwd.h"
#include "k_optim.h"

namespace rd {
constexpr int NW_PT = BW_PT;          // pixels of a tile: two k-steps of 32
constexpr int NW_RH = 16;             // image rows of a chunk
constexpr int NW_SLOT = 16;           // channels of the x slot: one N tile
constexpr int NW_WG_TARGET = 512;     // workgroups of a launch with the library's own split: two per CU of a 256-CU part

inline bool nw_shape_ok(int cin, int cout, int ksize) { return cin >= 1 && cin <= NW_SLOT && (cout == 64 || cout == 128) && (ksize == 1 || ksize == 3); }
inline long nw_chunks(int B, int H, int W) { return (long)B * ((H + NW_RH - 1) / NW_RH) * ((W + NW_PT - 1) / NW_PT); }
// partial sums per output element: the caller's cap (split > 0) or the library's, never more than there are chunks.  A partial image is
// at most 9 * 128 * 16 * 4 = 72 KB against 160 KB or more of input per chunk, so the library's split stops only at the workgroup count.
inline long nw_split(int B, int H, int W, int split) {
  const long n = nw_chunks(B, H, W), cap = split > 0 ? split : NW_WG_TARGET;
  return n < cap ? n : cap;
}
inline size_t nw_ws_bytes(int B, int H, int W, int cin, int cout, int ksize, int split) {
  return (size_t)nw_split(B, H, W, split) * ksize * ksize * cout * cin * sizeof(float);
}

struct NarrowWArgs {
  const unsigned short *x, *dz;
  int x_cs, x_co, dz_cs, dz_co;
  int B, H, W, nwt, nhs, cin;
  long nchunks;
  float* part;   // [S][KS * KS][cout][cin]
};

// grid (S), 256 threads.  Threads [0, 8 cout / 8) load dz (pixel group u % 8, channel group u / 8), the next 16 KS load x (pixel group
// u % 8, half slot (u / 8) % 2, tap column u / 16).
template <int DT, int COUT, int KS>
__global__ __launch_bounds__(256) void conv_bwd_weight_narrow_kernel(NarrowWArgs a) {
  static_assert(KS == 1 || KS == 3, "1x1 or 3x3");
  static_assert(NW_PT % 32 == 0, "whole k-steps");
  constexpr int P = KS / 2, T = KS * KS, MT = COUT / 64;
  constexpr int NZU = (NW_PT / 8) * (COUT / 8), NXU = (NW_PT / 8) * (NW_SLOT / 8) * KS;
  static_assert(NZU + NXU <= 256, "one load unit per thread");
  __shared__ __attribute__((aligned(16))) unsigned short Tx[KS][KS][NW_SLOT][BW_RS];   // [ring row][tap column][slot channel][pixel]
  __shared__ __attribute__((aligned(16))) unsigned short Tz[COUT][BW_RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = gridDim.x, s = blockIdx.x;
  const bool is_z = tid < NZU, is_x = tid >= NZU && tid < NZU + NXU;
  const int u = is_z ? tid : tid - NZU;
  const int pg = u & 7, cg = is_z ? u >> 3 : (u >> 3) & 1, kx = is_x ? u >> 4 : 0, dw = kx - P;
  f32x4 acc[T][MT];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][i][r] = 0.f;

  const long c_lo = s * a.nchunks / S, c_hi = (s + 1) * a.nchunks / S;
  for (long ch = c_lo; ch < c_hi; ++ch) {
    const int wt = (int)(ch % a.nwt), hs = (int)((ch / a.nwt) % a.nhs), b = (int)(ch / ((long)a.nwt * a.nhs));
    const int h0 = hs * NW_RH, h1 = h0 + NW_RH < a.H ? h0 + NW_RH : a.H;
    const int p0 = wt * NW_PT + 8 * pg;
    const unsigned short* xb = a.x + (long)b * a.H * a.W * a.x_cs + a.x_co + 8 * cg;
    const unsigned short* zb = a.dz + (long)b * a.H * a.W * a.dz_cs + a.dz_co + 8 * cg;
    Slot16 v[8];
    auto load_x = [&](int r) {      // x row r shifted by dw; rows outside the image are zeros
      const int rc = r < 0 ? 0 : r >= a.H ? a.H - 1 : r;
      bw_load(xb + (long)rc * a.W * a.x_cs, r == rc, a.x_cs, p0 + dw, a.W, v);
    };
    if (is_x) {
      if constexpr (KS == 3) {
        load_x(h0 - 1);
        bw_store_t(Tx[(h0 + 2) % 3][kx], 8 * cg, pg, v);
        load_x(h0);
        bw_store_t(Tx[h0 % 3][kx], 8 * cg, pg, v);
      }
      load_x(h0 + P);
    } else if (is_z) {
      bw_load(zb + (long)h0 * a.W * a.dz_cs, true, a.dz_cs, p0, a.W, v);
    }
    for (int h = h0; h < h1; ++h) {
      if (is_x) bw_store_t(Tx[(h + P) % KS][kx], 8 * cg, pg, v);
      else if (is_z) bw_store_t(Tz, 8 * cg, pg, v);
      __syncthreads();
      if (h + 1 < h1) {             // the next row's loads fly during this row's MFMAs
        if (is_x) load_x(h + 1 + P);
        else if (is_z) bw_load(zb + (long)(h + 1) * a.W * a.dz_cs, true, a.dz_cs, p0, a.W, v);
      }
      const int r = lane & 15, k8 = 8 * (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < NW_PT / 32; ++ks) {
        s16x8 af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[i] = *(const s16x8*)&Tz[16 * (wave * MT + i) + r][32 * ks + k8];
#pragma unroll
        for (int d = 0; d < KS; ++d)      // tap row dh = d - P: x row h + dh
#pragma unroll
          for (int e = 0; e < KS; ++e) {  // tap column dw = e - P
            const s16x8 bf = *(const s16x8*)&Tx[(h + d + 2 * P) % KS][e][r][32 * ks + k8];
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[d * KS + e][i] = H16<DT>::mfma16(af[i], bf, acc[d * KS + e][i]);
          }
      }
      __syncthreads();
    }
  }
  // D[m][n]: column n = lane & 15 (slot channel), row m = 4 (lane >> 4) + reg (output channel)
  const int ci = lane & 15;
  if (ci < a.cin) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int co = 16 * (wave * MT + i) + 4 * (lane >> 4) + rg;
          a.part[(((long)s * T + t) * COUT + co) * a.cin + ci] = acc[t][i][rg];
        }
  }
}

// bwd_weight_reduce_kernel (k_convbwd.h) writing at a channel stride: dW (cout, cin_stride, nt) channels [cin_off, cin_off + cin) = the S
// partial images [nt][cout][cin] added in index order -- the same additions in the same order, so the bits are those of that kernel.
// There are only nt * cout * cin threads (512 to 9216 for the narrow convs) and up to 512 partial images, and the sum of a thread is one
// dependent chain, so the launch runs at the latency of its loads: they are issued NW_RED_BATCH at a time (independent, clamped to the
// last image and the value dropped) and then added one by one in index order, as bwd1_weight_reduce_kernel does.
constexpr int NW_RED_BATCH = 32;
__global__ __launch_bounds__(256) void bwd_weight_reduce_strided_kernel(const float* __restrict__ part, int S, int cout, int cin,
                                                                        float* __restrict__ dW, int nt, int cin_stride, int cin_off) {
  const int n = nt * cout * cin, idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float sum = 0.f;
  for (int k0 = 0; k0 < S; k0 += NW_RED_BATCH) {
    float v[NW_RED_BATCH];
#pragma unroll
    for (int j = 0; j < NW_RED_BATCH; ++j) {
      const int k = k0 + j < S ? k0 + j : S - 1;
      v[j] = part[(long)k * n + idx];
    }
#pragma unroll
    for (int j = 0; j < NW_RED_BATCH; ++j)
      if (k0 + j < S) sum = k0 + j == 0 ? v[j] : sum + v[j];     // (the first image starts the sum: 0 + -0 would lose its sign)
  }
  const int t = idx / (cout * cin), co = idx / cin % cout, ci = idx % cin;
  dW[((long)co * cin_stride + cin_off + ci) * nt + t] = sum;
}

// ---- the launch images of these convs from a device-resident float32 master (the re-pack behind an optimizer step) ---------------------------
// One thread per 16-byte slot [ks][cb][lane][8] of a step's slab, as in k_optim.h's sgd_pack_slot; the zero fill behind the body and the
// RD_CONV_TAIL zero bytes are written too.  Rounding is round-to-nearest-even, what h16_from_f32 does on the host.
//   NWP_NARROW3   (cout, cin, 3, 3), cin <= 16: the body form [P5] of k_conv3.h -- five steps, k-step ks of step s is tap 2 s + ks on the
//                 first 16 channels (tap 9: zeros) -- what rd_pack_conv3x3_ex_host(w, fold, cout, cin, 1, cin, dtype) writes WITH a fold scale
//   NWP_NARROW1   (cout, cin, 1, 1): pack_taps_frag(1, cin, cout), what rd_pack_conv_weight_host(w, cout, cin, 1, 1, dtype) writes; no scale
//   NWP_CAT_FWD   (cout, 64 + cin2, 3, 3): the body form [T9, T9, P5], what rd_pack_conv3x3_cat_host writes WITH a fold scale
//   NWP_CAT_BWD   the data gradient towards x1: pack_taps_frag(9, cout, 64) of W[q][r][8 - t], image row r the master's input channel
//                 (< 64), image column q its output channel; the master's channel stride is 64 + cin2
// The host packers choose the two body forms only when they are given a fold scale, and the forward launches always read those forms
// (RD_SCALE_FOLDED): the unscaled training image is the host packer called with a vector of ONES -- the product by 1.0f is exact -- and
// fold == nullptr means exactly that here.
enum { NWP_NARROW3 = 0, NWP_NARROW1 = 1, NWP_CAT_FWD = 2, NWP_CAT_BWD = 3 };
constexpr int NWP_CIN1 = 64;
inline long nwp_body_slots(int mode, int cout) {
  const long slab = 2L * (cout / 32) * 64;
  return mode == NWP_NARROW3 ? 5 * slab : mode == NWP_NARROW1 ? slab : mode == NWP_CAT_FWD ? 23 * slab
                                                                                           : (long)(cout / 32) * 9 * 2 * (NWP_CIN1 / 32) * 64;
}
inline long nwp_total_slots(int mode, int cout, int cin, int dt) {   // cin: the master's channels (the concat: 64 + cin2)
  return (long)(mode == NWP_NARROW1 ? conv_packed_bytes(1, cin, cout, dt)
                : mode == NWP_CAT_BWD ? conv_packed_bytes(9, cout, NWP_CIN1, RD_BF16) : conv_packed_bytes(9, cin, cout, RD_BF16)) / 16;
}
template <int DT>
__global__ __launch_bounds__(256) void pack_narrow_dev_kernel(const float* __restrict__ w, const float* __restrict__ fold, int cout, int cin,
                                                              int mode, long body, long total, unsigned short* __restrict__ out) {
  _Pragma("clang fp contract(off)")
  const long slot = (long)blockIdx.x * SGD_PACK_SLOTS + threadIdx.x;
  if (slot >= total) return;
  Slot16 o = {0u, 0u, 0u, 0u};
  if (slot < body) {
    const int ncb = (mode == NWP_CAT_BWD ? NWP_CIN1 : cout) / 32;
    const int sl = (int)slot, lane = sl & 63, cb = (sl >> 6) % ncb, u = sl / (64 * ncb), ks = u & 1, step = u >> 1, hi = lane >> 5;
    const int r = 32 * cb + conv_row_perm(lane & 31);
    float f[8];
    if (mode == NWP_CAT_BWD) {
      const int t = step % 9, q0 = 32 * (step / 9) + 16 * ks + 8 * hi;
      const float* src = w + ((long)q0 * cin + r) * 9 + (8 - t);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = src[(long)9 * cin * j];
    } else {
      const int nt = mode == NWP_NARROW1 ? 1 : 9;
      const bool p5 = mode == NWP_NARROW3 || (mode == NWP_CAT_FWD && step >= 18);
      const int s = mode == NWP_CAT_FWD ? (step >= 18 ? step - 18 : step % 9) : step;
      const int t2 = 2 * s + ks;
      const bool zero = p5 && t2 > 8;
      const int tap = mode == NWP_NARROW1 ? 0 : p5 ? (t2 > 8 ? 8 : t2) : s;
      const int c0 = p5 ? (mode == NWP_CAT_FWD ? NWP_CIN1 : 0) + 8 * hi : (mode == NWP_CAT_FWD ? 32 * (step / 9) : 0) + 16 * ks + 8 * hi;
      const float sc = fold ? fold[r] : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ci = c0 + j, cc = ci < cin ? ci : 0;
        const float v = sc * w[((long)r * cin + cc) * nt + tap];
        f[j] = ci < cin && !zero ? v : 0.f;
      }
    }
    o = slot_pack<DT>(f);
  }
  *(Slot16*)(out + 8 * slot) = o;
}
}  // namespace rd
