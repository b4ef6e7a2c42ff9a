// Backward primitives of the conv family (16-bit activations, float32 weight gradients): what carries the loss head's d_logit / d_delta
// back through a head tower (rangedet/symbol/head/builder.py:221-255: four 3x3 conv + norm + ReLU layers, then a 1x1 output conv with
// bias; float32 weight gradients as under multi_precision, tools/train.py:358-360).
//   relu_affine_bwd_kernel       dz = g * [y > 0] * s[c], one float32 product rounded once
//   conv3_bwd_weight_kernel      dW[co][ci][tap] = sum over pixels of dz[pix][co] * x[pix + tap][ci] on the matrix cores, partial sums per
//                                workgroup in the workspace;  bwd_weight_reduce_kernel adds them in index order.  SW = 2: the stride-(1,2)
//                                conv of a down-sampling BasicBlock, dz at half width against x[2 pix + tap]
//   conv1_bwd_weight_kernel      the same for a 1x1 conv (the projection shortcut of a backbone BasicBlock): dW[co][ci], one tap, the flat
//                                pixel axis;  bwd1_weight_reduce_kernel adds the partial images in index order
//   head_out_bwd_kernel         the 1x1 output conv: dx (optionally times [x > 0] * s[c], the dz of the last tower conv), and the
//                                partial sums of dw and dbias;  head_out_bwd_reduce_kernel adds them in index order
// (The data gradient of a 3x3 conv is the forward launch on the transposed, flipped weight: rangedet_amd/backward.py.)
// No atomics anywhere: every sum has a fixed order, two calls give the same bits.
//
// Weight gradient as a GEMM: M = cout (A = dz transposed), N = cin (B = x), K = pixels.  Both MFMA operands run along the pixel axis,
// memory is channels-last, so both are transposed on their way into LDS: a thread loads 8 pixels x 8 channels (eight 16-byte loads,
// each load instruction reading whole 128-byte lines), transposes the 8 x 8 block of 16-bit values in registers and stores eight
// 16-byte pieces of [channel][pixel] rows.  The operand fragments are then plain 16-byte row reads (32x32x16: lane l holds
// k = 8 (l >> 5) .. + 8 of row l & 31).  Rows are 64 pixels + 8 of padding = 144 bytes: the sixteen lanes of every ds_read_b128 group
// fall on sixteen different 16-byte slots of the 256-byte bank row, and the eight lanes of a ds_write_b128 group write 128 contiguous
// bytes.
// A workgroup owns one tap COLUMN dw and 64 output channels: the x image is stored shifted by dw (x[w + dw] at column w, zeros outside
// the image), so the three taps of the column are the same dz fragment against three x rows, every read is aligned, and the x rows
// live in a ring of three while the workgroup walks down a strip of BW_RH rows.  The reduction over pixels is split over `S`
// workgroups per (dw, channel block); each takes a contiguous run of (frame, row strip, 64-pixel tile) chunks.
#pragma once
#include "rd_common.h"

namespace rd {
constexpr int BW_PT = 64;            // pixels of a tile: four k-steps of 16
constexpr int BW_RS = BW_PT + 8;     // elements of an LDS row (144 bytes)
constexpr int BW_RH = 16;            // image rows of a chunk (the x ring is refilled with two rows per chunk)
constexpr int BW_COB = 64;           // output channels of a workgroup
constexpr int BW_WG_TARGET = 512;    // workgroups of a launch with the library's own split: two per CU of a 256-CU part

inline long bw_chunks(int B, int H, int W) { return (long)B * ((H + BW_RH - 1) / BW_RH) * ((W + BW_PT - 1) / BW_PT); }
// partial sums per output element: the caller's cap (split > 0) or the library's, never more than there are chunks
inline long bw_split(int B, int H, int W, int cout, int split) {
  const long n = bw_chunks(B, H, W), cap = split > 0 ? split : BW_WG_TARGET / (3 * (cout / BW_COB));
  return n < cap ? n : cap;
}
inline bool bw_weight_shape_ok(int cin, int cout) { return (cin == 64 || cin == 128) && (cout == 64 || cout == 128); }
inline size_t bw_weight_ws_bytes(int B, int H, int W, int cin, int cout, int split) {
  return (size_t)bw_split(B, H, W, cout, split) * 9 * cout * cin * sizeof(float);
}
// The weight gradient of a transposed conv (3, KW) / stride (1, s) / pad (1, p) with KW = 2 s = s + 2 p -- the two forms of the network,
// (3,4)/2/1 and (3,8)/4/2 -- is the same kernel with the two tensors swapped: the NARROW tensor is the deconv input x (B, H, Win, Cin),
// its channels the M axis (the kernel's COUT), the WIDE one is dz (B, H, s Win, Cout) read at pixel stride s with the column offsets
// kw - p, its channels the N axis (the kernel's CIN):  dW[ci][co][kh][kw] = sum x[b,hi,wi,ci] dz[b,hi-1+kh,s wi-p+kw,co] comes out in
// MXNet's (Cin, Cout, 3, KW) layout.  A workgroup owns ONE tap column kw, as in the conv: grid (S, KW, Cin / 64).
inline bool bw_deconv_form_ok(int kw, int s, int p) { return (kw == 4 && s == 2 && p == 1) || (kw == 8 && s == 4 && p == 2); }
inline bool bw_deconv_shape_ok(int cin, int cout, int kw) {   // the four transposed convs of the shipped configs
  return kw == 8 ? (cin == 128 && (cout == 128 || cout == 64)) : ((cin == 128 || cin == 64) && cout == 64);
}
inline long bw_deconv_split(int B, int H, int Win, int cin, int kw, int split) {
  const long n = bw_chunks(B, H, Win), cap = split > 0 ? split : BW_WG_TARGET / (kw * (cin / BW_COB));
  return n < cap ? n : cap;
}
inline size_t bw_deconv_ws_bytes(int B, int H, int Win, int cin, int cout, int kw, int split) {
  return (size_t)bw_deconv_split(B, H, Win, cin, kw, split) * 3 * kw * cin * cout * sizeof(float);
}

struct BwdWArgs {
  const unsigned short *x, *dz;
  int x_cs, x_co, dz_cs, dz_co;
  int B, H, W, nwt, nhs;
  long nchunks;
  float* part;   // [S][9][cout][cin]  (transposed conv: [S][3 KW][Cin][Cout])
  int Wz;        // pixels of a dz row: W (stride 1) or W / SW; tiles, strips and chunks are counted on the dz (narrow) grid
};

// eight pixels p0, p0 + step, .. p0 + 7 step of one image row, 8 channels each.  Every address is clamped into the row and the value
// dropped afterwards: no branch around a load.
__device__ __forceinline__ void bw_load(const unsigned short* __restrict__ row, bool row_ok, int cs, int p0, int W, Slot16 (&v)[8], int step = 1) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int p = p0 + step * j, pc = p < 0 ? 0 : p >= W ? W - 1 : p;
    const Slot16 t = *(const Slot16*)(row + (long)pc * cs);
    const bool ok = row_ok && p == pc;
    v[j] = ok ? t : Slot16{0u, 0u, 0u, 0u};
  }
}
// v[pixel][channel pair] -> eight rows [channel][8 pixels] of an LDS image, at column 8 pg of rows c0 .. c0 + 7
__device__ __forceinline__ void bw_store_t(unsigned short (*T)[BW_RS], int c0, int pg, const Slot16 (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    Slot16 lo, hi;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned a = v[2 * q][k], b = v[2 * q + 1][k];
      lo[q] = (a & 0xffffu) | (b << 16);
      hi[q] = (a >> 16) | (b & 0xffff0000u);
    }
    *(Slot16*)&T[c0 + 2 * k][8 * pg] = lo;
    *(Slot16*)&T[c0 + 2 * k + 1][8 * pg] = hi;
  }
}

// grid (S, 3, COUT / 64), 256 threads.  Waves: CIN 128 -> wave w owns input channels [32 w, 32 w + 32) and both 32-row halves of the
// 64 output channels; CIN 64 -> wave w owns input channels 32 (w & 1) .. and output half w >> 1.
// SW 2: the stride-(1,2) conv (conv2 of a down-sampling BasicBlock).  dz has Wz = W / 2 pixels per row and the tile runs over them; the
// x image of column dw holds x[2 p + dw] at column p (zeros outside the image), i.e. the same eight loads per thread at twice the pixel
// stride.  In a dense image a pixel is one or two whole 128-byte lines, and a load instruction already reads one pixel per eight (or
// sixteen) lanes, so every line fetched is used in full: column 0 reads the even pixels, columns -1 and +1 the odd ones, the pixels of
// the other parity are never touched by that workgroup.  Everything behind the loads is unchanged.
// KW, PW: tap columns and the pad, grid.y = KW, column offset dw = kw - PW (3, 1: the conv).  The transposed convs (above) are SW 2, KW 4,
// PW 1 and SW 4, KW 8, PW 2 with `dz` the deconv input, `x` the deconv output gradient, CIN the deconv's Cout and COUT its Cin: at stride 4 a
// workgroup touches every fourth pixel of the wide tensor -- whole 128-byte lines still -- and the columns kw and kw + 4 read the same ones.
template <int DT, int CIN, int COUT, int SW = 1, int KW = 3, int PW = 1>
__global__ __launch_bounds__(256) void conv3_bwd_weight_kernel(BwdWArgs a) {
  static_assert(SW == 1 || SW == 2 || SW == 4, "stride (1,1), (1,2) or (1,4)");
  constexpr int WN = CIN / 32 < 4 ? CIN / 32 : 4, WM = 4 / WN, MT = 2 / WM;
  constexpr int NXU = (BW_PT / 8) * (CIN / 8), NZU = (BW_PT / 8) * (BW_COB / 8);   // load units of an x row and of a dz row
  static_assert(NXU + NZU <= 256, "one load unit per thread");
  __shared__ __attribute__((aligned(16))) unsigned short Tx[3][CIN][BW_RS];
  __shared__ __attribute__((aligned(16))) unsigned short Tz[BW_COB][BW_RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = gridDim.x, s = blockIdx.x, dw = (int)blockIdx.y - PW, cob = blockIdx.z;
  const int wn = wave % WN, wm = wave / WN;
  const bool is_x = tid < NXU, is_z = tid >= NXU && tid < NXU + NZU;
  const int u = is_x ? tid : tid - NXU;            // unit: pixel group u % 8, channel group u / 8
  const int pg = u & 7, cg = u >> 3;
  f32x16 acc[3][MT];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[d][i][r] = 0.f;

  const long c_lo = s * a.nchunks / S, c_hi = (s + 1) * a.nchunks / S;
  for (long ch = c_lo; ch < c_hi; ++ch) {
    const int wt = (int)(ch % a.nwt), hs = (int)((ch / a.nwt) % a.nhs), b = (int)(ch / ((long)a.nwt * a.nhs));
    const int h0 = hs * BW_RH, h1 = h0 + BW_RH < a.H ? h0 + BW_RH : a.H;
    const int p0 = wt * BW_PT + 8 * pg;
    const unsigned short* xb = a.x + (long)b * a.H * a.W * a.x_cs + a.x_co + 8 * cg;
    const int Wz = SW == 1 ? a.W : a.Wz;
    const unsigned short* zb = a.dz + (long)b * a.H * Wz * a.dz_cs + a.dz_co + cob * BW_COB + 8 * cg;
    Slot16 v[8];
    auto load_x = [&](int r) {      // x row r shifted by dw; rows outside the image are zeros
      const int rc = r < 0 ? 0 : r >= a.H ? a.H - 1 : r;
      bw_load(xb + (long)rc * a.W * a.x_cs, r == rc, a.x_cs, SW * p0 + dw, a.W, v, SW);
    };
    if (is_x) {
      load_x(h0 - 1);
      bw_store_t(Tx[(h0 + 2) % 3], 8 * cg, pg, v);
      load_x(h0);
      bw_store_t(Tx[h0 % 3], 8 * cg, pg, v);
      load_x(h0 + 1);
    } else if (is_z) {
      bw_load(zb + (long)h0 * Wz * a.dz_cs, true, a.dz_cs, p0, Wz, v);
    }
    for (int h = h0; h < h1; ++h) {
      if (is_x) bw_store_t(Tx[(h + 1) % 3], 8 * cg, pg, v);
      else if (is_z) bw_store_t(Tz, 8 * cg, pg, v);
      __syncthreads();
      if (h + 1 < h1) {             // the next row's loads fly during this row's MFMAs
        if (is_x) load_x(h + 2);
        else if (is_z) bw_load(zb + (long)(h + 1) * Wz * a.dz_cs, true, a.dz_cs, p0, Wz, v);
      }
      const int r = lane & 31, k8 = 8 * (lane >> 5);
#pragma unroll
      for (int ks = 0; ks < BW_PT / 16; ++ks) {
        s16x8 af[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) af[i] = *(const s16x8*)&Tz[32 * (wm * MT + i) + r][16 * ks + k8];
#pragma unroll
        for (int d = 0; d < 3; ++d) {   // tap row dh = d - 1: x row h + dh
          const s16x8 bf = *(const s16x8*)&Tx[(h + d + 2) % 3][32 * wn + r][16 * ks + k8];
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[d][i] = H16<DT>::mfma(af[i], bf, acc[d][i]);
        }
      }
      __syncthreads();
    }
  }
  // D[m][n]: column n = lane & 31 (input channel), row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
  const int ci = 32 * wn + (lane & 31);
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int co = cob * BW_COB + 32 * (wm * MT + i) + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);
        a.part[(((long)s * (3 * KW) + (KW * d + dw + PW)) * COUT + co) * CIN + ci] = acc[d][i][rg];
      }
}

// dW (OIHW) = the S partial images added in index order; thread per (tap, co, ci), ci fastest: the reads are coalesced.  nt: taps (9; a
// transposed conv: 3 KW)
__global__ __launch_bounds__(256) void bwd_weight_reduce_kernel(const float* __restrict__ part, int S, int cout, int cin, float* __restrict__ dW,
                                                                int nt) {
  const int n = nt * cout * cin, idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float sum = part[idx];
  for (int k = 1; k < S; ++k) sum += part[(long)k * n + idx];
  const int t = idx / (cout * cin), co = idx / cin % cout, ci = idx % cin;
  dW[((long)co * cin + ci) * nt + t] = sum;
}

// ---- weight gradient of a 1x1 conv (the projection shortcut of a backbone BasicBlock, dla_backbone.py:34-51) --------------------------------
// dW[co][ci] = sum over pixels of dz[pix][co] * x[pix][ci]: the one-tap form of the kernel above.  Without a tap there is no image edge, so
// the pixel axis is the flat run of B H W pixels in tiles of BW_PT; a chunk is one tile, and the last one is clamped and zero-filled.  The
// same register transpose into [channel][pixel] rows and the same fragment reads; no shifted x image, no ring: one x tile and one dz tile
// in LDS, the next chunk's loads in flight during this chunk's MFMAs.
// The kernel is a stream: (cin + cout) * 2 bytes per pixel against cin * cout * 2 multiply-adds, 64 to 128 per byte.  A workgroup
// therefore owns ALL cout x cin outputs (at most sixteen 32 x 32 tiles, four per wave: 64 accumulator registers), so that every input byte
// is read once, and the launch is split over the pixel axis only.  A partial image costs cout * cin * 4 bytes written and read again --
// the bytes of four chunks at 128 x 128 -- so the library's own split gives a workgroup at least BW1_MIN_CHUNKS = 8 chunks (the partial
// sums then move at most half of what the inputs do) and stops at BW_WG_TARGET workgroups, two per CU of a 256-CU part, the most that are
// resident at once with 36 KB of LDS each.
constexpr int BW1_MIN_CHUNKS = 8;

inline long bw1_chunks(int B, int H, int W) { return ((long)B * H * W + BW_PT - 1) / BW_PT; }
inline long bw1_split(int B, int H, int W, int split) {
  const long n = bw1_chunks(B, H, W), own = (n + BW1_MIN_CHUNKS - 1) / BW1_MIN_CHUNKS;
  const long cap = split > 0 ? split : (own < BW_WG_TARGET ? own : BW_WG_TARGET);
  return n < cap ? n : cap;
}
inline size_t bw1_weight_ws_bytes(int B, int H, int W, int cin, int cout, int split) {
  return (size_t)bw1_split(B, H, W, split) * cout * cin * sizeof(float);
}

struct BwdW1Args {
  const unsigned short *x, *dz;
  int x_cs, x_co, dz_cs, dz_co;
  long npix, nchunks;
  float* part;   // [S][cout][cin]
};

// eight pixels p0 .. p0 + 7 of the flat pixel run, 8 channels each; addresses past the end are clamped and the values zeroed
__device__ __forceinline__ void bw1_load(const unsigned short* __restrict__ base, int cs, long p0, long npix, Slot16 (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long p = p0 + j, pc = p < npix ? p : npix - 1;
    const Slot16 t = *(const Slot16*)(base + pc * cs);
    v[j] = p == pc ? t : Slot16{0u, 0u, 0u, 0u};
  }
}

// grid (S), 256 threads.  Waves: CIN 128 -> wave w owns input channels [32 w, 32 w + 32) and every 32-row block of the output channels;
// CIN 64 -> wave w owns input channels 32 (w & 1) .. and the output half w >> 1.
template <int DT, int CIN, int COUT>
__global__ __launch_bounds__(256) void conv1_bwd_weight_kernel(BwdW1Args a) {
  constexpr int WN = CIN / 32 < 4 ? CIN / 32 : 4, WM = 4 / WN, MT = COUT / 32 / WM;
  constexpr int NXU = (BW_PT / 8) * (CIN / 8), NZU = (BW_PT / 8) * (COUT / 8);   // load units of an x tile and of a dz tile
  static_assert(NXU + NZU <= 256, "one load unit per thread");
  __shared__ __attribute__((aligned(16))) unsigned short Tx[CIN][BW_RS];
  __shared__ __attribute__((aligned(16))) unsigned short Tz[COUT][BW_RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = gridDim.x, s = blockIdx.x;
  const int wn = wave % WN, wm = wave / WN;
  const bool is_x = tid < NXU, is_z = tid >= NXU && tid < NXU + NZU;
  const int u = is_x ? tid : tid - NXU;            // unit: pixel group u % 8, channel group u / 8
  const int pg = u & 7, cg = u >> 3;
  f32x16 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const unsigned short* xb = a.x + a.x_co + 8 * cg;
  const unsigned short* zb = a.dz + a.dz_co + 8 * cg;
  const long c_lo = s * a.nchunks / S, c_hi = (s + 1) * a.nchunks / S;
  Slot16 v[8];
  auto load = [&](long ch) {
    const long p0 = ch * BW_PT + 8 * pg;
    if (is_x) bw1_load(xb, a.x_cs, p0, a.npix, v);
    else if (is_z) bw1_load(zb, a.dz_cs, p0, a.npix, v);
  };
  if (c_lo < c_hi) load(c_lo);
  for (long ch = c_lo; ch < c_hi; ++ch) {
    if (is_x) bw_store_t(Tx, 8 * cg, pg, v);
    else if (is_z) bw_store_t(Tz, 8 * cg, pg, v);
    __syncthreads();
    if (ch + 1 < c_hi) load(ch + 1);   // the next chunk's loads fly during this chunk's MFMAs
    const int r = lane & 31, k8 = 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < BW_PT / 16; ++ks) {
      const s16x8 bf = *(const s16x8*)&Tx[32 * wn + r][16 * ks + k8];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const s16x8 af = *(const s16x8*)&Tz[32 * (wm * MT + i) + r][16 * ks + k8];
        acc[i] = H16<DT>::mfma(af, bf, acc[i]);
      }
    }
    __syncthreads();
  }
  // D[m][n]: column n = lane & 31 (input channel), row m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
  const int ci = 32 * wn + (lane & 31);
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int co = 32 * (wm * MT + i) + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);
      a.part[((long)s * COUT + co) * CIN + ci] = acc[i][rg];
    }
}

// dW (cout, cin) = the S partial images added in index order.  There are only cout * cin threads (16 to 64 workgroups) and the sum of a
// thread is one dependent chain, so the launch runs at the latency of its loads: they are issued BW1_RED_BATCH at a time (independent,
// clamped to the last image and the value dropped) and then added one by one in index order.
constexpr int BW1_RED_BATCH = 16;
__global__ __launch_bounds__(256) void bwd1_weight_reduce_kernel(const float* __restrict__ part, int S, int n, float* __restrict__ dW) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  float sum = 0.f;
  for (int k0 = 0; k0 < S; k0 += BW1_RED_BATCH) {
    float v[BW1_RED_BATCH];
#pragma unroll
    for (int j = 0; j < BW1_RED_BATCH; ++j) {
      const int k = k0 + j < S ? k0 + j : S - 1;
      v[j] = part[(long)k * n + idx];
    }
#pragma unroll
    for (int j = 0; j < BW1_RED_BATCH; ++j)
      if (k0 + j < S) sum += v[j];
  }
  dW[idx] = sum;
}

// ---- dz = g * [y > 0] * s[c] -----------------------------------------------------------------------------------------------------------
// one thread per pixel and 8-channel slot; y == nullptr: no mask, scale == nullptr: 1
template <int DT>
__global__ __launch_bounds__(256) void relu_affine_bwd_kernel(const unsigned short* __restrict__ g, int g_cs, int g_co, const unsigned short* __restrict__ y,
                                                              int y_cs, int y_co, const float* __restrict__ scale, unsigned short* __restrict__ dz,
                                                              int dz_cs, int dz_co, long npix, int C) {
  const int slots = C / 8;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= npix * slots) return;
  const long p = i / slots;
  const int c = (int)(i % slots) * 8;
  const Slot16 gv = *(const Slot16*)(g + p * g_cs + g_co + c);
  Slot16 yv = {0u, 0u, 0u, 0u};
  if (y) yv = *(const Slot16*)(y + p * y_cs + y_co + c);
  float gf[8], yf[8];
  slot_unpack<DT>(gv, gf);
  slot_unpack<DT>(yv, yf);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float s = scale ? scale[c + j] : 1.f;
    gf[j] = (!y || yf[j] > 0.f) ? gf[j] * s : 0.f;
  }
  *(Slot16*)(dz + p * dz_cs + dz_co + c) = slot_pack<DT>(gf);
}

// ---- backward of the 1x1 output conv (rd_head_out) ----------------------------------------------------------------------------------------
constexpr int HOB_MAX_BLOCKS = 1024;
constexpr int HOB_MIN_PIXELS = 64;     // pixels of a block before a second block is worth its workspace slot
// (kept apart from k_norm.h's nm_parts, like the final-reduce kernels: they split and add in different orders, merging would change result bits)
inline int hob_blocks(long total) {
  const long nb = (total + HOB_MIN_PIXELS - 1) / HOB_MIN_PIXELS;
  return (int)(nb < 1 ? 1 : nb > HOB_MAX_BLOCKS ? HOB_MAX_BLOCKS : nb);
}
__host__ __device__ inline int hob_slot_floats(int cin) { return 8 * cin + 8; }   // [8][cin] dw, then 8 dbias
inline size_t hob_ws_bytes(long total, int cin) { return (size_t)hob_blocks(total) * hob_slot_floats(cin) * sizeof(float); }

struct HobArgs {
  const float* d_out;
  long obs, n_off, HW, total, per_block;
  const unsigned short* x;
  int x_cs, x_co;
  const float *w, *scale;
  int relu_mask, nout;
  unsigned short* dx;
  int dx_cs, dx_co;
  float* part;
};

// A thread owns one 8-channel slot and every (256 / slots)-th pixel of the block's run: dx of its slot per pixel, and nout x 8 running
// sums of d_out * x in float32.  The block adds its pixel lanes in index order through LDS and writes one workspace slot.
template <int DT, int CIN>
__global__ __launch_bounds__(256) void head_out_bwd_kernel(HobArgs a) {
  constexpr int CG = CIN / 8, PL = 256 / CG;
  __shared__ float red[PL][CIN];
  __shared__ float redb[PL];
  const int tid = threadIdx.x, cg = tid % CG, pl = tid / CG;
  float wr[8][8], sc[8], acc[8][8], accb[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    accb[o] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wr[o][j] = o < a.nout ? a.w[o * CIN + cg * 8 + j] : 0.f;
      acc[o][j] = 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] = a.scale ? a.scale[cg * 8 + j] : 1.f;
  const long g0 = blockIdx.x * a.per_block, g1 = g0 + a.per_block < a.total ? g0 + a.per_block : a.total;
  for (long g = g0 + pl; g < g1; g += PL) {
    const long b = g / a.HW, p = g % a.HW;
    const float* d = a.d_out + b * a.obs + (a.n_off + p) * a.nout;
    float dv[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) dv[o] = o < a.nout ? d[o] : 0.f;
    const Slot16 xv = *(const Slot16*)(a.x + g * a.x_cs + a.x_co + cg * 8);
    float xf[8], r[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // (not slot_unpack: through it the bf16 form compiles to a longer loop, measured 0.8 % slower)
      const f32x2_t_ t = H16<DT>::unpk(xv[k]);
      xf[2 * k] = t[0];
      xf[2 * k + 1] = t[1];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = 0.f;
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (o < a.nout) {
        accb[o] += dv[o];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          r[j] = fmaf(dv[o], wr[o][j], r[j]);
          acc[o][j] = fmaf(dv[o], xf[j], acc[o][j]);
        }
      }
    if (a.dx) {
      Slot16 ov;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float r0 = r[2 * k], r1 = r[2 * k + 1];
        if (a.relu_mask) { r0 = xf[2 * k] > 0.f ? r0 : 0.f; r1 = xf[2 * k + 1] > 0.f ? r1 : 0.f; }
        if (a.scale) { r0 *= sc[2 * k]; r1 *= sc[2 * k + 1]; }
        ov[k] = H16<DT>::pk(r0, r1);
      }
      *(Slot16*)(a.dx + g * a.dx_cs + a.dx_co + cg * 8) = ov;
    }
  }
  float* slot = a.part + (long)blockIdx.x * hob_slot_floats(CIN);
#pragma unroll
  for (int o = 0; o < 8; ++o)
    if (o < a.nout) {       // uniform over the block: the barriers are not divergent
#pragma unroll
      for (int j = 0; j < 8; ++j) red[pl][cg * 8 + j] = acc[o][j];
      if (cg == 0) redb[pl] = accb[o];
      __syncthreads();
      if (tid < CIN) slot[o * CIN + tid] = lane_sum(&red[0][0], PL, CIN, tid);
      else if (tid == CIN) slot[8 * CIN + o] = lane_sum(redb, PL, 1, 0);
      __syncthreads();
    }
}
// dw (nout, cin) and dbias (nout): the blocks' slots added in index order
__global__ __launch_bounds__(256) void head_out_bwd_reduce_kernel(const float* __restrict__ part, int nblocks, int cin, int nout,
                                                                  float* __restrict__ dw, float* __restrict__ dbias) {
  const int idx = blockIdx.x * 256 + threadIdx.x, slotf = hob_slot_floats(cin);
  if (idx >= nout * cin + nout) return;
  const int off = idx < nout * cin ? idx : 8 * cin + (idx - nout * cin);
  float sum = part[off];
  for (int k = 1; k < nblocks; ++k) sum += part[(long)k * slotf + off];
  if (idx < nout * cin) dw[idx] = sum;
  else dbias[idx - nout * cin] = sum;
}
}  // namespace rd
