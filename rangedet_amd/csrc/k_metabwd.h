// Backward of the fused Meta-Kernel unit (k_meta.h) for gfx950, RD_BF16 / RD_F16, with the folded (inference-mode) normalisation s1, t1:
// the gradient of the function rd_meta_kernel_fwd computes, up to z (dz = dL/dz comes from rd_relu_affine_bwd).  Per pixel p, tap k
// (n_k = p + d_k), data channel c, hidden unit j, output channel o -- the forward, then the backward:
//   rel_k = coord[n_k] - coord[p]       u_k = W0 rel_k + b0        h_k = relu(u_k)        w_k = (s1 W1)_k h_k + s1 b1
//   r_k = data[n_k] w_k + t1            a_k = relu(r_k)            z = sum_{c,k} A[o, c 9 + k] a_k[c]
//   da_k = A_k^T dz                     dr_k = da_k [r_k > 0]      dA = sum_p dz (x) a_k
//   dt1 = sum_p dr_k                    dq1 = sum_p dr_k (r_k - t1)
//   e_k = dr_k data[n_k]                dW1[c,j] = sum_k s1[c,k] sum_p e_k[c] h_k[j]     db1[c] = sum_k s1[c,k] sum_p e_k[c]
//   du_k[j] = [u_k[j] > 0] sum_c (s1 W1)_k[c,j] e_k[c]             dW0[j,i] = sum_{p,k} du_k[j] rel_k[i]     db0[j] = sum_{p,k} du_k[j]
//   ddata[p',c] = sum_k (w_k [r_k > 0] da_k)(p' - d_k)[c]          (pixels p' - d_k inside the image)
// Neither kernel writes a per-pixel 576-channel tensor: w_k, r_k, a_k are recomputed per pixel fragment and stay in registers / LDS.
//
// meta_bwd_data_kernel   gather form: a lane owns the output pixel p' and walks the nine source pixels q = p' - d_k.  r_k(q) needs only
//                        data[p'] and coord[p'] - coord[q], so the kernel is the forward's shape: MFMA #1 gives w_k (lane = pixel, registers =
//                        channels), a per-tap 64 x 64 product A_k^T dz[q] on the matrix cores gives da_k in the SAME register layout, and
//                        the element-wise product and the sum over taps stay in float32 registers.  dz[q] is read as zeros outside the
//                        image, which makes da_k = 0 there: no scatter, no atomics, no bounds logic behind the loads.  An optional
//                        residual is added in float32 before the one rounding of ddata.
//                        512 threads = 8 waves, a wave owns one FRAGMENT of 32 consecutive pixels of an image row; W1 and A^T fragments of
//                        all nine taps (108 KiB) and the per-tap constants live in LDS, workgroups are persistent over runs of 8 fragments.
// meta_bwd_params_kernel grid (S, 9): a workgroup owns ONE tap k and a contiguous run of chunks (4 fragments = 128 pixels), so the tap's
//                        MFMA operands (W1_k, A_k^T, W1_k^T: 16 KiB) and constants sit in LDS once and the accumulators of a workgroup are
//                        64 x 64 (dA_k) + 64 x 32 (dW1's tap term) values.  Per chunk: the forward of the tap and da_k per pixel lane as in the
//                        data kernel; dt1, dq1, sum e, dW0 and db0 accumulate per lane in float32 registers; dz, a_k, e_k and h_k go
//                        through LDS as [channel][pixel] rows (the transpose that puts the PIXEL axis on the MFMA's K axis) and two
//                        products on the matrix cores add dA_k += dz^T a_k and E_k += e_k^T h_k.  At the end the lanes' sums are added in
//                        lane order through LDS and the workgroup writes one partial of MB_PART floats.
// meta_bwd_reduce_kernel adds the S partials of every tap in index order, applies s1[c,k] to the dW1 / db1 tap terms and adds the taps in
//                        index order.  The CENTRE tap (rel = 0: pack_meta folds w_4 = s1 (W1 relu(b0) + b1) into a constant, in double) has
//                        no MLP launch work at all: its terms follow exactly from P4[c] = sum_p e_4[p,c] here:
//                          dW1[c,j] += s1[c,4] relu(b0[j]) P4[c]     db1[c] += s1[c,4] P4[c]     db0[j] += [b0[j] > 0] sum_c s1[c,4] W1[c,j] P4[c]
//                        and dW0 gets nothing from it.
// No atomics; every sum has a fixed order that depends on the shape and on `split` only (never on the CU count): two calls give the same bytes.
//
// ARITHMETIC CONTRACT -- every point where a value is rounded to the 16-bit type (everything else is float32; MFMA accumulation is float32):
//   (1) h_k = relu(round(u_k)), u_k in float32 from float32 coordinates and W0, b0 (both kernels; as the forward, whose u is fp32-accurate)
//   (2) (s1 W1)_k[c,j] = round(float(s1[c,k]) * W1[c,j]) and (3) A = round(A): the PACKER's values, the ones rd_pack_meta_host makes
//   (4) a_k = relu(round(r_k)) as the B operand of dA (params kernel only; the masks [r_k > 0] test the float32 r_k)
//   (5) e_k = round(dr_k * data[n_k]) as the operand of the dW1 product and of du_k (params kernel; db1 and P4 sum the float32 e_k)
//   (6) ddata = round(sum + residual), once (data kernel)
// The centre tap's w_4 is the packer's float32 constant; dz and data are 16-bit inputs.  [u_k > 0] tests the float32 u_k.
// TRAINING FORM (k_metatrain.h: batch statistics; blocks packed with s1 = 1, t1 = 0; q_k = data[n_k] * w_k, r_k = fmaf(q_k, a1, bb1),
// dq_k = a1 * fmaf(-xh_k, c2, gy_k - c1)) -- its 16-bit rounding points, everything else float32:
//   (1) as above; (2) round(W1) and (3) round(A): the packer's values with s1 = 1
//   (4t) a_k = relu(round(r_k)) as the B operand of z (training forward) and of dA (pass A); the masks [r_k > 0] test the float32 r_k
//   (5t) e_k = round(dq_k * data[n_k]) as the operand of the dW1 product and of du_k (pass B; db1 and P4 sum the float32 e_k)
//   (6) ddata = round(sum + residual), once; (7t) z = round(float32 sum), once (training forward)
#pragma once
#include "k_meta.h"

namespace rd {

struct MetaBwdLayout {   // byte offsets inside the packed block of the backward
  size_t w1s, at, w1t, b1s, t1, s1, w0, w1raw, total;
  size_t wbytes;         // w1s + at: what the data kernel holds in LDS
};
__host__ __device__ constexpr MetaBwdLayout meta_bwd_layout() {
  MetaBwdLayout L{};
  L.w1s = 0;                               // [k][mt][ks][lane][8]  A operand of MFMA #1 (k_meta.h's own order)
  L.at = L.w1s + 9 * 2 * 2 * 64 * 16;      // [k][mt][ko][lane][8]  A operand of da = A_k^T dz: row = channel, K = output channel
  L.wbytes = L.at + 9 * 2 * 4 * 64 * 16;
  L.w1t = L.wbytes;                        // [k][kc][lane][8]      A operand of du = (s1 W1)_k^T e: row = hidden unit, K = channel
  L.b1s = L.w1t + 9 * 4 * 64 * 16;         // [k][c] float32: s1 b1 (centre tap: the folded w_4), then t1 [k][c], s1 [k][c]
  L.t1 = L.b1s + 9 * 64 * 4;
  L.s1 = L.t1 + 9 * 64 * 4;
  L.w0 = L.s1 + 9 * 64 * 4;                // [j][4] float32: W0[j][0..2], b0[j]
  L.w1raw = L.w0 + 32 * 4 * 4;             // [c][j] float32: W1 itself (the centre tap's db0 term)
  L.total = L.w1raw + 64 * 32 * 4;
  return L;
}
// lane (pixel, hi) of a fragment holds hidden units MB_J(r, hi), r < 16 (the D rows of a 32x32 MFMA), and channels 32 mt + 16 hi + r
__host__ __device__ constexpr int mb_j(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

inline void pack_meta_bwd(const float* w0, const float* b0, const float* w1, const float* b1, const float* s1, const float* t1,
                          const float* agg, int dt, void* out) {
  constexpr MetaBwdLayout L = meta_bwd_layout();
  unsigned char* base = (unsigned char*)out;
  memset(base, 0, L.total);
  auto w1s16 = [&](int k, int c, int j) { return h16_from_f32(dt, s1[c * 9 + k] * w1[c * 32 + j]); };   // the forward packer's product
  unsigned short* pw1 = (unsigned short*)(base + L.w1s);
  unsigned short* pat = (unsigned short*)(base + L.at);
  unsigned short* pwt = (unsigned short*)(base + L.w1t);
  for (int k = 0; k < 9; ++k)
    for (int lane = 0; lane < 64; ++lane) {
      const int m = lane & 31, hi = lane >> 5;
      for (int e = 0; e < 8; ++e) {
        for (int mt = 0; mt < 2; ++mt) {
          const int c = meta_perm(mt, m);
          for (int ks = 0; ks < 2; ++ks)
            pw1[((((size_t)k * 2 + mt) * 2 + ks) * 64 + lane) * 8 + e] = w1s16(k, c, mb_j(8 * ks + e, hi));
          for (int ko = 0; ko < 4; ++ko)
            pat[((((size_t)k * 2 + mt) * 4 + ko) * 64 + lane) * 8 + e] = h16_from_f32(dt, agg[(size_t)(16 * ko + 8 * hi + e) * 576 + c * 9 + k]);
        }
        for (int kc = 0; kc < 4; ++kc)
          pwt[(((size_t)k * 4 + kc) * 64 + lane) * 8 + e] = w1s16(k, 32 * (kc >> 1) + 16 * hi + 8 * (kc & 1) + e, m);
      }
    }
  float* fb1 = (float*)(base + L.b1s);
  float* ft1 = (float*)(base + L.t1);
  float* fs1 = (float*)(base + L.s1);
  for (int k = 0; k < 9; ++k)
    for (int c = 0; c < 64; ++c) {
      double w = b1[c];                    // (pack_meta: the centre tap's dynamic weight is a constant, folded in double)
      if (k == META_CENTRE_TAP)
        for (int j = 0; j < 32; ++j) w += (double)w1[c * 32 + j] * (double)(b0[j] > 0.f ? b0[j] : 0.f);
      fb1[k * 64 + c] = (float)((double)s1[c * 9 + k] * w);
      ft1[k * 64 + c] = t1[c * 9 + k];
      fs1[k * 64 + c] = s1[c * 9 + k];
    }
  float* fw0 = (float*)(base + L.w0);
  for (int j = 0; j < 32; ++j) {
    fw0[j * 4 + 0] = w0[j * 3 + 0]; fw0[j * 4 + 1] = w0[j * 3 + 1]; fw0[j * 4 + 2] = w0[j * 3 + 2]; fw0[j * 4 + 3] = b0[j];
  }
  memcpy(base + L.w1raw, w1, 64 * 32 * sizeof(float));
}

struct MetaBwdArgs {
  const unsigned short *dz, *data, *res;
  int z_cs, z_co, d_cs, d_co, r_cs, r_co;
  const float* coord;            // NCHW (B,3,H,W)
  const unsigned char* packed;
  unsigned short* ddata; int g_cs, g_co;
  int B, H, W, nfw;              // nfw: fragments (32 pixels) of an image row
  long nfrag, nchunks;
  float* part;                   // params: [S][9][MB_PART]
};

constexpr int MB_DATA_WAVES = 8;                       // data kernel: fragments of a run
constexpr int MB_WAVES = 4, MB_PT = 32 * MB_WAVES;     // params kernel: fragments / pixels of a chunk
constexpr int MB_RS = MB_PT + 8;                       // elements of an LDS row: 272 bytes, 17 x 16 (conflict-free 16-byte row reads)
constexpr int MB_SPLIT = 64;                           // partials per tap with the library's own split: 576 workgroups
// floats of one partial (one tap of one split slot): dA_k [64 o][64 c], E_k [64 c][32 j], dt1 [64], dq1 [64], sum e [64], [32 j][4]: dW0, db0
constexpr int MB_OFF_E = 4096, MB_OFF_T1 = 6144, MB_OFF_Q1 = 6208, MB_OFF_B1 = 6272, MB_OFF_W0 = 6336, MB_PART = 6464;
constexpr int MB_NOUT = 64 * 576 + 64 * 32 + 64 + 32 * 3 + 32 + 576 + 576;   // gradient floats in all

inline long mb_frags(int B, int H, int W) { return (long)B * H * ((W + 31) / 32); }
inline long mb_chunks(int B, int H, int W) { return (mb_frags(B, H, W) + MB_WAVES - 1) / MB_WAVES; }
inline long mb_split(int B, int H, int W, int split) {
  const long n = mb_chunks(B, H, W), cap = split > 0 ? split : MB_SPLIT;
  return n < cap ? n : cap;
}
inline size_t mb_ws_bytes(int B, int H, int W, int split) { return (size_t)mb_split(B, H, W, split) * 9 * MB_PART * sizeof(float); }

struct MetaBwdDataLds {
  static constexpr size_t W_B = meta_bwd_layout().wbytes;                                  // 108 KiB
  static constexpr size_t CONST_B = meta_bwd_layout().w1raw - meta_bwd_layout().b1s;       // b1s, t1, s1, W0: 7.25 KiB
  static constexpr size_t WEIGHTS = 0, CONSTS = W_B, TOTAL = CONSTS + CONST_B;
};
struct MetaBwdParamsLds {
  static constexpr size_t T_B = (size_t)(64 * 3 + 32) * MB_RS * 2;                          // Tz, Ta, Te [64][MB_RS], Th [32][MB_RS]
  static constexpr size_t FRAG_B = 4096 + 8192 + 4096;                                      // W1_k, A_k^T, W1_k^T
  static constexpr size_t CONST_B = 256 + 256 + 512;                                        // b1s_k, t1_k, W0
  static constexpr size_t T = 0, FRAGS = T_B, CONSTS = FRAGS + FRAG_B, TOTAL = CONSTS + CONST_B;
};
static_assert(MetaBwdDataLds::TOTAL <= 160 * 1024 && 2 * MetaBwdParamsLds::TOTAL <= 160 * 1024, "LDS budget of the Meta-Kernel backward");
static_assert((size_t)MB_PT * 64 * sizeof(float) <= MetaBwdParamsLds::T_B, "the lane-sum buffer reuses the transpose rows");

// fragment f -> image row (b H + h) and first column; the pixel of lane px
struct MbPixel { int b, h, w; bool live; };
__device__ __forceinline__ MbPixel mb_pixel(const MetaBwdArgs& a, long f, int px) {
  MbPixel p;
  const long row = f / a.nfw;
  p.w = (int)(f - row * a.nfw) * 32 + px;
  p.b = (int)(row / a.H);
  p.h = (int)(row - (long)p.b * a.H);
  p.live = f < a.nfrag && p.w < a.W;
  return p;
}
// u = W0 rel + b0 for the lane's 16 hidden units (float32), and relu(round(u)) as the two B fragments of MFMA #1
template <int DT>
__device__ __forceinline__ void mb_hidden(const float* w0l, int hi, float r0, float r1, float r2, float (&u)[16], s16x8 (&hf)[2]) {
  typedef short s16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const f32x4 wq = *(const f32x4*)(w0l + mb_j(r, hi) * 4);
    u[r] = fmaf(wq[0], r0, fmaf(wq[1], r1, fmaf(wq[2], r2, wq[3])));
  }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    unsigned pk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned v = H16<DT>::pk(u[8 * ks + 2 * e], u[8 * ks + 2 * e + 1]);
      pk[e] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), (s16x2){0, 0}));
    }
    memcpy(&hf[ks], pk, 16);
  }
}
__device__ __forceinline__ f32x16 mb_load16(const float* p) {
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 t = *(const f32x4*)(p + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
  }
  return v;
}
__device__ __forceinline__ const float* mb_coord(const MetaBwdArgs& a, int b, int h, int w) {
  return a.coord + (size_t)b * 3 * a.H * a.W + (size_t)h * a.W + w;
}

// ---- data gradient -------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MB_DATA_WAVES * 64) void meta_bwd_data_kernel(MetaBwdArgs a) {
  using HT = H16<DT>;
  using L = MetaBwdDataLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_DATA_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned char* lw = smem + L::WEIGHTS;
  float* lc = (float*)(smem + L::CONSTS);
  const float* cb1 = lc;                    // [9][64]
  const float* ct1 = lc + 9 * 64;           // [9][64]
  const float* cw0 = lc + 3 * 9 * 64;       // [32][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5;
  for (size_t i = tid; i < L::W_B / 16; i += NT) ((Slot16*)lw)[i] = ((const Slot16*)a.packed)[i];
  for (size_t i = tid; i < L::CONST_B / 16; i += NT) ((Slot16*)lc)[i] = ((const Slot16*)(a.packed + P.b1s))[i];
  __syncthreads();
  const unsigned char* w1l = lw + P.w1s + lane * 16;
  const unsigned char* atl = lw + P.at + lane * 16;
  const size_t HW = (size_t)a.H * a.W;

  for (long run = blockIdx.x; run < a.nchunks; run += gridDim.x) {
    const long f = run * MB_DATA_WAVES + wave;
    if (f >= a.nfrag) continue;             // (uniform over the wave; there is no barrier in this loop)
    const MbPixel p = mb_pixel(a, f, px);
    const size_t pix = ((size_t)p.b * a.H + p.h) * a.W + p.w;
    float x[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        Slot16 v = {0u, 0u, 0u, 0u};
        if (p.live) v = *(const Slot16*)(a.data + pix * a.d_cs + a.d_co + 32 * mt + 16 * hi + 8 * s);
        float t[8];
        slot_unpack<DT>(v, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[mt][8 * s + e] = t[e];
      }
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (p.live) {
      const float* cp = mb_coord(a, p.b, p.h, p.w);
      c0 = cp[0]; c1 = cp[HW]; c2 = cp[2 * HW];
    }
    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    // (one tap per trip, not unrolled: unrolled, the nine taps' loads are hoisted and the kernel spills ~2.9 KB per lane to scratch)
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      const int qh = p.h - (k / 3 - 1), qw = p.w - (k % 3 - 1);    // the pixel whose tap k reads p'
      const bool inq = p.live && (unsigned)qh < (unsigned)a.H && (unsigned)qw < (unsigned)a.W;
      const size_t qpix = ((size_t)p.b * a.H + qh) * a.W + qw;
      s16x8 zf[4];
#pragma unroll
      for (int ko = 0; ko < 4; ++ko) {
        Slot16 v = {0u, 0u, 0u, 0u};      // outside the image dz is zero: da = 0, the tap adds nothing
        if (inq) v = *(const Slot16*)(a.dz + qpix * a.z_cs + a.z_co + 16 * ko + 8 * hi);
        zf[ko] = __builtin_bit_cast(s16x8, v);
      }
      s16x8 hf[2] = {};
      if (k != META_CENTRE_TAP) {
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
        if (inq) {
          const float* cq = mb_coord(a, p.b, qh, qw);
          q0 = cq[0]; q1 = cq[HW]; q2 = cq[2 * HW];
        }
        float u[16];
        mb_hidden<DT>(cw0, hi, c0 - q0, c1 - q1, c2 - q2, u, hf);   // rel of q's tap k: coord[q + d_k] - coord[q]
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x16 w = mb_load16(cb1 + k * 64 + 32 * mt + 16 * hi);
        if (k != META_CENTRE_TAP) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) w = HT::mfma(*(const s16x8*)(w1l + ((k * 2 + mt) * 2 + ks) * 1024), hf[ks], w);
        }
        f32x16 da;
#pragma unroll
        for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
        for (int ko = 0; ko < 4; ++ko) da = HT::mfma(*(const s16x8*)(atl + ((k * 2 + mt) * 4 + ko) * 1024), zf[ko], da);
        const f32x16 t1v = mb_load16(ct1 + k * 64 + 32 * mt + 16 * hi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float rr = fmaf(x[mt][r], w[r], t1v[r]);
          acc[mt][r] = fmaf(rr > 0.f ? w[r] : 0.f, da[r], acc[mt][r]);
        }
      }
    }
    if (p.live) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int c = 32 * mt + 16 * hi + 8 * s;
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = acc[mt][8 * s + e];
          if (a.res) {
            float rv[8];
            slot_unpack<DT>(*(const Slot16*)(a.res + pix * a.r_cs + a.r_co + c), rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += rv[e];
          }
          *(Slot16*)(a.ddata + pix * a.g_cs + a.g_co + c) = slot_pack<DT>(o);
        }
    }
  }
}

// ---- parameter gradients -----------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MB_WAVES * 64) void meta_bwd_params_kernel(MetaBwdArgs a) {
  using HT = H16<DT>;
  using L = MetaBwdParamsLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned short (*Tz)[MB_RS] = (unsigned short (*)[MB_RS])(smem + L::T);   // [64 o][pixel]
  unsigned short (*Ta)[MB_RS] = Tz + 64;                                    // [64 c][pixel]
  unsigned short (*Te)[MB_RS] = Ta + 64;                                    // [64 c][pixel]
  unsigned short (*Th)[MB_RS] = Te + 64;                                    // [32 j][pixel]
  float* red = (float*)(smem + L::T);                                       // [MB_PT][64], after the chunk loop
  unsigned char* lf = smem + L::FRAGS;
  float* lc = (float*)(smem + L::CONSTS);
  const float* cb1 = lc;          // [64]
  const float* ct1 = lc + 64;     // [64]
  const float* cw0 = lc + 128;    // [32][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5, pl = wave * 32 + px;
  const int S = gridDim.x, s = blockIdx.x, k = blockIdx.y;
  const bool centre = k == META_CENTRE_TAP;
  const int dh = k / 3 - 1, dw = k % 3 - 1;
  for (int i = tid; i < 256; i += NT) ((Slot16*)lf)[i] = ((const Slot16*)(a.packed + P.w1s + (size_t)k * 4096))[i];
  for (int i = tid; i < 512; i += NT) ((Slot16*)(lf + 4096))[i] = ((const Slot16*)(a.packed + P.at + (size_t)k * 8192))[i];
  for (int i = tid; i < 256; i += NT) ((Slot16*)(lf + 12288))[i] = ((const Slot16*)(a.packed + P.w1t + (size_t)k * 4096))[i];
  if (tid < 64) {
    lc[tid] = ((const float*)(a.packed + P.b1s))[k * 64 + tid];
    lc[64 + tid] = ((const float*)(a.packed + P.t1))[k * 64 + tid];
  }
  if (tid < 128) lc[128 + tid] = ((const float*)(a.packed + P.w0))[tid];
  __syncthreads();
  const unsigned char* w1l = lf + lane * 16;             // + (mt * 2 + ks) * 1024
  const unsigned char* atl = lf + 4096 + lane * 16;      // + (mt * 4 + ko) * 1024
  const unsigned char* wtl = lf + 12288 + lane * 16;     // + kc * 1024
  const size_t HW = (size_t)a.H * a.W;

  float st1[2][16], sq1[2][16], se[2][16], sw0[16][4];
  f32x16 accA, accE;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accA[r] = accE[r] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) st1[mt][r] = sq1[mt][r] = se[mt][r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sw0[r][i] = 0.f;
  }

  const long c_lo = s * a.nchunks / S, c_hi = (s + 1) * a.nchunks / S;
  for (long ch = c_lo; ch < c_hi; ++ch) {
    const MbPixel p = mb_pixel(a, ch * MB_WAVES + wave, px);
    const int nh = p.h + dh, nw = p.w + dw;
    const bool nin = p.live && (unsigned)nh < (unsigned)a.H && (unsigned)nw < (unsigned)a.W;
    const size_t pix = ((size_t)p.b * a.H + p.h) * a.W + p.w, npix = ((size_t)p.b * a.H + nh) * a.W + nw;
    s16x8 zf[4];
#pragma unroll
    for (int ko = 0; ko < 4; ++ko) {
      Slot16 v = {0u, 0u, 0u, 0u};        // a lane past the image or the last fragment carries dz = 0: it adds nothing to any sum
      if (p.live) v = *(const Slot16*)(a.dz + pix * a.z_cs + a.z_co + 16 * ko + 8 * hi);
      zf[ko] = __builtin_bit_cast(s16x8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) Tz[16 * ko + 8 * hi + e][pl] = (unsigned short)zf[ko][e];
    }
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, u[16];
    s16x8 hf[2] = {};
    if (!centre) {
      float c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
      if (p.live) { const float* cp = mb_coord(a, p.b, p.h, p.w); c0 = cp[0]; c1 = cp[HW]; c2 = cp[2 * HW]; }
      if (nin) { const float* cn = mb_coord(a, p.b, nh, nw); n0 = cn[0]; n1 = cn[HW]; n2 = cn[2 * HW]; }   // zero padding outside
      r0 = n0 - c0; r1 = n1 - c1; r2 = n2 - c2;
      mb_hidden<DT>(cw0, hi, r0, r1, r2, u, hf);
#pragma unroll
      for (int r = 0; r < 16; ++r) Th[mb_j(r, hi)][pl] = (unsigned short)hf[r >> 3][r & 7];
    }
    s16x8 ef[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      float x[16];
#pragma unroll
      for (int sl = 0; sl < 2; ++sl) {
        Slot16 v = {0u, 0u, 0u, 0u};      // a padded tap reads data = 0: r = t1
        if (nin) v = *(const Slot16*)(a.data + npix * a.d_cs + a.d_co + 32 * mt + 16 * hi + 8 * sl);
        float t[8];
        slot_unpack<DT>(v, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[8 * sl + e] = t[e];
      }
      f32x16 w = mb_load16(cb1 + 32 * mt + 16 * hi);
      if (!centre) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) w = HT::mfma(*(const s16x8*)(w1l + (mt * 2 + ks) * 1024), hf[ks], w);
      }
      f32x16 da;
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
      for (int ko = 0; ko < 4; ++ko) da = HT::mfma(*(const s16x8*)(atl + (mt * 4 + ko) * 1024), zf[ko], da);
      const f32x16 t1v = mb_load16(ct1 + 32 * mt + 16 * hi);
      unsigned short e16[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float xw = x[r] * w[r], rr = fmaf(x[r], w[r], t1v[r]);
        const float dr = rr > 0.f ? da[r] : 0.f, ev = dr * x[r];
        st1[mt][r] += dr;
        sq1[mt][r] = fmaf(dr, xw, sq1[mt][r]);
        se[mt][r] += ev;
        const unsigned short a16 = HT::from_f32(rr);
        e16[r] = HT::from_f32(ev);
        const int c = 32 * mt + 16 * hi + r;
        Ta[c][pl] = (short)a16 < 0 ? (unsigned short)0 : a16;
        Te[c][pl] = e16[r];
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int e = 0; e < 8; ++e) ef[2 * mt + sl][e] = (short)e16[8 * sl + e];
    }
    if (!centre) {
      f32x16 du;
#pragma unroll
      for (int r = 0; r < 16; ++r) du[r] = 0.f;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) du = HT::mfma(*(const s16x8*)(wtl + kc * 1024), ef[kc], du);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = u[r] > 0.f ? du[r] : 0.f;
        sw0[r][0] = fmaf(d, r0, sw0[r][0]);
        sw0[r][1] = fmaf(d, r1, sw0[r][1]);
        sw0[r][2] = fmaf(d, r2, sw0[r][2]);
        sw0[r][3] += d;
      }
    }
    __syncthreads();
    {   // the pixel axis as K: dA_k[o][c] += sum_p dz[p][o] a[p][c], wave = one 32 x 32 tile; E_k[c][j] += sum_p e[p][c] h[p][j] on waves 0, 1
      const int m = lane & 31, k8 = 8 * hi, ot = wave >> 1, ct = wave & 1;
#pragma unroll
      for (int ks = 0; ks < MB_PT / 16; ++ks)
        accA = HT::mfma(*(const s16x8*)&Tz[32 * ot + m][16 * ks + k8], *(const s16x8*)&Ta[32 * ct + m][16 * ks + k8], accA);
      if (!centre && wave < 2) {
#pragma unroll
        for (int ks = 0; ks < MB_PT / 16; ++ks)
          accE = HT::mfma(*(const s16x8*)&Te[32 * wave + m][16 * ks + k8], *(const s16x8*)&Th[m][16 * ks + k8], accE);
      }
    }
    __syncthreads();
  }

  float* part = a.part + ((size_t)s * 9 + k) * MB_PART;
  {   // D[m][n]: column n = lane & 31, row m = mb_j(reg, hi)
    const int n = lane & 31, ot = wave >> 1, ct = wave & 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      part[(32 * ot + mb_j(r, hi)) * 64 + 32 * ct + n] = accA[r];
      if (!centre && wave < 2) part[MB_OFF_E + (32 * wave + mb_j(r, hi)) * 32 + n] = accE[r];
    }
  }
  // the lanes' float32 sums, added in lane order
  auto lane_reduce = [&](const float (&v)[2][16], int off) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[pl * 64 + 32 * mt + 16 * hi + r] = v[mt][r];
    __syncthreads();
    if (tid < 64) part[off + tid] = lane_sum(red, MB_PT, 64, tid);
    __syncthreads();
  };
  lane_reduce(st1, MB_OFF_T1);
  lane_reduce(sq1, MB_OFF_Q1);
  lane_reduce(se, MB_OFF_B1);
  if (!centre) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {   // hidden units 16 half .. + 16: registers 8 half .. + 8 of both lane halves
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[pl * 64 + (mb_j(8 * half + r, hi) & 15) * 4 + i] = sw0[8 * half + r][i];
      __syncthreads();
      if (tid < 64) part[MB_OFF_W0 + 64 * half + tid] = lane_sum(red, MB_PT, 64, tid);
      __syncthreads();
    }
  }
}

// One thread per gradient float: the S partials of a tap in index order, then (dW1, db1, dW0, db0) the taps in index order.
struct MetaBwdOut { float *dA, *dW1, *db1, *dW0, *db0, *dt1, *dq1; };
__device__ __forceinline__ float mb_sum(const float* part, int S, int k, int off) {
  _Pragma("clang fp contract(off)")
  float sum = part[(size_t)k * MB_PART + off];
  for (int s = 1; s < S; ++s) sum += part[((size_t)s * 9 + k) * MB_PART + off];
  return sum;
}
__global__ __launch_bounds__(256) void meta_bwd_reduce_kernel(const float* __restrict__ part, int S, const unsigned char* __restrict__ packed,
                                                              MetaBwdOut o) {
  constexpr MetaBwdLayout P = meta_bwd_layout();
  const float* s1 = (const float*)(packed + P.s1);       // [k][c]
  const float* w0 = (const float*)(packed + P.w0);       // [j][4]
  const float* w1 = (const float*)(packed + P.w1raw);    // [c][j]
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 64 * 576) {                                  // dA[o][c 9 + k]
    const int oc = idx / 576, ck = idx - oc * 576, c = ck / 9, k = ck - c * 9;
    o.dA[idx] = mb_sum(part, S, k, oc * 64 + c);
    return;
  }
  idx -= 64 * 576;
  if (idx < 64 * 32) {                                   // dW1[c][j]
    const int c = idx >> 5, j = idx & 31;
    float acc = 0.f;
    for (int k = 0; k < 9; ++k) {
      const float t = k == META_CENTRE_TAP ? fmaxf(w0[j * 4 + 3], 0.f) * mb_sum(part, S, k, MB_OFF_B1 + c) : mb_sum(part, S, k, MB_OFF_E + c * 32 + j);
      acc = fmaf(s1[k * 64 + c], t, acc);
    }
    o.dW1[idx] = acc;
    return;
  }
  idx -= 64 * 32;
  if (idx < 64) {                                        // db1[c]
    float acc = 0.f;
    for (int k = 0; k < 9; ++k) acc = fmaf(s1[k * 64 + idx], mb_sum(part, S, k, MB_OFF_B1 + idx), acc);
    o.db1[idx] = acc;
    return;
  }
  idx -= 64;
  if (idx < 128) {                                       // dW0[j][i] (i < 3) and db0[j] (i == 3)
    const int j = idx >> 2, i = idx & 3;
    float acc = 0.f;
    for (int k = 0; k < 9; ++k) {
      if (k != META_CENTRE_TAP) { acc += mb_sum(part, S, k, MB_OFF_W0 + idx); continue; }
      if (i != 3 || !(w0[j * 4 + 3] > 0.f)) continue;    // centre tap: rel = 0, nothing for dW0; db0 through w_4 = s1 (W1 relu(b0) + b1)
      float t = 0.f;
      for (int c = 0; c < 64; ++c) t = fmaf(s1[k * 64 + c] * w1[c * 32 + j], mb_sum(part, S, k, MB_OFF_B1 + c), t);
      acc += t;
    }
    if (i == 3) o.db0[j] = acc;
    else o.dW0[j * 3 + i] = acc;
    return;
  }
  idx -= 128;
  if (idx < 2 * 576) {                                   // dt1[c 9 + k], dq1[c 9 + k]
    const int q = idx >= 576, ck = idx - 576 * q, c = ck / 9, k = ck - c * 9;
    (q ? o.dq1 : o.dt1)[ck] = mb_sum(part, S, k, (q ? MB_OFF_Q1 : MB_OFF_T1) + c);
  }
}
constexpr int MB_REDUCE_THREADS = 64 * 576 + 64 * 32 + 64 + 128 + 2 * 576;

// ---- launches: the callers (rd_meta_kernel_bwd_data / _params) have checked pointers, dtype, shape, strides and the workspace ----------------
inline int launch_meta_bwd_data(MetaBwdArgs a, int dt, hipStream_t st) {
  a.nfw = (a.W + 31) / 32;
  a.nfrag = mb_frags(a.B, a.H, a.W);
  a.nchunks = (a.nfrag + MB_DATA_WAVES - 1) / MB_DATA_WAVES;
  static std::atomic<unsigned long long> seen{0};
  once_per_device(seen, [] { allow_big_lds(meta_bwd_data_kernel<RD_BF16>); allow_big_lds(meta_bwd_data_kernel<RD_F16>); });
  const dim3 grid((unsigned)std::min<long>(a.nchunks, conv_num_cus())), block(MB_DATA_WAVES * 64);
  if (dt == RD_F16) hipLaunchKernelGGL(meta_bwd_data_kernel<RD_F16>, grid, block, MetaBwdDataLds::TOTAL, st, a);
  else hipLaunchKernelGGL(meta_bwd_data_kernel<RD_BF16>, grid, block, MetaBwdDataLds::TOTAL, st, a);
  return check_launch("meta_kernel_bwd_data");
}
inline int launch_meta_bwd_params(MetaBwdArgs a, const MetaBwdOut& out, int split, int dt, hipStream_t st) {
  a.nfw = (a.W + 31) / 32;
  a.nfrag = mb_frags(a.B, a.H, a.W);
  a.nchunks = mb_chunks(a.B, a.H, a.W);
  const int S = (int)mb_split(a.B, a.H, a.W, split);
  static std::atomic<unsigned long long> seen{0};
  once_per_device(seen, [] { allow_big_lds(meta_bwd_params_kernel<RD_BF16>); allow_big_lds(meta_bwd_params_kernel<RD_F16>); });
  const dim3 grid(S, 9), block(MB_WAVES * 64);
  if (dt == RD_F16) hipLaunchKernelGGL(meta_bwd_params_kernel<RD_F16>, grid, block, MetaBwdParamsLds::TOTAL, st, a);
  else hipLaunchKernelGGL(meta_bwd_params_kernel<RD_BF16>, grid, block, MetaBwdParamsLds::TOTAL, st, a);
  hipLaunchKernelGGL(meta_bwd_reduce_kernel, dim3((MB_REDUCE_THREADS + 255) / 256), dim3(256), 0, st, (const float*)a.part, S, a.packed, out);
  return check_launch("meta_kernel_bwd_params");
}

}  // namespace rd
