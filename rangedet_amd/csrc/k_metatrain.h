// The Meta-Kernel unit in TRAINING mode for gfx950, RD_BF16 / RD_F16: the 576-channel BatchNorm normalises with the batch's own statistics
// (the reference's normalizer_factory(type="localbn"), use_global_stats = False).  The batch-dependent scale does NOT live in the rounded
// weights: every kernel here reads the packed blocks made with s1 = 1, t1 = 0 (s2 = 1, t2 = 0) -- round16(W1), b1 with the centre tap's
// constant folded in double, round16(A), W0, b0 -- and takes the normalisation as float32 device tables of 576 values, index c 9 + k like
// s1 / t1 / dt1 / dq1.  A packed block therefore depends on the parameters only (rd_pack_meta_dev re-makes both after an SGD step), and the
// statistics and the forward see the same q.  n = B H W.
//
//   FORWARD    rel_k, u_k, h_k = relu(round16(u_k))          as k_metabwd.h (contract points 1 - 3; u_k by the fmaf chain of mb_hidden in
//                                                            EVERY kernel of this file, so that all of them see the same bits)
//              w_k = round16(W1) h_k + b1                    MFMA #1, float32 accumulation; k = 4: the packer's constant
//              q_k[c] = data[n_k][c] * w_k[c]                ONE float32 product; 0 where n_k is outside the image
//              mean1, var1                                   biased, over all n pixels of q_k[c] (border pixels count, with q = 0)
//              r_k = fmaf(q_k, a1, bb1)      a_k = relu(round16(r_k))          (a border tap gives relu(round16(bb1)), not 0)
//              z = round16(sum_{c,k} round16(A)[o, c 9 + k] a_k[c])            no affine, no ReLU: BN2 is rd_bn_stats / rd_bn_fold / rd_affine_relu
//   BACKWARD   da_k = round16(A)_k^T dz      gy_k = da_k [r_k > 0]             xh_k = (q_k - mean1) * rstd1      (two operations)
//              dbeta1 = sum_p gy_k           dgamma1: acc = fmaf(gy_k, xh_k, acc)          dA = sum_p dz (x) a_k
//              c1 = dbeta1 / (float)n        c2 = dgamma1 / (float)n
//              dq_k = a1 * fmaf(-xh_k, c2, gy_k - c1)        at EVERY pixel and tap, masked and border ones too (rd_bn_relu_bwd's formula)
//              e_k = dq_k * data[n_k]        ddata[p'] = round16(sum_k fmaf(w_k, dq_k, .)(p' - d_k) [+ residual])
//              dW1[c,j] = sum_{k,p} e_k[c] h_k[j]            db1[c] = sum_{k,p} e_k[c]
//              du_k = [u_k > 0] round16(W1)^T e_k            dW0 = sum du_k (x) rel_k      db0 = sum du_k
//              centre tap: meta_bwd_reduce_kernel's terms with s1 = 1, from P4[c] = sum_p e_4[p, c]
// dbeta1 and dgamma1 need the whole batch before any dq exists: the backward is two passes over the pixels.
//
// meta_stats_kernel        grid (S, 9) like the parameter kernels: a workgroup owns ONE tap and a contiguous run of chunks (4 fragments = 128
//                          pixel lanes); a lane carries 32 channels x (S1, S2).  Never E[q^2] - E[q]^2 about zero: the sums are shifted by a
//                          per-workgroup PILOT, as rd_bn_stats does (k_norm.h).  The pilot of a channel is the mean of 128 samples of q -- the
//                          lanes of the run's first chunk, a lane past the image taking the run's first pixel instead -- added as a halving tree
//                          over the lanes (64, 32, .. 1) and scaled by 1 / 128: 128 equal samples give that value in every bit.
//                            sweep   d = live ? q - p : 0;  S1 += d;  S2 = fmaf(d, d, S2)    per lane in chunk order, then the lanes in lane order
//                            partial (p[64], S1[64], S2[64], n_k = live pixels of the run) per (split slot, tap)
// meta_stats_merge_kernel  one thread per (c, k), the S partials in index order (rd_bn_stats' formulas, a sequential sum for its tree):
//                            q_s = S1_s / n_s;  m_s = p_s + q_s;  M2_s = fmaf(-S1_s, q_s, S2_s)
//                            mean = m_0 + (sum_s n_s (m_s - m_0)) / N;  e_s = m_s - mean;  var = max((sum_s fmaf(n_s e_s, e_s, M2_s)) / N, 0)
// meta_fwd_train_kernel    512 threads = 8 waves, a wave owns one fragment of 32 pixels, persistent over runs of 8 fragments; W1 and A fragments
//                          of the FORWARD block (108 KiB) and the [9][64] tables b1, a1, bb1 in LDS; W0 / b0 as float32 from the backward block.
// meta_train_sums_kernel   PASS A, grid (S, 9): the parameter kernel without the e / h transposes, the E product, du and dW0.  Partial:
//                          dA_k [64][64], sum gy [64], sum gy xh [64].  meta_train_sums_reduce_kernel adds the S partials in index order and
//                          writes dA, dbeta1, dgamma1, c1, c2.
// meta_train_params_kernel PASS B, grid (S, 9): the parameter kernel without the dz / a transposes and the dA product.  Partial: E_k [64][32],
//                          sum e [64], dW0 / db0 [32][4].  meta_train_params_reduce_kernel: partials, then taps, in index order.
// meta_train_data_kernel   meta_bwd_data_kernel's gather form with dq in place of dr; a source pixel outside the image adds nothing (its dq is
//                          not zero any more, so the tap is switched off explicitly).
// No atomics; every sum has a fixed order that depends on the shape and on `split` only: two calls give the same bytes.
//
// ARITHMETIC CONTRACT, training form -- every point where a value is rounded to the 16-bit type (everything else is float32):
//   (1) h_k = relu(round(u_k))                (2) round(W1) and (3) round(A): the packer's values with s1 = 1
//   (4t) a_k = relu(round(r_k)) as the B operand of z (forward) and of dA (pass A); the masks [r_k > 0] test the float32 r_k
//   (5t) e_k = round(dq_k * data[n_k]) as the operand of the dW1 product and of du_k (pass B); db1 and P4 sum the float32 e_k
//   (6) ddata = round(sum + residual), once   (7t) z = round(float32 sum), once
// q_k, r_k, xh_k, dq_k, the statistics, c1 and c2 are float32; contraction is off in every function of this file: what is not spelled fmaf
// is a separately rounded operation.
#pragma once
#include "k_metabwd.h"

namespace rd {

struct MetaTrainArgs : MetaBwdArgs {
  const unsigned char* packed_fwd;                       // forward launch: the block of meta_layout (W1, A fragments, b1)
  const float *a1, *bb1, *mean1, *rstd1, *c1, *c2;       // [c 9 + k]
};

constexpr int MT_ST_PART = 256;                          // stats partial: pilot [64], S1 [64], S2 [64], n_k
constexpr int MTA_OFF_BETA = 4096, MTA_OFF_GAMMA = 4160, MTA_PART = 4224;          // pass A partial: dA_k [64 o][64 c], sum gy, sum gy xh
constexpr int MTB_OFF_B1 = 2048, MTB_OFF_W0 = 2112, MTB_PART = 2240;               // pass B partial: E_k [64 c][32 j], sum e, [32 j][4]
inline size_t mt_stats_ws_bytes(int B, int H, int W, int split) { return (size_t)mb_split(B, H, W, split) * 9 * MT_ST_PART * sizeof(float); }
inline size_t mt_bwd_ws_bytes(int B, int H, int W, int split) { return (size_t)mb_split(B, H, W, split) * 9 * MTA_PART * sizeof(float); }
static_assert(MTB_PART <= MTA_PART, "one workspace serves both passes");

constexpr size_t MT_RED_B = (size_t)MB_PT * 64 * sizeof(float);   // the lane-sum buffer [128][64]
struct MetaTrainFwdLds {
  static constexpr size_t W_B = Meta16Lds::W_B;                                              // 108 KiB
  static constexpr size_t WEIGHTS = 0, B1 = W_B, A1 = B1 + 2304, BB1 = A1 + 2304, W0 = BB1 + 2304, TOTAL = W0 + 512;
};
struct MetaTrainDataLds {
  static constexpr size_t W_B = meta_bwd_layout().wbytes;                                    // 108 KiB
  static constexpr size_t WEIGHTS = 0, B1 = W_B, W0 = B1 + 2304, TABS = W0 + 512, TOTAL = TABS + 6 * 2304;
};
static_assert(MetaTrainFwdLds::TOTAL <= 160 * 1024 && MetaTrainDataLds::TOTAL <= 160 * 1024, "LDS budget of the training Meta-Kernel");

// one [64] row of tap k out of an ABI vector [c 9 + k]
__device__ __forceinline__ void mt_tab_row(float* dst, const float* tab, int k, int tid) {
  if (tid < 64) dst[tid] = tab[tid * 9 + k];
}
// all nine rows [k][64]
__device__ __forceinline__ void mt_tab_all(float* dst, const float* tab, int tid, int nt) {
  for (int i = tid; i < 576; i += nt) dst[i] = tab[(i & 63) * 9 + (i >> 6)];
}
// the 16 channels 32 mt + 16 hi .. of pixel `pix`, zeros when `on` is false
template <int DT>
__device__ __forceinline__ void mt_load_x(const MetaBwdArgs& a, bool on, size_t pix, int mt, int hi, float (&x)[16]) {
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    Slot16 v = {0u, 0u, 0u, 0u};
    if (on) v = *(const Slot16*)(a.data + pix * a.d_cs + a.d_co + 32 * mt + 16 * hi + 8 * sl);
    float t[8];
    slot_unpack<DT>(v, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[8 * sl + e] = t[e];
  }
}
// w_k of the lane's 16 channels of block mt: b1 (the centre tap: the folded constant) + round16(W1) h
template <int DT>
__device__ __forceinline__ f32x16 mt_w(const float* b1k, const unsigned char* w1lk, int mt, int hi, bool centre, const s16x8 (&hf)[2]) {
  f32x16 w = mb_load16(b1k + 32 * mt + 16 * hi);
  if (!centre) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) w = H16<DT>::mfma(*(const s16x8*)(w1lk + (mt * 2 + ks) * 1024), hf[ks], w);
  }
  return w;
}
// rel of the tap (zero padding outside the image) and the hidden layer of a lane that owns pixel p with neighbour (nh, nw)
template <int DT>
__device__ __forceinline__ void mt_hidden_fwd(const MetaBwdArgs& a, const MbPixel& p, bool nin, int nh, int nw, const float* cw0, int hi,
                                              float (&rel)[3], float (&u)[16], s16x8 (&hf)[2]) {
  _Pragma("clang fp contract(off)")
  const size_t HW = (size_t)a.H * a.W;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
  if (p.live) { const float* cp = mb_coord(a, p.b, p.h, p.w); c0 = cp[0]; c1 = cp[HW]; c2 = cp[2 * HW]; }
  if (nin) { const float* cn = mb_coord(a, p.b, nh, nw); n0 = cn[0]; n1 = cn[HW]; n2 = cn[2 * HW]; }
  rel[0] = n0 - c0; rel[1] = n1 - c1; rel[2] = n2 - c2;
  mb_hidden<DT>(cw0, hi, rel[0], rel[1], rel[2], u, hf);
}
// dq = a1 * fmaf(-xh, c2, gy - c1)
__device__ __forceinline__ float mt_dq(float q, float r, float da, float a1, float mean, float rstd, float c1, float c2) {
  _Pragma("clang fp contract(off)")
  const float gy = r > 0.f ? da : 0.f;
  const float xh = (q - mean) * rstd;
  return a1 * fmaf(-xh, c2, gy - c1);
}
__device__ __forceinline__ float mt_mul(float x, float w) {
  _Pragma("clang fp contract(off)")
  return x * w;
}

// ---- statistics of q ---------------------------------------------------------------------------------------------------------------------
struct MetaStatsLds {
  static constexpr size_t RED = 0, FRAG = MT_RED_B, CONSTS = FRAG + 4096, TOTAL = CONSTS + (64 + 128 + 64) * 4;   // b1_k, W0, pilot
};
template <int DT>
__global__ __launch_bounds__(MB_WAVES * 64) void meta_stats_kernel(MetaTrainArgs a) {
  _Pragma("clang fp contract(off)")
  using L = MetaStatsLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  float* red = (float*)(smem + L::RED);                  // [MB_PT][64]
  unsigned char* lf = smem + L::FRAG;
  float* lc = (float*)(smem + L::CONSTS);
  const float* cb1 = lc;
  const float* cw0 = lc + 64;
  float* pil = lc + 192;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5, pl = wave * 32 + px;
  const int S = gridDim.x, s = blockIdx.x, k = blockIdx.y;
  const bool centre = k == META_CENTRE_TAP;
  const int dh = k / 3 - 1, dw = k % 3 - 1;
  for (int i = tid; i < 256; i += NT) ((Slot16*)lf)[i] = ((const Slot16*)(a.packed + P.w1s + (size_t)k * 4096))[i];
  if (tid < 64) lc[tid] = ((const float*)(a.packed + P.b1s))[k * 64 + tid];
  if (tid < 128) lc[64 + tid] = ((const float*)(a.packed + P.w0))[tid];
  __syncthreads();
  const unsigned char* w1l = lf + lane * 16;
  const long c_lo = s * a.nchunks / S, c_hi = (s + 1) * a.nchunks / S;

  // q of the lane's 32 channels at pixel p (p.live), tap k
  auto qcalc = [&](const MbPixel& p, float (&q)[2][16]) {
    const int nh = p.h + dh, nw = p.w + dw;
    const bool nin = p.live && (unsigned)nh < (unsigned)a.H && (unsigned)nw < (unsigned)a.W;
    const size_t npix = ((size_t)p.b * a.H + nh) * a.W + nw;
    float rel[3], u[16];
    s16x8 hf[2] = {};
    if (!centre) mt_hidden_fwd<DT>(a, p, nin, nh, nw, cw0, hi, rel, u, hf);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      float x[16];
      mt_load_x<DT>(a, nin, npix, mt, hi, x);
      const f32x16 w = mt_w<DT>(cb1, w1l, mt, hi, centre, hf);
#pragma unroll
      for (int r = 0; r < 16; ++r) q[mt][r] = mt_mul(x[r], w[r]);
    }
  };
  auto put = [&](const float (&v)[2][16]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[pl * 64 + 32 * mt + 16 * hi + r] = v[mt][r];
  };

  float q[2][16], pv[2][16], s1[2][16], s2[2][16];
  {   // pilot: 128 samples, a halving tree over the pixel lanes
    MbPixel p = mb_pixel(a, c_lo * MB_WAVES + wave, px);
    if (!p.live) p = mb_pixel(a, c_lo * MB_WAVES, 0);    // (the first pixel of a run is always inside the image)
    qcalc(p, q);
    put(q);
    __syncthreads();
    for (int st = MB_PT / 2; st >= 1; st >>= 1) {
      for (int i = tid; i < st * 64; i += NT) red[i] += red[st * 64 + i];
      __syncthreads();
    }
    if (tid < 64) pil[tid] = red[tid] * (1.0f / MB_PT);
    __syncthreads();
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pv[mt][r] = pil[32 * mt + 16 * hi + r];
      s1[mt][r] = s2[mt][r] = 0.f;
    }
  for (long ch = c_lo; ch < c_hi; ++ch) {
    const MbPixel p = mb_pixel(a, ch * MB_WAVES + wave, px);
    qcalc(p, q);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = p.live ? q[mt][r] - pv[mt][r] : 0.f;
        s1[mt][r] += d;
        s2[mt][r] = fmaf(d, d, s2[mt][r]);
      }
  }
  float* part = a.part + ((size_t)s * 9 + k) * MT_ST_PART;
  put(s1);
  __syncthreads();
  if (tid < 64) part[64 + tid] = lane_sum(red, MB_PT, 64, tid);
  __syncthreads();
  put(s2);
  __syncthreads();
  if (tid < 64) {
    part[128 + tid] = lane_sum(red, MB_PT, 64, tid);
    part[tid] = pil[tid];
  }
  if (tid == 0) {   // live pixels of the run: 32 per fragment, the last fragment of an image row has W - 32 (nfw - 1)
    const long f_lo = c_lo * MB_WAVES, f_hi = c_hi * MB_WAVES < a.nfrag ? c_hi * MB_WAVES : a.nfrag;
    const long nlast = f_hi / a.nfw - f_lo / a.nfw;
    part[192] = (float)(32 * (f_hi - f_lo) - (32L * a.nfw - a.W) * nlast);
  }
}
__global__ __launch_bounds__(64) void meta_stats_merge_kernel(const float* __restrict__ part, int S, float N, float* __restrict__ mean,
                                                              float* __restrict__ var) {
  _Pragma("clang fp contract(off)")
  const int c = threadIdx.x, k = blockIdx.x;
  auto at = [&](int s, int off) { return part[((size_t)s * 9 + k) * MT_ST_PART + off]; };
  const float m0 = at(0, c) + at(0, 64 + c) / at(0, 192);
  float acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const float nf = at(s, 192), mk = at(s, c) + at(s, 64 + c) / nf;
    acc += nf * (mk - m0);
  }
  const float mu = m0 + acc / N;
  acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const float nf = at(s, 192), S1 = at(s, 64 + c), q = S1 / nf, mk = at(s, c) + q, e = mk - mu;
    acc += fmaf(nf * e, e, fmaf(-S1, q, at(s, 128 + c)));
  }
  mean[c * 9 + k] = mu;
  var[c * 9 + k] = fmaxf(acc / N, 0.f);
}

// ---- training forward ------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MB_DATA_WAVES * 64) void meta_fwd_train_kernel(MetaTrainArgs a) {
  _Pragma("clang fp contract(off)")
  using HT = H16<DT>;
  using L = MetaTrainFwdLds;
  constexpr MetaLayout PF = meta_layout(DT);
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_DATA_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned char* lw = smem + L::WEIGHTS;
  float* cb1 = (float*)(smem + L::B1);                   // [9][64]
  float* ca1 = (float*)(smem + L::A1);
  float* cbb = (float*)(smem + L::BB1);
  float* cw0 = (float*)(smem + L::W0);                   // [32][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5;
  for (size_t i = tid; i < L::W_B / 16; i += NT) ((Slot16*)lw)[i] = ((const Slot16*)a.packed_fwd)[i];
  for (int i = tid; i < 576; i += NT) cb1[i] = ((const float*)(a.packed_fwd + PF.b1p))[i];
  if (tid < 128) cw0[tid] = ((const float*)(a.packed + P.w0))[tid];
  mt_tab_all(ca1, a.a1, tid, NT);
  mt_tab_all(cbb, a.bb1, tid, NT);
  __syncthreads();
  const unsigned char* w1l = lw + PF.w1s + lane * 16;
  const unsigned char* a2l = lw + PF.a2 + lane * 16;

  for (long run = blockIdx.x; run < a.nchunks; run += gridDim.x) {
    const long f = run * MB_DATA_WAVES + wave;
    if (f >= a.nfrag) continue;                          // (uniform over the wave; there is no barrier in this loop)
    const MbPixel p = mb_pixel(a, f, px);
    f32x16 acc2[2];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[ot][r] = 0.f;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      const bool centre = k == META_CENTRE_TAP;
      const int nh = p.h + (k / 3 - 1), nw = p.w + (k % 3 - 1);
      const bool nin = p.live && (unsigned)nh < (unsigned)a.H && (unsigned)nw < (unsigned)a.W;
      const size_t npix = ((size_t)p.b * a.H + nh) * a.W + nw;
      float rel[3], u[16];
      s16x8 hf[2] = {};
      if (!centre) mt_hidden_fwd<DT>(a, p, nin, nh, nw, cw0, hi, rel, u, hf);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        float x[16];
        mt_load_x<DT>(a, nin, npix, mt, hi, x);
        const f32x16 w = mt_w<DT>(cb1 + k * 64, w1l + k * 4096, mt, hi, centre, hf);
        const f32x16 va = mb_load16(ca1 + k * 64 + 32 * mt + 16 * hi), vb = mb_load16(cbb + k * 64 + 32 * mt + 16 * hi);
        s16x8 bfr[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float rr = fmaf(mt_mul(x[r], w[r]), va[r], vb[r]);
          const unsigned short a16 = HT::from_f32(rr);
          bfr[r >> 3][r & 7] = (short)a16 < 0 ? (short)0 : (short)a16;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int ot = 0; ot < 2; ++ot)
            acc2[ot] = HT::mfma(*(const s16x8*)(a2l + (((k * 2 + ot) * 2 + mt) * 2 + s2) * 1024), bfr[s2], acc2[ot]);
      }
    }
    if (p.live) {
      const size_t pix = ((size_t)p.b * a.H + p.h) * a.W + p.w;
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = acc2[ot][8 * sl + e];
          *(Slot16*)(a.ddata + pix * a.g_cs + a.g_co + 32 * ot + 16 * hi + 8 * sl) = slot_pack<DT>(o);
        }
    }
  }
}

// ---- pass A: dA, dbeta1, dgamma1 ---------------------------------------------------------------------------------------------------------
struct MetaTrainSumsLds {
  static constexpr size_t T_B = (size_t)128 * MB_RS * 2;                                    // Tz, Ta [64][MB_RS]; then the lane-sum buffer
  static constexpr size_t T = 0, FRAGS = T_B, CONSTS = FRAGS + 4096 + 8192, TOTAL = CONSTS + (64 * 5 + 128) * 4;
};
static_assert(MT_RED_B <= MetaTrainSumsLds::T_B, "the lane-sum buffer reuses the transpose rows");
template <int DT>
__global__ __launch_bounds__(MB_WAVES * 64) void meta_train_sums_kernel(MetaTrainArgs a) {
  _Pragma("clang fp contract(off)")
  using HT = H16<DT>;
  using L = MetaTrainSumsLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned short (*Tz)[MB_RS] = (unsigned short (*)[MB_RS])(smem + L::T);   // [64 o][pixel]
  unsigned short (*Ta)[MB_RS] = Tz + 64;                                    // [64 c][pixel]
  float* red = (float*)(smem + L::T);
  unsigned char* lf = smem + L::FRAGS;
  float* lc = (float*)(smem + L::CONSTS);
  const float *cb1 = lc, *ca1 = lc + 64, *cbb = lc + 128, *cmu = lc + 192, *crs = lc + 256, *cw0 = lc + 320;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5, pl = wave * 32 + px;
  const int S = gridDim.x, s = blockIdx.x, k = blockIdx.y;
  const bool centre = k == META_CENTRE_TAP;
  const int dh = k / 3 - 1, dw = k % 3 - 1;
  for (int i = tid; i < 256; i += NT) ((Slot16*)lf)[i] = ((const Slot16*)(a.packed + P.w1s + (size_t)k * 4096))[i];
  for (int i = tid; i < 512; i += NT) ((Slot16*)(lf + 4096))[i] = ((const Slot16*)(a.packed + P.at + (size_t)k * 8192))[i];
  if (tid < 64) lc[tid] = ((const float*)(a.packed + P.b1s))[k * 64 + tid];
  mt_tab_row(lc + 64, a.a1, k, tid);
  mt_tab_row(lc + 128, a.bb1, k, tid);
  mt_tab_row(lc + 192, a.mean1, k, tid);
  mt_tab_row(lc + 256, a.rstd1, k, tid);
  if (tid < 128) lc[320 + tid] = ((const float*)(a.packed + P.w0))[tid];
  __syncthreads();
  const unsigned char* w1l = lf + lane * 16;
  const unsigned char* atl = lf + 4096 + lane * 16;

  float sb[2][16], sg[2][16];
  f32x16 accA;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accA[r] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) sb[mt][r] = sg[mt][r] = 0.f;
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
      Slot16 v = {0u, 0u, 0u, 0u};        // a lane past the image carries dz = 0: gy = 0, nothing for any sum
      if (p.live) v = *(const Slot16*)(a.dz + pix * a.z_cs + a.z_co + 16 * ko + 8 * hi);
      zf[ko] = __builtin_bit_cast(s16x8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) Tz[16 * ko + 8 * hi + e][pl] = (unsigned short)zf[ko][e];
    }
    float rel[3], u[16];
    s16x8 hf[2] = {};
    if (!centre) mt_hidden_fwd<DT>(a, p, nin, nh, nw, cw0, hi, rel, u, hf);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      float x[16];
      mt_load_x<DT>(a, nin, npix, mt, hi, x);
      const f32x16 w = mt_w<DT>(cb1, w1l, mt, hi, centre, hf);
      f32x16 da;
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
      for (int ko = 0; ko < 4; ++ko) da = HT::mfma(*(const s16x8*)(atl + (mt * 4 + ko) * 1024), zf[ko], da);
      const int cb = 32 * mt + 16 * hi;
      const f32x16 va = mb_load16(ca1 + cb), vb = mb_load16(cbb + cb), vm = mb_load16(cmu + cb), vr = mb_load16(crs + cb);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float q = mt_mul(x[r], w[r]), rr = fmaf(q, va[r], vb[r]);
        const float gy = rr > 0.f ? da[r] : 0.f, xh = (q - vm[r]) * vr[r];
        sb[mt][r] += gy;
        sg[mt][r] = fmaf(gy, xh, sg[mt][r]);
        const unsigned short a16 = HT::from_f32(rr);
        Ta[cb + r][pl] = (short)a16 < 0 ? (unsigned short)0 : a16;
      }
    }
    __syncthreads();
    {   // the pixel axis as K: dA_k[o][c] += sum_p dz[p][o] a[p][c], wave = one 32 x 32 tile
      const int m = lane & 31, k8 = 8 * hi, ot = wave >> 1, ct = wave & 1;
#pragma unroll
      for (int ks = 0; ks < MB_PT / 16; ++ks)
        accA = HT::mfma(*(const s16x8*)&Tz[32 * ot + m][16 * ks + k8], *(const s16x8*)&Ta[32 * ct + m][16 * ks + k8], accA);
    }
    __syncthreads();
  }
  float* part = a.part + ((size_t)s * 9 + k) * MTA_PART;
  {
    const int n = lane & 31, ot = wave >> 1, ct = wave & 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(32 * ot + mb_j(r, hi)) * 64 + 32 * ct + n] = accA[r];
  }
  auto lane_reduce = [&](const float (&v)[2][16], int off) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[pl * 64 + 32 * mt + 16 * hi + r] = v[mt][r];
    __syncthreads();
    if (tid < 64) part[off + tid] = lane_sum(red, MB_PT, 64, tid);
    __syncthreads();
  };
  lane_reduce(sb, MTA_OFF_BETA);
  lane_reduce(sg, MTA_OFF_GAMMA);
}
__device__ __forceinline__ float mt_sum(const float* part, int stride, int S, int k, int off) {
  _Pragma("clang fp contract(off)")
  float sum = part[(size_t)k * stride + off];
  for (int s = 1; s < S; ++s) sum += part[((size_t)s * 9 + k) * stride + off];
  return sum;
}
struct MetaTrainSumsOut { float *dA, *dbeta1, *dgamma1, *c1, *c2; };
constexpr int MTA_REDUCE_THREADS = 64 * 576 + 576;
__global__ __launch_bounds__(256) void meta_train_sums_reduce_kernel(const float* __restrict__ part, int S, float N, MetaTrainSumsOut o) {
  _Pragma("clang fp contract(off)")
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 64 * 576) {
    const int oc = idx / 576, ck = idx - oc * 576, c = ck / 9, k = ck - c * 9;
    o.dA[idx] = mt_sum(part, MTA_PART, S, k, oc * 64 + c);
    return;
  }
  idx -= 64 * 576;
  if (idx < 576) {
    const int c = idx / 9, k = idx - c * 9;
    const float db = mt_sum(part, MTA_PART, S, k, MTA_OFF_BETA + c), dg = mt_sum(part, MTA_PART, S, k, MTA_OFF_GAMMA + c);
    o.dbeta1[idx] = db;
    o.dgamma1[idx] = dg;
    o.c1[idx] = db / N;
    o.c2[idx] = dg / N;
  }
}

// ---- pass B: dW1, db1, dW0, db0 ----------------------------------------------------------------------------------------------------------
struct MetaTrainParamsLds {
  static constexpr size_t T_B = MT_RED_B;                                                   // Te [64][MB_RS], Th [32][MB_RS]; the lane-sum buffer
  static constexpr size_t T = 0, FRAGS = T_B, CONSTS = FRAGS + 4096 + 8192 + 4096, TOTAL = CONSTS + (64 * 7 + 128) * 4;
};
static_assert((size_t)96 * MB_RS * 2 <= MetaTrainParamsLds::T_B, "the transpose rows fit the lane-sum buffer");
template <int DT>
__global__ __launch_bounds__(MB_WAVES * 64) void meta_train_params_kernel(MetaTrainArgs a) {
  _Pragma("clang fp contract(off)")
  using HT = H16<DT>;
  using L = MetaTrainParamsLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned short (*Te)[MB_RS] = (unsigned short (*)[MB_RS])(smem + L::T);   // [64 c][pixel]
  unsigned short (*Th)[MB_RS] = Te + 64;                                    // [32 j][pixel]
  float* red = (float*)(smem + L::T);
  unsigned char* lf = smem + L::FRAGS;
  float* lc = (float*)(smem + L::CONSTS);
  const float *cb1 = lc, *ca1 = lc + 64, *cbb = lc + 128, *cmu = lc + 192, *crs = lc + 256, *cc1 = lc + 320, *cc2 = lc + 384, *cw0 = lc + 448;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5, pl = wave * 32 + px;
  const int S = gridDim.x, s = blockIdx.x, k = blockIdx.y;
  const bool centre = k == META_CENTRE_TAP;
  const int dh = k / 3 - 1, dw = k % 3 - 1;
  for (int i = tid; i < 256; i += NT) ((Slot16*)lf)[i] = ((const Slot16*)(a.packed + P.w1s + (size_t)k * 4096))[i];
  for (int i = tid; i < 512; i += NT) ((Slot16*)(lf + 4096))[i] = ((const Slot16*)(a.packed + P.at + (size_t)k * 8192))[i];
  for (int i = tid; i < 256; i += NT) ((Slot16*)(lf + 12288))[i] = ((const Slot16*)(a.packed + P.w1t + (size_t)k * 4096))[i];
  if (tid < 64) lc[tid] = ((const float*)(a.packed + P.b1s))[k * 64 + tid];
  mt_tab_row(lc + 64, a.a1, k, tid);
  mt_tab_row(lc + 128, a.bb1, k, tid);
  mt_tab_row(lc + 192, a.mean1, k, tid);
  mt_tab_row(lc + 256, a.rstd1, k, tid);
  mt_tab_row(lc + 320, a.c1, k, tid);
  mt_tab_row(lc + 384, a.c2, k, tid);
  if (tid < 128) lc[448 + tid] = ((const float*)(a.packed + P.w0))[tid];
  __syncthreads();
  const unsigned char* w1l = lf + lane * 16;
  const unsigned char* atl = lf + 4096 + lane * 16;
  const unsigned char* wtl = lf + 12288 + lane * 16;

  float se[2][16], sw0[16][4];
  f32x16 accE;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accE[r] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) se[mt][r] = 0.f;
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
      Slot16 v = {0u, 0u, 0u, 0u};
      if (p.live) v = *(const Slot16*)(a.dz + pix * a.z_cs + a.z_co + 16 * ko + 8 * hi);
      zf[ko] = __builtin_bit_cast(s16x8, v);
    }
    float rel[3] = {0.f, 0.f, 0.f}, u[16];
    s16x8 hf[2] = {};
    if (!centre) {
      mt_hidden_fwd<DT>(a, p, nin, nh, nw, cw0, hi, rel, u, hf);
#pragma unroll
      for (int r = 0; r < 16; ++r) Th[mb_j(r, hi)][pl] = (unsigned short)hf[r >> 3][r & 7];
    }
    s16x8 ef[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      float x[16];
      mt_load_x<DT>(a, nin, npix, mt, hi, x);      // a lane past the image and a padded tap read data = 0: e = 0
      const f32x16 w = mt_w<DT>(cb1, w1l, mt, hi, centre, hf);
      f32x16 da;
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
      for (int ko = 0; ko < 4; ++ko) da = HT::mfma(*(const s16x8*)(atl + (mt * 4 + ko) * 1024), zf[ko], da);
      const int cb = 32 * mt + 16 * hi;
      const f32x16 va = mb_load16(ca1 + cb), vb = mb_load16(cbb + cb), vm = mb_load16(cmu + cb), vr = mb_load16(crs + cb);
      const f32x16 v1 = mb_load16(cc1 + cb), v2 = mb_load16(cc2 + cb);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float q = mt_mul(x[r], w[r]), rr = fmaf(q, va[r], vb[r]);
        const float ev = mt_mul(mt_dq(q, rr, da[r], va[r], vm[r], vr[r], v1[r], v2[r]), x[r]);
        se[mt][r] += ev;
        const unsigned short e16 = HT::from_f32(ev);
        Te[cb + r][pl] = e16;
        ef[2 * mt + (r >> 3)][r & 7] = (short)e16;
      }
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
        sw0[r][0] = fmaf(d, rel[0], sw0[r][0]);
        sw0[r][1] = fmaf(d, rel[1], sw0[r][1]);
        sw0[r][2] = fmaf(d, rel[2], sw0[r][2]);
        sw0[r][3] += d;
      }
    }
    __syncthreads();
    if (!centre && wave < 2) {   // E_k[c][j] += sum_p e[p][c] h[p][j]
      const int m = lane & 31, k8 = 8 * hi;
#pragma unroll
      for (int ks = 0; ks < MB_PT / 16; ++ks)
        accE = HT::mfma(*(const s16x8*)&Te[32 * wave + m][16 * ks + k8], *(const s16x8*)&Th[m][16 * ks + k8], accE);
    }
    __syncthreads();
  }
  float* part = a.part + ((size_t)s * 9 + k) * MTB_PART;
  if (!centre && wave < 2) {
    const int n = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(32 * wave + mb_j(r, hi)) * 32 + n] = accE[r];
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[pl * 64 + 32 * mt + 16 * hi + r] = se[mt][r];
  __syncthreads();
  if (tid < 64) part[MTB_OFF_B1 + tid] = lane_sum(red, MB_PT, 64, tid);
  __syncthreads();
  if (!centre) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[pl * 64 + (mb_j(8 * half + r, hi) & 15) * 4 + i] = sw0[8 * half + r][i];
      __syncthreads();
      if (tid < 64) part[MTB_OFF_W0 + 64 * half + tid] = lane_sum(red, MB_PT, 64, tid);
      __syncthreads();
    }
  }
}
struct MetaTrainParamsOut { float *dW1, *db1, *dW0, *db0; };
constexpr int MTB_REDUCE_THREADS = 64 * 32 + 64 + 128;
__global__ __launch_bounds__(256) void meta_train_params_reduce_kernel(const float* __restrict__ part, int S, const unsigned char* __restrict__ packed,
                                                                       MetaTrainParamsOut o) {
  _Pragma("clang fp contract(off)")
  constexpr MetaBwdLayout P = meta_bwd_layout();
  const float* w0 = (const float*)(packed + P.w0);       // [j][4]
  const float* w1 = (const float*)(packed + P.w1raw);    // [c][j]
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 64 * 32) {                                   // dW1[c][j]
    const int c = idx >> 5, j = idx & 31;
    float acc = 0.f;
    for (int k = 0; k < 9; ++k)
      acc += k == META_CENTRE_TAP ? fmaxf(w0[j * 4 + 3], 0.f) * mt_sum(part, MTB_PART, S, k, MTB_OFF_B1 + c) : mt_sum(part, MTB_PART, S, k, c * 32 + j);
    o.dW1[idx] = acc;
    return;
  }
  idx -= 64 * 32;
  if (idx < 64) {                                        // db1[c]
    float acc = 0.f;
    for (int k = 0; k < 9; ++k) acc += mt_sum(part, MTB_PART, S, k, MTB_OFF_B1 + idx);
    o.db1[idx] = acc;
    return;
  }
  idx -= 64;
  if (idx < 128) {                                       // dW0[j][i] (i < 3) and db0[j] (i == 3)
    const int j = idx >> 2, i = idx & 3;
    float acc = 0.f;
    for (int k = 0; k < 9; ++k) {
      if (k != META_CENTRE_TAP) { acc += mt_sum(part, MTB_PART, S, k, MTB_OFF_W0 + idx); continue; }
      if (i != 3 || !(w0[j * 4 + 3] > 0.f)) continue;    // centre tap: rel = 0, nothing for dW0; db0 through w_4 = W1 relu(b0) + b1
      float t = 0.f;
      for (int c = 0; c < 64; ++c) t = fmaf(w1[c * 32 + j], mt_sum(part, MTB_PART, S, k, MTB_OFF_B1 + c), t);
      acc += t;
    }
    if (i == 3) o.db0[j] = acc;
    else o.dW0[j * 3 + i] = acc;
  }
}

// ---- data gradient, training form ----------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(MB_DATA_WAVES * 64) void meta_train_data_kernel(MetaTrainArgs a) {
  _Pragma("clang fp contract(off)")
  using HT = H16<DT>;
  using L = MetaTrainDataLds;
  constexpr MetaBwdLayout P = meta_bwd_layout();
  constexpr int NT = MB_DATA_WAVES * 64;
  HIP_DYNAMIC_SHARED(unsigned char, smem);
  unsigned char* lw = smem + L::WEIGHTS;
  float* cb1 = (float*)(smem + L::B1);                   // [9][64]
  float* cw0 = (float*)(smem + L::W0);                   // [32][4]
  float* tabs = (float*)(smem + L::TABS);                // a1, bb1, mean1, rstd1, c1, c2: [9][64] each
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 31, hi = lane >> 5;
  for (size_t i = tid; i < L::W_B / 16; i += NT) ((Slot16*)lw)[i] = ((const Slot16*)a.packed)[i];
  for (int i = tid; i < 576; i += NT) cb1[i] = ((const float*)(a.packed + P.b1s))[i];
  if (tid < 128) cw0[tid] = ((const float*)(a.packed + P.w0))[tid];
  mt_tab_all(tabs, a.a1, tid, NT);
  mt_tab_all(tabs + 576, a.bb1, tid, NT);
  mt_tab_all(tabs + 2 * 576, a.mean1, tid, NT);
  mt_tab_all(tabs + 3 * 576, a.rstd1, tid, NT);
  mt_tab_all(tabs + 4 * 576, a.c1, tid, NT);
  mt_tab_all(tabs + 5 * 576, a.c2, tid, NT);
  __syncthreads();
  const unsigned char* w1l = lw + P.w1s + lane * 16;
  const unsigned char* atl = lw + P.at + lane * 16;
  const size_t HW = (size_t)a.H * a.W;

  for (long run = blockIdx.x; run < a.nchunks; run += gridDim.x) {
    const long f = run * MB_DATA_WAVES + wave;
    if (f >= a.nfrag) continue;
    const MbPixel p = mb_pixel(a, f, px);
    const size_t pix = ((size_t)p.b * a.H + p.h) * a.W + p.w;
    float x[2][16];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) mt_load_x<DT>(a, p.live, pix, mt, hi, x[mt]);
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
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
      const int qh = p.h - (k / 3 - 1), qw = p.w - (k % 3 - 1);    // the pixel whose tap k reads p'
      const bool inq = p.live && (unsigned)qh < (unsigned)a.H && (unsigned)qw < (unsigned)a.W;
      const size_t qpix = ((size_t)p.b * a.H + qh) * a.W + qw;
      s16x8 zf[4];
#pragma unroll
      for (int ko = 0; ko < 4; ++ko) {
        Slot16 v = {0u, 0u, 0u, 0u};
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
        const f32x16 w = mt_w<DT>(cb1 + k * 64, w1l + k * 4096, mt, hi, k == META_CENTRE_TAP, hf);
        f32x16 da;
#pragma unroll
        for (int r = 0; r < 16; ++r) da[r] = 0.f;
#pragma unroll
        for (int ko = 0; ko < 4; ++ko) da = HT::mfma(*(const s16x8*)(atl + ((k * 2 + mt) * 4 + ko) * 1024), zf[ko], da);
        const float* t = tabs + k * 64 + 32 * mt + 16 * hi;
        // (the six table rows are read four channels at a time, next to their use.  The kernel still spills 14 dwords per lane at its 256
        //  registers -- as it did with all 16 channels of the six rows loaded up front: DESIGN.md section 5)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const f32x4 va = *(const f32x4*)(t + 4 * g4), vb = *(const f32x4*)(t + 576 + 4 * g4), vm = *(const f32x4*)(t + 2 * 576 + 4 * g4);
          const f32x4 vr = *(const f32x4*)(t + 3 * 576 + 4 * g4), v1 = *(const f32x4*)(t + 4 * 576 + 4 * g4), v2 = *(const f32x4*)(t + 5 * 576 + 4 * g4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g4 + e;
            const float q = mt_mul(x[mt][r], w[r]), rr = fmaf(q, va[e], vb[e]);
            const float dq = mt_dq(q, rr, da[r], va[e], vm[e], vr[e], v1[e], v2[e]);
            acc[mt][r] = fmaf(inq ? w[r] : 0.f, dq, acc[mt][r]);   // a source pixel outside the image does not exist
          }
        }
      }
    }
    if (p.live) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          const int c = 32 * mt + 16 * hi + 8 * sl;
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = acc[mt][8 * sl + e];
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

// ---- re-pack on the device: both blocks from the float32 masters, s1 = s2 = 1, t1 = t2 = 0 ---------------------------------------------------
// Byte for byte what pack_meta / pack_meta_bwd write for those tables.  The centre tap's fold is the host loop: a multiply, then an add, in
// double (contraction off).  Threads: [0, 4608) one (tap, lane, element) of the MFMA fragments; then 576 (k, c): b1, t1, s1; 64 lanes of the
// hidden layer's A operand; 128: W0 / b0 of the backward block, zeros of the forward block's W0 slot, s2 and t2; 2048: W1 itself.
struct MetaPackDevArgs { const float *w0, *b0, *w1, *b1, *agg; unsigned char *fwd, *bwd; };
constexpr int MT_PACK_THREADS = 4608 + 576 + 64 + 128 + 2048;
__device__ __forceinline__ int mt_perm(int blk, int m) { return 32 * blk + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3); }   // meta_perm
template <int DT>
__global__ __launch_bounds__(256) void meta_pack_dev_kernel(MetaPackDevArgs a) {
  _Pragma("clang fp contract(off)")
  using HT = H16<DT>;
  constexpr MetaLayout F = meta_layout(DT);
  constexpr MetaBwdLayout Bk = meta_bwd_layout();
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < 4608) {
    const int k = idx / 512, lane = (idx >> 3) & 63, e = idx & 7, m = lane & 31, hi = lane >> 5;
    unsigned short* fw1 = (unsigned short*)(a.fwd + F.w1s);
    unsigned short* fa2 = (unsigned short*)(a.fwd + F.a2);
    unsigned short* pw1 = (unsigned short*)(a.bwd + Bk.w1s);
    unsigned short* pat = (unsigned short*)(a.bwd + Bk.at);
    unsigned short* pwt = (unsigned short*)(a.bwd + Bk.w1t);
    for (int mt = 0; mt < 2; ++mt) {
      const int c = mt_perm(mt, m);
      for (int ks = 0; ks < 2; ++ks) {
        const unsigned short v = HT::from_f32(a.w1[c * 32 + mb_j(8 * ks + e, hi)]);
        const size_t at = ((((size_t)k * 2 + mt) * 2 + ks) * 64 + lane) * 8 + e;
        fw1[at] = v;
        pw1[at] = v;
      }
      for (int ko = 0; ko < 4; ++ko)
        pat[((((size_t)k * 2 + mt) * 4 + ko) * 64 + lane) * 8 + e] = HT::from_f32(a.agg[(size_t)(16 * ko + 8 * hi + e) * 576 + c * 9 + k]);
      // forward A operand: row o = meta_perm(ot, m), elements r = 8 s2 + e of channel 32 mt + 16 hi + r  (mt here: the output tile ot)
      const int o = c;
      for (int mc = 0; mc < 2; ++mc)
        for (int s2 = 0; s2 < 2; ++s2)
          fa2[(((((size_t)k * 2 + mt) * 2 + mc) * 2 + s2) * 64 + lane) * 8 + e] =
              HT::from_f32(a.agg[(size_t)o * 576 + (32 * mc + 16 * hi + 8 * s2 + e) * 9 + k]);
    }
    for (int kc = 0; kc < 4; ++kc)
      pwt[(((size_t)k * 4 + kc) * 64 + lane) * 8 + e] = HT::from_f32(a.w1[(32 * (kc >> 1) + 16 * hi + 8 * (kc & 1) + e) * 32 + m]);
    return;
  }
  idx -= 4608;
  if (idx < 576) {
    const int k = idx >> 6, c = idx & 63;
    double w = a.b1[c];
    if (k == META_CENTRE_TAP)
      for (int j = 0; j < 32; ++j) {
        const double prod = (double)a.w1[c * 32 + j] * (double)(a.b0[j] > 0.f ? a.b0[j] : 0.f);
        w = w + prod;
      }
    const float v = (float)w;
    ((float*)(a.fwd + F.b1p))[idx] = v;
    ((float*)(a.fwd + F.t1))[idx] = 0.f;
    ((float*)(a.bwd + Bk.b1s))[idx] = v;
    ((float*)(a.bwd + Bk.t1))[idx] = 0.f;
    ((float*)(a.bwd + Bk.s1))[idx] = 1.f;
    return;
  }
  idx -= 576;
  if (idx < 64) {
    const int lane = idx, m = lane & 31, hi = lane >> 5;
    unsigned short* fa = (unsigned short*)(a.fwd + F.w0f);
    const float v[4] = {a.w0[m * 3], a.w0[m * 3 + 1], a.w0[m * 3 + 2], a.b0[m]};
    for (int e = 0; e < 4; ++e) {
      const unsigned short h = HT::from_f32(v[e]);
      const unsigned short l = HT::from_f32(v[e] - HT::to_f32(h));
      fa[lane * 8 + e] = hi ? l : h;
      fa[lane * 8 + 4 + e] = (hi || e == 3) ? (unsigned short)0 : h;
    }
    return;
  }
  idx -= 64;
  if (idx < 128) {
    const int j = idx >> 2, i = idx & 3;
    ((float*)(a.bwd + Bk.w0))[idx] = i == 3 ? a.b0[j] : a.w0[j * 3 + i];
    ((float*)(a.fwd + F.w0p))[idx] = 0.f;
    ((float*)(a.fwd + F.s2t2))[idx] = idx < 64 ? 1.f : 0.f;
    return;
  }
  idx -= 128;
  if (idx < 2048) ((float*)(a.bwd + Bk.w1raw))[idx] = a.w1[idx];
}

// ---- launches: the callers (rd_api.hip) have checked pointers, dtype, shape, strides and the workspace --------------------------------------
inline void mt_shape(MetaTrainArgs& a, int waves) {
  a.nfw = (a.W + 31) / 32;
  a.nfrag = mb_frags(a.B, a.H, a.W);
  a.nchunks = (a.nfrag + waves - 1) / waves;
}
#define RD_MT_LAUNCH(dt, KERNEL, grid, block, lds, st, a)                                              \
  do {                                                                                                 \
    static std::atomic<unsigned long long> seen{0};                                                    \
    once_per_device(seen, [] { allow_big_lds(KERNEL<RD_BF16>); allow_big_lds(KERNEL<RD_F16>); });      \
    if ((dt) == RD_F16) hipLaunchKernelGGL(KERNEL<RD_F16>, grid, block, lds, st, a);                   \
    else hipLaunchKernelGGL(KERNEL<RD_BF16>, grid, block, lds, st, a);                                 \
  } while (0)
inline int launch_meta_stats(MetaTrainArgs a, float* mean, float* var, int split, int dt, hipStream_t st) {
  mt_shape(a, MB_WAVES);
  const int S = (int)mb_split(a.B, a.H, a.W, split);
  RD_MT_LAUNCH(dt, meta_stats_kernel, dim3(S, 9), dim3(MB_WAVES * 64), MetaStatsLds::TOTAL, st, a);
  hipLaunchKernelGGL(meta_stats_merge_kernel, dim3(9), dim3(64), 0, st, (const float*)a.part, S, (float)((long)a.B * a.H * a.W), mean, var);
  return check_launch("meta_kernel_stats");
}
inline int launch_meta_fwd_train(MetaTrainArgs a, int dt, hipStream_t st) {
  mt_shape(a, MB_DATA_WAVES);
  const dim3 grid((unsigned)std::min<long>(a.nchunks, conv_num_cus()));
  RD_MT_LAUNCH(dt, meta_fwd_train_kernel, grid, dim3(MB_DATA_WAVES * 64), MetaTrainFwdLds::TOTAL, st, a);
  return check_launch("meta_kernel_fwd_train");
}
inline int launch_meta_train_sums(MetaTrainArgs a, const MetaTrainSumsOut& out, int split, int dt, hipStream_t st) {
  mt_shape(a, MB_WAVES);
  const int S = (int)mb_split(a.B, a.H, a.W, split);
  RD_MT_LAUNCH(dt, meta_train_sums_kernel, dim3(S, 9), dim3(MB_WAVES * 64), MetaTrainSumsLds::TOTAL, st, a);
  hipLaunchKernelGGL(meta_train_sums_reduce_kernel, dim3((MTA_REDUCE_THREADS + 255) / 256), dim3(256), 0, st, (const float*)a.part, S,
                     (float)((long)a.B * a.H * a.W), out);
  return check_launch("meta_kernel_bwd_sums");
}
inline int launch_meta_train_params(MetaTrainArgs a, const MetaTrainParamsOut& out, int split, int dt, hipStream_t st) {
  mt_shape(a, MB_WAVES);
  const int S = (int)mb_split(a.B, a.H, a.W, split);
  RD_MT_LAUNCH(dt, meta_train_params_kernel, dim3(S, 9), dim3(MB_WAVES * 64), MetaTrainParamsLds::TOTAL, st, a);
  hipLaunchKernelGGL(meta_train_params_reduce_kernel, dim3((MTB_REDUCE_THREADS + 255) / 256), dim3(256), 0, st, (const float*)a.part, S, a.packed, out);
  return check_launch("meta_kernel_bwd_params_train");
}
inline int launch_meta_train_data(MetaTrainArgs a, int dt, hipStream_t st) {
  mt_shape(a, MB_DATA_WAVES);
  const dim3 grid((unsigned)std::min<long>(a.nchunks, conv_num_cus()));
  RD_MT_LAUNCH(dt, meta_train_data_kernel, grid, dim3(MB_DATA_WAVES * 64), MetaTrainDataLds::TOTAL, st, a);
  return check_launch("meta_kernel_bwd_data_train");
}
inline int launch_meta_pack_dev(const MetaPackDevArgs& a, int dt, hipStream_t st) {
  RD_LAUNCH_H16(dt, (meta_pack_dev_kernel<DT>), dim3((MT_PACK_THREADS + 255) / 256), dim3(256), st, a);
  return check_launch("pack_meta_dev");
}

}  // namespace rd
