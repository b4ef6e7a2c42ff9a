// Training-mode batch normalisation of a head-tower layer (the reference's normalizer_factory(type="localbn"): mx.sym.BatchNorm with
// fix_gamma=False, use_global_stats=False, momentum 0.9, eps 1e-5 + 1e-10 on every rpn_{cls,reg}_conv_*; mxnext/complicate.py:26-45,
// mxnext/simple.py:502-508, rangedet/symbol/head/builder.py:212-240), forward and backward, on the 16-bit conv output z (channels-last,
// a channel stride and offset like everywhere).  n = B H W pixels, float32 arithmetic throughout, EVERY fused multiply-add is written as
// fmaf and contraction is off in every function of this file: what is not spelled fmaf is a separately rounded operation.
//   bn_stats_partial_kernel + bn_stats_final_kernel      mean[c], biased var[c]
//   bn_fold_kernel                                       rstd, a = gamma rstd, b = beta - mean a, the moving statistics
//   affine_relu_kernel                                   y = round16(max(fmaf(z, a, b), 0))
//   bn_bwd_partial_kernel + bn_bwd_final_kernel          dbeta = sum gy, dgamma = sum gy zh
//   bn_bwd_dz_kernel                                     dz = round16(gamma rstd (gy - c1 - zh c2))
// No atomics; every reduction writes per-workgroup partial sums to the workspace and a second launch adds them in a fixed order.
//
// Work split of every kernel: 256 threads, slots = C / 8 sixteen-byte channel slots per pixel, PL = 256 / slots pixel lanes; thread t owns
// slot t % slots and pixel lane t / slots (so C / 8 is a power of two up to 32: C in {8, 16, 32, 64, 128, 256}).  A reducing launch has
// P = nm_parts(n, split) workgroups = partial sums per channel: min(split > 0 ? split : 1024, ceil(n / 64)), a function of the shape and of
// split only.  Workgroup k owns the pixel run [k n / P, (k + 1) n / P) (integer division: never empty, lengths differ by at most one), a
// thread the pixels lo + lane, lo + lane + PL, ... of it in that order, four at a time: the four 16-byte loads (eight with two tensors) are
// issued before the first use, addresses past the run are clamped to its last pixel and the values dropped, so EXEC stays full.
// A workgroup adds its PL lanes per channel in lane order through LDS.  The final launches add the P partial values of a channel as a
// tree of fixed shape (nm_tree32): thread j of 32 adds k = j, j + 32, ... in that order, then five halving steps through LDS
// (r[j] += r[j + s], s = 16 .. 1).
//
// ---- statistics: ONE sweep over z, sums shifted by a per-workgroup pilot -----------------------------------------------------------------
// (DESIGN.md section 5 compares the bytes with the two-sweep form.)  Workgroup k with n_k pixels, per channel:
//   pilot   p = (v_0 + v_1 + ... + v_{PL-1}) * (1 / PL), added in that order; v_j = z at pixel lo + floor(j n_k / PL): PL samples spread
//           evenly over the run (PL is a power of two: the scaling is exact).  p lies within the range of the run's values.
//   sweep   d = z - p;  S1 += d;  S2 = fmaf(d, d, S2)     per thread in pixel order, then the lanes in lane order
//   partial (p, S1, S2) -> ws[(0, 1, 2) P + k][c]
// final launch, per channel, nf = (float)n_k, N = (float)n:
//   q_k = S1_k / nf;  m_k = p_k + q_k;  M2_k = fmaf(-S1_k, q_k, S2_k)
//   mean = m_0 + tree(nf * (m_k - m_0)) / N
//   e_k = m_k - mean;  var = max(tree(fmaf(nf * e_k, e_k, M2_k)) / N, 0)
// A channel whose values are all the same small integer v gives p = v, d = 0, mean = v in every bit and var = 0 exactly.
//
// ---- fold --------------------------------------------------------------------------------------------------------------------------------
//   rstd = 1.0f / sqrtf(var + eps);  a = gamma * rstd;  b = fmaf(-mean, a, beta)
//   om = 1.0f - momentum;  moving_mean = fmaf(moving_mean, momentum, mean * om)
//   vu = unbiased ? var * ((float)n / (float)(n - 1)) : var;  moving_var = fmaf(moving_var, momentum, vu * om)
//
// ---- backward ----------------------------------------------------------------------------------------------------------------------------
// The ReLU mask is recomputed as [fmaf(z, a, b) > 0]: y is not read, one tensor read fewer per pass.  This differs from a mask on the stored
// y only where a positive float32 value rounds to zero in the 16-bit type (fp16: below 2^-25; bf16 has float32's exponent range).
//   gy = mask ? g : 0;  zh = (z - mean) * rstd                             (two operations)
//   dbeta = sum gy;  dgamma: acc = fmaf(gy, zh, acc)                       per thread in pixel order, lanes in lane order, tree over k
//   c1 = dbeta / N;  c2 = dgamma / N;  gr = gamma * rstd
//   dz = round16(gr * fmaf(-zh, c2, gy - c1))                              one rounding to the activation type
//
// ---- residual form: the second BatchNorm of a backbone BasicBlock (dla_backbone.py:31-45: conv2 -> BN -> + shortcut -> ReLU) ----------------
// r is the shortcut in the activation type: the block input (identity, ar = br = NULL) or the output zs of the 1x1 projection conv, whose own
// BatchNorm is folded into ar, br (rd_bn_stats and rd_bn_fold on zs).  The same work split, the same clamped loads, one more tensor each.
//   affine_add_relu_kernel                               t = fmaf(z, a, b);  u = ar ? fmaf(r, ar, br) : r;  v = t + u (a rounding of its own)
//                                                        y = round16(relu ? max(v, 0) : v)
//   bn_add_bwd_partial_kernel + bn_add_bwd_final_kernel  one sweep over g, z, r: the mask is [t + u > 0] with t, u, and their sum formed exactly as
//                                                        above (y is not read);  gy = mask ? g : 0;  zh = (z - mean) * rstd
//                                                        dbeta = sum gy;  dgamma: acc = fmaf(gy, zh, acc)
//                                                        projection: zhr = (r - mean_r) * rstd_r;  dgamma_r: acc = fmaf(gy, zhr, acc);  dbeta_r = dbeta
//                                                        (two or three partial sums per workgroup and channel, ws[(0, 1, 2) P + k][c], then nm_tree32)
//   bn_add_bwd_dzdr_kernel                               c1 = dbeta / N;  c2 = dgamma / N;  dz = round16(gamma * rstd * fmaf(-zh, c2, gy - c1))
//                                                        identity:    dr = gy (its 16 bits are those of g, or +0)
//                                                        projection:  c2r = dgamma_r / N;  dr = round16(gamma_r * rstd_r * fmaf(-zhr, c2r, gy - c1))
//                                                        one launch reads g, z, r once more and writes both tensors
#pragma once
#include "rd_common.h"

namespace rd {
constexpr int NM_MAX_PARTS = 1024;   // partial sums per channel with the library's own split: four workgroups per CU of a 256-CU part
constexpr int NM_MIN_PIXELS = 64;    // pixels of a workgroup before a second one is worth its workspace slot
constexpr int NM_UNROLL = 4;         // pixels of a thread in flight
constexpr int NM_EW_ITERS = 4;       // elementwise launches: NM_EW_ITERS * NM_UNROLL pixels per thread
constexpr int NM_KL = 32;            // threads per channel of a final launch

inline bool nm_channels_ok(int C) { return C == 8 || C == 16 || C == 32 || C == 64 || C == 128 || C == 256; }
inline long nm_parts(long npix, int split) {
  const long nb = (npix + NM_MIN_PIXELS - 1) / NM_MIN_PIXELS, cap = split > 0 ? split : NM_MAX_PARTS;
  return nb < cap ? nb : cap;
}
inline long nm_ew_blocks(long npix, int C) {
  const long per = (long)(2048 / C) * NM_UNROLL * NM_EW_ITERS;
  return (npix + per - 1) / per;
}

// NM_UNROLL pixels q0, q0 + PL, ... of one slot; an address at or past `hi` reads pixel hi - 1 (the caller drops the value)
__device__ __forceinline__ void nm_load(const unsigned short* __restrict__ base, int cs, long q0, int PL, long hi, Slot16 (&v)[NM_UNROLL]) {
#pragma unroll
  for (int u = 0; u < NM_UNROLL; ++u) {
    const long q = q0 + (long)u * PL, qc = q < hi ? q : hi - 1;
    v[u] = *(const Slot16*)(base + qc * cs);
  }
}
// one value per (kl, cl) -> the sum over kl of channel cl, the same in all 32 threads of the channel; every thread of the block calls it
__device__ __forceinline__ float nm_tree32(float v, float (*red)[8], int kl, int cl) {
  _Pragma("clang fp contract(off)")
  red[kl][cl] = v;
  __syncthreads();
  for (int s = NM_KL / 2; s >= 1; s >>= 1) {
    if (kl < s) red[kl][cl] += red[kl + s][cl];
    __syncthreads();
  }
  const float r = red[0][cl];
  __syncthreads();
  return r;
}

// ---- statistics --------------------------------------------------------------------------------------------------------------------------
struct NmStatsArgs {
  const unsigned short* z;
  int cs, co, C, P;
  long npix;
  float* part;   // [3][P][C]: pilot, S1, S2
};

template <int DT>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(NmStatsArgs a) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[2][2048];
  __shared__ float pil[256];
  const int C = a.C, slots = C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long k = blockIdx.x, lo = k * a.npix / a.P, hi = (k + 1) * a.npix / a.P, nk = hi - lo;
  const unsigned short* zb = a.z + a.co + 8 * sl;
  float f[8];
  slot_unpack<DT>(*(const Slot16*)(zb + (lo + (long)pl * nk / PL) * a.cs), f);
#pragma unroll
  for (int j = 0; j < 8; ++j) red[0][pl * C + 8 * sl + j] = f[j];
  __syncthreads();
  if (tid < C) pil[tid] = lane_sum(red[0], PL, C, tid) * (1.0f / PL);
  __syncthreads();
  float p[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    p[j] = pil[8 * sl + j];
    s1[j] = 0.f;
    s2[j] = 0.f;
  }
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 v[NM_UNROLL];
    nm_load(zb, a.cs, q0, PL, hi, v);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const bool ok = q0 + (long)u * PL < hi;
      slot_unpack<DT>(v[u], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = ok ? f[j] - p[j] : 0.f;
        s1[j] += d;
        s2[j] = fmaf(d, d, s2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][pl * C + 8 * sl + j] = s1[j];
    red[1][pl * C + 8 * sl + j] = s2[j];
  }
  __syncthreads();
  if (tid < C) {
    a.part[k * C + tid] = pil[tid];
    a.part[((long)a.P + k) * C + tid] = lane_sum(red[0], PL, C, tid);
    a.part[(2L * a.P + k) * C + tid] = lane_sum(red[1], PL, C, tid);
  }
}

// grid C / 8, 256 threads: channel 8 blockIdx.x + (tid & 7), partial lane tid >> 3
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int P, int C, long npix, float* __restrict__ mean,
                                                             float* __restrict__ var) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[NM_KL][8];
  const int cl = threadIdx.x & 7, kl = threadIdx.x >> 3, c = 8 * blockIdx.x + cl;
  const float N = (float)npix;
  const float* pp = part + c;
  const float* p1 = part + (long)P * C + c;
  const float* p2 = part + 2L * P * C + c;
  const float m0 = pp[0] + p1[0] / (float)(npix / P);
  float acc = 0.f;
  for (long k = kl; k < P; k += NM_KL) {
    const float nf = (float)((k + 1) * npix / P - k * npix / P);
    const float mk = pp[k * C] + p1[k * C] / nf;
    acc += nf * (mk - m0);
  }
  const float mu = m0 + nm_tree32(acc, red, kl, cl) / N;
  acc = 0.f;
  for (long k = kl; k < P; k += NM_KL) {
    const float nf = (float)((k + 1) * npix / P - k * npix / P);
    const float S1 = p1[k * C], q = S1 / nf, mk = pp[k * C] + q, e = mk - mu;
    acc += fmaf(nf * e, e, fmaf(-S1, q, p2[k * C]));
  }
  const float v = nm_tree32(acc, red, kl, cl) / N;
  if (kl == 0) {
    mean[c] = mu;
    var[c] = fmaxf(v, 0.f);
  }
}

// ---- fold --------------------------------------------------------------------------------------------------------------------------------
struct NmFoldArgs {
  const float *mean, *var, *gamma, *beta;
  float eps, momentum, nratio;   // nratio: n / (n - 1), or 0: biased
  float *rstd, *a, *b, *mmean, *mvar;
  int C;
};
__global__ __launch_bounds__(256) void bn_fold_kernel(NmFoldArgs a) {
  _Pragma("clang fp contract(off)")
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.C) return;
  const float mu = a.mean[c], v = a.var[c];
  const float rstd = 1.0f / sqrtf(v + a.eps);
  const float sa = a.gamma[c] * rstd;
  a.rstd[c] = rstd;
  a.a[c] = sa;
  a.b[c] = fmaf(-mu, sa, a.beta[c]);
  const float om = 1.0f - a.momentum;
  if (a.mmean) a.mmean[c] = fmaf(a.mmean[c], a.momentum, mu * om);
  if (a.mvar) {
    const float vu = a.nratio != 0.f ? v * a.nratio : v;
    a.mvar[c] = fmaf(a.mvar[c], a.momentum, vu * om);
  }
}

// ---- y = round16(max(fmaf(z, a, b), 0)) ----------------------------------------------------------------------------------------------------
struct NmAffineArgs {
  const unsigned short* z;
  int z_cs, z_co;
  const float *a, *b;
  int relu;
  unsigned short* y;
  int y_cs, y_co, C;
  long npix;
};
template <int DT>
__global__ __launch_bounds__(256) void affine_relu_kernel(NmAffineArgs a) {
  _Pragma("clang fp contract(off)")
  const int slots = a.C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long per = (long)PL * NM_UNROLL * NM_EW_ITERS, lo = blockIdx.x * per, hi = lo + per < a.npix ? lo + per : a.npix;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  unsigned short* yb = a.y + a.y_co + 8 * sl;
  float sa[8], sb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sa[j] = a.a[8 * sl + j];
    sb[j] = a.b[8 * sl + j];
  }
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 v[NM_UNROLL];
    nm_load(zb, a.z_cs, q0, PL, hi, v);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const long q = q0 + (long)u * PL;
      float f[8];
      slot_unpack<DT>(v[u], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = fmaf(f[j], sa[j], sb[j]);
        f[j] = a.relu ? fmaxf(t, 0.f) : t;
      }
      if (q < hi) *(Slot16*)(yb + q * a.y_cs) = slot_pack<DT>(f);
    }
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
struct NmBwdArgs {
  const unsigned short *g, *z;
  int g_cs, g_co, z_cs, z_co;
  const float *a, *b, *mean, *rstd, *gamma;
  int relu;
  unsigned short* dz;
  int dz_cs, dz_co, C, P;
  long npix;
  float* part;                  // [2][P][C]: sum gy, sum gy zh
  const float *dgamma, *dbeta;  // the dz launch reads the sums the final launch wrote
};

template <int DT>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(NmBwdArgs a) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[2][2048];
  const int C = a.C, slots = C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long k = blockIdx.x, lo = k * a.npix / a.P, hi = (k + 1) * a.npix / a.P;
  const unsigned short* gb = a.g + a.g_co + 8 * sl;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  float sa[8], sb[8], mu[8], rs[8], sg[8], sz[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sa[j] = a.relu ? a.a[8 * sl + j] : 0.f;
    sb[j] = a.relu ? a.b[8 * sl + j] : 0.f;
    mu[j] = a.mean[8 * sl + j];
    rs[j] = a.rstd[8 * sl + j];
    sg[j] = 0.f;
    sz[j] = 0.f;
  }
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vg[NM_UNROLL], vz[NM_UNROLL];
    nm_load(gb, a.g_cs, q0, PL, hi, vg);
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const bool ok = q0 + (long)u * PL < hi;
      float fg[8], fz[8];
      slot_unpack<DT>(vg[u], fg);
      slot_unpack<DT>(vz[u], fz);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool on = ok && (!a.relu || fmaf(fz[j], sa[j], sb[j]) > 0.f);
        const float gy = on ? fg[j] : 0.f;
        const float zh = (fz[j] - mu[j]) * rs[j];
        sg[j] += gy;
        sz[j] = fmaf(gy, zh, sz[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][pl * C + 8 * sl + j] = sg[j];
    red[1][pl * C + 8 * sl + j] = sz[j];
  }
  __syncthreads();
  if (tid < C) {
    a.part[k * C + tid] = lane_sum(red[0], PL, C, tid);
    a.part[((long)a.P + k) * C + tid] = lane_sum(red[1], PL, C, tid);
  }
}

// grid (C / 8, 2): blockIdx.y 0 -> dbeta, 1 -> dgamma
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ part, int P, int C, float* __restrict__ dbeta,
                                                           float* __restrict__ dgamma) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[NM_KL][8];
  const int cl = threadIdx.x & 7, kl = threadIdx.x >> 3, c = 8 * blockIdx.x + cl;
  const float* p = part + (long)blockIdx.y * P * C + c;
  float acc = 0.f;
  for (long k = kl; k < P; k += NM_KL) acc += p[k * C];
  const float s = nm_tree32(acc, red, kl, cl);
  if (kl == 0) (blockIdx.y ? dgamma : dbeta)[c] = s;
}

template <int DT>
__global__ __launch_bounds__(256) void bn_bwd_dz_kernel(NmBwdArgs a) {
  _Pragma("clang fp contract(off)")
  const int slots = a.C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long per = (long)PL * NM_UNROLL * NM_EW_ITERS, lo = blockIdx.x * per, hi = lo + per < a.npix ? lo + per : a.npix;
  const unsigned short* gb = a.g + a.g_co + 8 * sl;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  unsigned short* ob = a.dz + a.dz_co + 8 * sl;
  const float N = (float)a.npix;
  float sa[8], sb[8], mu[8], rs[8], gr[8], c1[8], c2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * sl + j;
    sa[j] = a.relu ? a.a[c] : 0.f;
    sb[j] = a.relu ? a.b[c] : 0.f;
    mu[j] = a.mean[c];
    rs[j] = a.rstd[c];
    gr[j] = a.gamma[c] * rs[j];
    c1[j] = a.dbeta[c] / N;
    c2[j] = a.dgamma[c] / N;
  }
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vg[NM_UNROLL], vz[NM_UNROLL];
    nm_load(gb, a.g_cs, q0, PL, hi, vg);
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const long q = q0 + (long)u * PL;
      float fg[8], fz[8];
      slot_unpack<DT>(vg[u], fg);
      slot_unpack<DT>(vz[u], fz);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool on = !a.relu || fmaf(fz[j], sa[j], sb[j]) > 0.f;
        const float gy = on ? fg[j] : 0.f;
        const float zh = (fz[j] - mu[j]) * rs[j];
        fg[j] = gr[j] * fmaf(-zh, c2[j], gy - c1[j]);
      }
      if (q < hi) *(Slot16*)(ob + q * a.dz_cs) = slot_pack<DT>(fg);
    }
  }
}

// ---- residual form: y = round16(max(fmaf(z, a, b) + u, 0)), u = r or fmaf(r, ar, br) ------------------------------------------------------------
struct NmAddArgs {
  const unsigned short *z, *r;
  int z_cs, z_co, r_cs, r_co;
  const float *a, *b, *ar, *br;   // ar, br: both NULL for an identity shortcut
  int relu;
  unsigned short* y;
  int y_cs, y_co, C;
  long npix;
};
// the eight per-channel values of a slot; p == nullptr gives `dflt`
__device__ __forceinline__ void nm_vec8(const float* __restrict__ p, int sl, float dflt, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = p ? p[8 * sl + j] : dflt;
}
// v = fmaf(z, a, b) + u: what the forward rounds and the backward takes the sign of
template <bool PROJ>
__device__ __forceinline__ float nm_add_pre(float z, float r, float sa, float sb, float ra, float rb) {
  _Pragma("clang fp contract(off)")
  const float t = fmaf(z, sa, sb);
  const float u = PROJ ? fmaf(r, ra, rb) : r;
  return t + u;
}

template <int DT, bool PROJ>
__global__ __launch_bounds__(256) void affine_add_relu_kernel(NmAddArgs a) {
  _Pragma("clang fp contract(off)")
  const int slots = a.C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long per = (long)PL * NM_UNROLL * NM_EW_ITERS, lo = blockIdx.x * per, hi = lo + per < a.npix ? lo + per : a.npix;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  const unsigned short* rb = a.r + a.r_co + 8 * sl;
  unsigned short* yb = a.y + a.y_co + 8 * sl;
  float sa[8], sb[8], ra[8], rbv[8];
  nm_vec8(a.a, sl, 0.f, sa);
  nm_vec8(a.b, sl, 0.f, sb);
  nm_vec8(PROJ ? a.ar : nullptr, sl, 0.f, ra);
  nm_vec8(PROJ ? a.br : nullptr, sl, 0.f, rbv);
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vz[NM_UNROLL], vr[NM_UNROLL];
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
    nm_load(rb, a.r_cs, q0, PL, hi, vr);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const long q = q0 + (long)u * PL;
      float fz[8], fr[8];
      slot_unpack<DT>(vz[u], fz);
      slot_unpack<DT>(vr[u], fr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = nm_add_pre<PROJ>(fz[j], fr[j], sa[j], sb[j], ra[j], rbv[j]);
        fz[j] = a.relu ? fmaxf(v, 0.f) : v;
      }
      if (q < hi) *(Slot16*)(yb + q * a.y_cs) = slot_pack<DT>(fz);
    }
  }
}

// ---- the join of an aggregation stage: y = round16(max(fmaf(z, a, b), 0) + r) ------------------------------------------------------------------
// (dla_backbone.py agg_stage: Deconvolution -> BatchNorm -> ReLU -> add(skip, .)).  The ReLU comes BEFORE the add: max(t, 0) is t where
// t > 0 and +0 elsewhere (a -0 or a NaN pre-activation gives +0), then one float32 add of the skip r and one rounding.  NmAddArgs with
// ar = br = NULL; `relu` is not read.  No backward launch of its own: the up-branch gradient is rd_bn_relu_bwd on z (the mask is
// [fmaf(z, a, b) > 0], the same comparison), the skip gradient is g itself.
template <int DT>
__global__ __launch_bounds__(256) void affine_relu_add_kernel(NmAddArgs a) {
  _Pragma("clang fp contract(off)")
  const int slots = a.C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long per = (long)PL * NM_UNROLL * NM_EW_ITERS, lo = blockIdx.x * per, hi = lo + per < a.npix ? lo + per : a.npix;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  const unsigned short* rb = a.r + a.r_co + 8 * sl;
  unsigned short* yb = a.y + a.y_co + 8 * sl;
  float sa[8], sb[8];
  nm_vec8(a.a, sl, 0.f, sa);
  nm_vec8(a.b, sl, 0.f, sb);
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vz[NM_UNROLL], vr[NM_UNROLL];
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
    nm_load(rb, a.r_cs, q0, PL, hi, vr);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const long q = q0 + (long)u * PL;
      float fz[8], fr[8];
      slot_unpack<DT>(vz[u], fz);
      slot_unpack<DT>(vr[u], fr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = fmaf(fz[j], sa[j], sb[j]);
        fz[j] = (t > 0.f ? t : 0.f) + fr[j];
      }
      if (q < hi) *(Slot16*)(yb + q * a.y_cs) = slot_pack<DT>(fz);
    }
  }
}

struct NmAddBwdArgs {
  const unsigned short *g, *z, *r;
  int g_cs, g_co, z_cs, z_co, r_cs, r_co;
  const float *a, *b, *mean, *rstd, *gamma;
  const float *ar, *br, *mean_r, *rstd_r, *gamma_r;   // all NULL for an identity shortcut
  unsigned short *dz, *dr;
  int dz_cs, dz_co, dr_cs, dr_co, C, P;
  long npix;
  float* part;                             // [2 or 3][P][C]: sum gy, sum gy zh, sum gy zhr
  const float *dbeta, *dgamma, *dgamma_r;  // the dz / dr launch reads the sums the final launch wrote
};

template <int DT, bool PROJ>
__global__ __launch_bounds__(256) void bn_add_bwd_partial_kernel(NmAddBwdArgs a) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[PROJ ? 3 : 2][2048];
  const int C = a.C, slots = C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long k = blockIdx.x, lo = k * a.npix / a.P, hi = (k + 1) * a.npix / a.P;
  const unsigned short* gb = a.g + a.g_co + 8 * sl;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  const unsigned short* rb = a.r + a.r_co + 8 * sl;
  float sa[8], sb[8], mu[8], rs[8], ra[8], rbv[8], mur[8], rsr[8], sg[8], sz[8], sr[8];
  nm_vec8(a.a, sl, 0.f, sa);
  nm_vec8(a.b, sl, 0.f, sb);
  nm_vec8(a.mean, sl, 0.f, mu);
  nm_vec8(a.rstd, sl, 0.f, rs);
  nm_vec8(PROJ ? a.ar : nullptr, sl, 0.f, ra);
  nm_vec8(PROJ ? a.br : nullptr, sl, 0.f, rbv);
  nm_vec8(PROJ ? a.mean_r : nullptr, sl, 0.f, mur);
  nm_vec8(PROJ ? a.rstd_r : nullptr, sl, 0.f, rsr);
#pragma unroll
  for (int j = 0; j < 8; ++j) sg[j] = sz[j] = sr[j] = 0.f;
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vg[NM_UNROLL], vz[NM_UNROLL], vr[NM_UNROLL];
    nm_load(gb, a.g_cs, q0, PL, hi, vg);
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
    nm_load(rb, a.r_cs, q0, PL, hi, vr);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const bool ok = q0 + (long)u * PL < hi;
      float fg[8], fz[8], fr[8];
      slot_unpack<DT>(vg[u], fg);
      slot_unpack<DT>(vz[u], fz);
      slot_unpack<DT>(vr[u], fr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool on = ok && nm_add_pre<PROJ>(fz[j], fr[j], sa[j], sb[j], ra[j], rbv[j]) > 0.f;
        const float gy = on ? fg[j] : 0.f;
        const float zh = (fz[j] - mu[j]) * rs[j];
        sg[j] += gy;
        sz[j] = fmaf(gy, zh, sz[j]);
        if (PROJ) {
          const float zhr = (fr[j] - mur[j]) * rsr[j];
          sr[j] = fmaf(gy, zhr, sr[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][pl * C + 8 * sl + j] = sg[j];
    red[1][pl * C + 8 * sl + j] = sz[j];
    if (PROJ) red[2][pl * C + 8 * sl + j] = sr[j];
  }
  __syncthreads();
  if (tid < C) {
    a.part[k * C + tid] = lane_sum(red[0], PL, C, tid);
    a.part[((long)a.P + k) * C + tid] = lane_sum(red[1], PL, C, tid);
    if (PROJ) a.part[(2L * a.P + k) * C + tid] = lane_sum(red[2], PL, C, tid);
  }
}

// grid (C / 8, 2 or 3): blockIdx.y 0 -> dbeta (and dbeta_r, the same value), 1 -> dgamma, 2 -> dgamma_r
__global__ __launch_bounds__(256) void bn_add_bwd_final_kernel(const float* __restrict__ part, int P, int C, float* __restrict__ dbeta,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta_r,
                                                               float* __restrict__ dgamma_r) {
  _Pragma("clang fp contract(off)")
  __shared__ float red[NM_KL][8];
  const int cl = threadIdx.x & 7, kl = threadIdx.x >> 3, c = 8 * blockIdx.x + cl;
  const float* p = part + (long)blockIdx.y * P * C + c;
  float acc = 0.f;
  for (long k = kl; k < P; k += NM_KL) acc += p[k * C];
  const float s = nm_tree32(acc, red, kl, cl);
  if (kl != 0) return;
  if (blockIdx.y == 0) {
    dbeta[c] = s;
    if (dbeta_r) dbeta_r[c] = s;
  } else {
    (blockIdx.y == 1 ? dgamma : dgamma_r)[c] = s;
  }
}

template <int DT, bool PROJ>
__global__ __launch_bounds__(256) void bn_add_bwd_dzdr_kernel(NmAddBwdArgs a) {
  _Pragma("clang fp contract(off)")
  const int slots = a.C / 8, PL = 256 / slots, tid = threadIdx.x, sl = tid % slots, pl = tid / slots;
  const long per = (long)PL * NM_UNROLL * NM_EW_ITERS, lo = blockIdx.x * per, hi = lo + per < a.npix ? lo + per : a.npix;
  const unsigned short* gb = a.g + a.g_co + 8 * sl;
  const unsigned short* zb = a.z + a.z_co + 8 * sl;
  const unsigned short* rb = a.r + a.r_co + 8 * sl;
  unsigned short* ozb = a.dz + a.dz_co + 8 * sl;
  unsigned short* orb = a.dr + a.dr_co + 8 * sl;
  const float N = (float)a.npix;
  float sa[8], sb[8], mu[8], rs[8], ra[8], rbv[8], mur[8], rsr[8], gr[8], grr[8], c1[8], c2[8], c2r[8];
  nm_vec8(a.a, sl, 0.f, sa);
  nm_vec8(a.b, sl, 0.f, sb);
  nm_vec8(a.mean, sl, 0.f, mu);
  nm_vec8(a.rstd, sl, 0.f, rs);
  nm_vec8(PROJ ? a.ar : nullptr, sl, 0.f, ra);
  nm_vec8(PROJ ? a.br : nullptr, sl, 0.f, rbv);
  nm_vec8(PROJ ? a.mean_r : nullptr, sl, 0.f, mur);
  nm_vec8(PROJ ? a.rstd_r : nullptr, sl, 0.f, rsr);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * sl + j;
    gr[j] = a.gamma[c] * rs[j];
    c1[j] = a.dbeta[c] / N;
    c2[j] = a.dgamma[c] / N;
    grr[j] = PROJ ? a.gamma_r[c] * rsr[j] : 0.f;
    c2r[j] = PROJ ? a.dgamma_r[c] / N : 0.f;
  }
  for (long q0 = lo + pl; q0 < hi; q0 += (long)NM_UNROLL * PL) {
    Slot16 vg[NM_UNROLL], vz[NM_UNROLL], vr[NM_UNROLL];
    nm_load(gb, a.g_cs, q0, PL, hi, vg);
    nm_load(zb, a.z_cs, q0, PL, hi, vz);
    nm_load(rb, a.r_cs, q0, PL, hi, vr);
#pragma unroll
    for (int u = 0; u < NM_UNROLL; ++u) {
      const long q = q0 + (long)u * PL;
      float fg[8], fz[8], fr[8];
      slot_unpack<DT>(vg[u], fg);
      slot_unpack<DT>(vz[u], fz);
      slot_unpack<DT>(vr[u], fr);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool on = nm_add_pre<PROJ>(fz[j], fr[j], sa[j], sb[j], ra[j], rbv[j]) > 0.f;
        const float gy = on ? fg[j] : 0.f;
        const float zh = (fz[j] - mu[j]) * rs[j];
        const float d = gy - c1[j];
        fz[j] = gr[j] * fmaf(-zh, c2[j], d);
        if (PROJ) {
          const float zhr = (fr[j] - mur[j]) * rsr[j];
          fr[j] = grr[j] * fmaf(-zhr, c2r[j], d);
        } else {
          fr[j] = gy;
        }
      }
      if (q < hi) {
        *(Slot16*)(ozb + q * a.dz_cs) = slot_pack<DT>(fz);
        *(Slot16*)(orb + q * a.dr_cs) = slot_pack<DT>(fr);
      }
    }
  }
}
}  // namespace rd
