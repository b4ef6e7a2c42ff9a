// RPN loss head of one pyramid level (rangedet/symbol/head/builder.py:156-196,268-422 and rangedet/symbol/head/loss.py:4-30 in the
// reference): IoU target (Decode3DBbox + 'bev' batch_rotated_iou, block_grad), varifocal loss, normalised smooth-L1 / L1 loss, and the
// gradients MakeLoss sends back to the logits and the deltas.  Two phases, each a kernel and a single-block finishing kernel:
//   1  norm_cls = float(sum mask) + 1, norm_reg = float(sum reg_normalize_weight) + 1 over the whole batch (builder.py:366,411)
//   2  one thread per pixel: decode in registers, max cleaned IoU over the frame's GT boxes (in LDS), both losses, both gradients
// Every sum is a double: thread, wave (__shfl_xor), block, one partial per block in a workspace slot indexed by the block id; the finishing
// kernel adds the slots in index order.  No atomics: the result does not depend on scheduling.
#pragma once
#include "k_misc.h"
#include "k_riou.h"

namespace rd {
constexpr int LOSS_NORM_MAX_BLOCKS = 1024;
constexpr int LOSS_NORM_FLOATS_PER_BLOCK = 256 * 16;   // four float4 per thread before a second block is worth its launch slot

inline int loss_norm_blocks(int B, long n) {
  const long nb = ((long)B * n * 8 + LOSS_NORM_FLOATS_PER_BLOCK - 1) / LOSS_NORM_FLOATS_PER_BLOCK;
  return (int)(nb < 1 ? 1 : nb > LOSS_NORM_MAX_BLOCKS ? LOSS_NORM_MAX_BLOCKS : nb);
}
inline long loss_pixel_blocks(int B, long n) { return (long)B * ((n + 255) / 256); }
// workspace: doubles [mask partials | norm-weight partials] (phase 1), [cls_loss partials | reg_loss partials] (phase 2)
inline size_t loss_ws_bytes(int B, long n) { return (2 * (size_t)loss_norm_blocks(B, n) + 2 * (size_t)loss_pixel_blocks(B, n)) * sizeof(double); }

struct LossArgs {
  const float *logit, *delta, *pc, *gt, *mask, *reg_target, *reg_weight, *reg_norm_weight;
  long logit_bs, delta_bs, n;
  int B, ngt;
  rd_loss_param_t p;
  float *cls_loss, *reg_loss, *d_logit, *d_delta, *iou_target, *boxes10;
  float* stats;          // [0], [1]: the norms, written by phase 1 and read by phase 2
  double *part_mask, *part_nw, *part_cls, *part_reg;
  int norm_blocks;
};

// block sum of one double per thread (256 threads); the value is valid in thread 0.  Fixed order: xor butterfly in the wave, then wave 0..3.
__device__ __forceinline__ double loss_block_sum(double v, double* lds4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}
// this thread's share of sum p[0..len): scalar head up to a 16-byte boundary, float4 body, scalar tail
__device__ __forceinline__ double loss_thread_sum(const float* __restrict__ p, long len, long tid, long nthreads) {
  long head = (long)((16 - ((uintptr_t)p & 15)) & 15) / 4;
  if (head > len) head = len;
  const long n4 = (len - head) / 4, tail0 = head + n4 * 4;
  double acc = 0.0;
  if (tid < head) acc += (double)p[tid];
  const float4* q = (const float4*)(p + head);
  for (long i = tid; i < n4; i += nthreads) {
    const float4 v = q[i];
    acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
  }
  if (tid < len - tail0) acc += (double)p[tail0 + tid];
  return acc;
}
__global__ __launch_bounds__(256) void loss_norm_kernel(LossArgs a) {
  __shared__ double red[8];
  const long tid = blockIdx.x * 256L + threadIdx.x, nthreads = gridDim.x * 256L;
  const double sm = loss_block_sum(loss_thread_sum(a.mask, a.B * a.n, tid, nthreads), red);
  const double sw = loss_block_sum(loss_thread_sum(a.reg_norm_weight, a.B * a.n * 8, tid, nthreads), red + 4);
  if (threadIdx.x == 0) { a.part_mask[blockIdx.x] = sm; a.part_nw[blockIdx.x] = sw; }
}
// out[k] = float(sum part_k[0..count)) + add, k = 0, 1.  One block: thread t adds its contiguous run of slots in index order, thread 0 the
// 256 runs in index order.
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ part0, const double* __restrict__ part1, long count,
                                                          float add, float* __restrict__ out) {
  __shared__ double run[2][256];
  const long per = (count + 255) / 256, lo = threadIdx.x * per, hi = lo + per < count ? lo + per : count;
  double s0 = 0.0, s1 = 0.0;
  for (long i = lo; i < hi; ++i) { s0 += part0[i]; s1 += part1[i]; }
  run[0][threadIdx.x] = s0;
  run[1][threadIdx.x] = s1;
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int t = 0; t < 256; ++t) s += run[threadIdx.x][t];
    out[threadIdx.x] = (float)s + add;
  }
}

// loss.py:4-30 with loss_scale = 1 and the inner alpha = 0.5, x = logit, s = IoU target: the loss before mask and norm, and its
// derivative in x (s behind block_grad, pred_sigmoid not)
__device__ __forceinline__ void loss_varifocal(float x, float s, float alpha, float gamma, float& vfl, float& dvfl) {
  RD_NOCONTRACT_R
  const float p = 1.0f / (1.0f + expf(-x));
  const float lo = 1e-6f, hi = 1.0f - 1e-6f;
  const float Lp = logf(fminf(fmaxf(p, lo), hi));
  const bool ge = x >= 0.0f;
  const float Lm = (ge ? -x : 0.0f) - log1pf(expf(ge ? -x : x));
  const float L0 = -1.0f * (0.5f * s * Lp + 0.5f * (1.0f - s) * Lm) * 2.0f;
  const float c = (p >= lo && p <= hi) ? 1.0f : 0.0f;                      // the gradient of clip is 1 at the bounds
  const float dL0 = -(s * c * (1.0f - p) - (1.0f - s) * p);
  if (s > 0.0f) {
    vfl = L0 * s;
    dvfl = s * dL0;
  } else {                                                                 // s == 0: |s - p| = p
    const float pg1 = gamma == 2.0f ? p : powf(p, gamma - 1.0f);           // p^(gamma-1)
    const float pg = pg1 * p;
    vfl = L0 * alpha * pg;
    dvfl = alpha * (dL0 * pg + L0 * gamma * pg1 * p * (1.0f - p));
  }
}

__global__ __launch_bounds__(256) void loss_pixel_kernel(LossArgs a) {
  __shared__ float g[256 * 8];
  __shared__ float gb[256 * 4];   // min x, max x, min y, max y
  __shared__ double red[8];
  const int b = blockIdx.y;
  const float* gt = a.gt + (long)b * a.ngt * 8;
  // the frame's GT boxes and bounds, as batch_riou_kernel (k_riou.h) loads them
  for (int i = threadIdx.x; i < a.ngt * 8; i += 256) g[i] = gt[i];
  __syncthreads();
  for (int j = threadIdx.x; j < a.ngt; j += 256) {
    const float* q = g + j * 8;
    gb[4 * j + 0] = fminf(fminf(q[0], q[2]), fminf(q[4], q[6]));
    gb[4 * j + 1] = fmaxf(fmaxf(q[0], q[2]), fmaxf(q[4], q[6]));
    gb[4 * j + 2] = fminf(fminf(q[1], q[3]), fminf(q[5], q[7]));
    gb[4 * j + 3] = fmaxf(fmaxf(q[1], q[3]), fmaxf(q[5], q[7]));
    bool nan = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) nan |= !(q[c] == q[c]);
    if (nan) { gb[4 * j + 0] = -INFINITY; gb[4 * j + 1] = INFINITY; gb[4 * j + 2] = -INFINITY; gb[4 * j + 3] = INFINITY; }
  }
  __syncthreads();
  const long n = a.n, i = blockIdx.x * 256L + threadIdx.x;
  double sum_cls = 0.0, sum_reg = 0.0;
  if (i < n) {
    const float norm_cls = a.stats[0], norm_reg = a.stats[1];
    const float4 d0 = *(const float4*)(a.delta + b * a.delta_bs + i * 8), d1 = *(const float4*)(a.delta + b * a.delta_bs + i * 8 + 4);
    const float d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    const float* pc = a.pc + (b * n + i) * 3;
    float box[10];
    decode3d_box(d, pc[0], pc[1], pc[2], 0, box);
    if (a.boxes10) {
      float* o = a.boxes10 + (b * n + i) * 10;
#pragma unroll
      for (int k = 0; k < 10; ++k) o[k] = box[k];
    }
    // IoU target: the loop of batch_riou_kernel
    const float lx = fminf(fminf(box[0], box[2]), fminf(box[4], box[6])), hx = fmaxf(fmaxf(box[0], box[2]), fmaxf(box[4], box[6]));
    const float ly = fminf(fminf(box[1], box[3]), fminf(box[5], box[7])), hy = fmaxf(fmaxf(box[1], box[3]), fmaxf(box[5], box[7]));
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) finite &= box[k] == box[k];
    float s = 0.f;
    for (int j = 0; j < a.ngt; ++j) {
      float v = 0.f;
      const bool apart = hx < gb[4 * j] || gb[4 * j + 1] < lx || hy < gb[4 * j + 2] || gb[4 * j + 3] < ly;
      if (!(finite && apart)) {
        v = r_iou8(box, g + j * 8);
        if (!(v == v) || isinf(v) || v > 1.0f || v < 0.f) v = 0.f;
      }
      if (v > s) s = v;
    }
    if (a.iou_target) a.iou_target[b * n + i] = s;
    {  // classification (builder.py:350-379)
      RD_NOCONTRACT_R
      float vfl, dvfl;
      loss_varifocal(a.logit[b * a.logit_bs + i], s, a.p.alpha, a.p.gamma, vfl, dvfl);
      const float m = a.mask[b * n + i];
      const float cl = vfl * m / norm_cls;
      a.cls_loss[b * n + i] = cl;
      sum_cls = (double)cl;
      if (a.d_logit) a.d_logit[b * a.logit_bs + i] = a.p.scale_loss_shift * a.p.cls_loss_weight * m / norm_cls * dvfl;
    }
    {  // regression (builder.py:381-422); MXNet smooth_l1 with scalar sigma
      RD_NOCONTRACT_R
      const float sig2 = a.p.smooth_l1_scalar * a.p.smooth_l1_scalar, inv = 1.0f / sig2;
      const float gs = a.p.scale_loss_shift * a.p.reg_loss_weight;
      float dd[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const long k = (b * 8L + c) * n + i;                      // plane c of the NCHW tensors: coalesced across the wave
        const float xr = d[c] - a.reg_target[k], ax = fabsf(xr);
        const float wn = a.reg_weight[k] * a.reg_norm_weight[k];
        const float sgn = xr > 0.f ? 1.f : xr < 0.f ? -1.f : 0.f;
        float l, dl;
        if (a.p.l1) { l = ax; dl = sgn; }
        else if (ax < inv) { l = 0.5f * sig2 * xr * xr; dl = sig2 * xr; }
        else { l = ax - 0.5f * inv; dl = sgn; }
        const float rl = l * wn / norm_reg * a.p.reg_loss_weight;
        a.reg_loss[k] = rl;
        sum_reg += (double)rl;
        dd[c] = gs * wn / norm_reg * dl;
      }
      if (a.d_delta) {
        float* o = a.d_delta + b * a.delta_bs + i * 8;
        *(float4*)o = make_float4(dd[0], dd[1], dd[2], dd[3]);
        *(float4*)(o + 4) = make_float4(dd[4], dd[5], dd[6], dd[7]);
      }
    }
  }
  sum_cls = loss_block_sum(sum_cls, red);
  sum_reg = loss_block_sum(sum_reg, red + 4);
  if (threadIdx.x == 0) {
    const long slot = (long)blockIdx.y * gridDim.x + blockIdx.x;
    a.part_cls[slot] = sum_cls;
    a.part_reg[slot] = sum_reg;
  }
}
}  // namespace rd
