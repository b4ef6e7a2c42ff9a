// Training-time input chain of the reference on the device: the sixteen transforms of the training config
// (config/rangedet/rangedet_veh_wo_aug_4_18e.py:346-366) for a whole batch, raw record arrays + ground truth in, every
// named tensor of data_name + label_name out.
//   LoadRecord .. CombineData            rangedet/core/input.py:14-42,89-229   as k_input.h (shared per-pixel functions)
//   Bbox3dAssigner                       input.py:276-320, operator_cxx/src_cxx/assigner.h:11-85   as k_assign.h (shared box test)
//   GenerateTarget                       input.py:323-519, assigner.h:87-109 (points per box)
//   PadData / TransposeData / GenerateFPNTarget / TransAndReshape     input.py:522-624 (training name lists, config:72-81,336)
// Two launches, blockIdx.y = frame: the number of points of a box has to be complete before a pixel divides by it.
//   pass 1  one thread per unpadded pixel: post-fill point + mask -> box index (bbox3d_ind), LDS histogram per block flushed
//           with integer atomics into counts (B,500) (order-independent: the result is deterministic)
//   pass 2  one thread per padded pixel: everything rd_input_transform writes, plus per level the regression target, its
//           two weights and the class target, each times the level's range-interval mask, sampled at columns s//2::s
// HBM-bound like k_input.h: 28 B/px in, ~100 B/px (input side) + 4 B/px (index) + ~25 floats x 1.75 levels per px out.
#pragma once
#include "k_assign.h"
#include "k_input.h"

namespace rd {
constexpr int TRAIN_FRAMES_PER_LAUNCH = 64;   // frames whose box counts travel in one launch's arguments

struct TrainArgs {
  const float* ri;         // (B,H,W,4)
  const float* pc;         // (B,H,W,3)
  const float* incl;       // (B,H)
  const float* gt_imu;     // (B,Mmax,24)
  const float* gt_center;  // (B,Mmax,3)
  const float* gt_limits;  // (B,6) max_x min_x max_y min_y max_z min_z
  const float* gt_csa;     // (B,Mmax,7) x y z l w h yaw
  int* ind;                // (B,H,W)
  int* counts;             // (B,POINT_NUM_MAX_BOXES)
  rd_train_outputs_t o;
  int num_gt[TRAIN_FRAMES_PER_LAUNCH];   // of frames b0 .. b0 + gridDim.y - 1
  int b0, Mmax;
  float radius, max_dist;
  float reg_weight[8];
  int H, W, Hp, Wp;
  rd_input_norm_t n;
};

__global__ __launch_bounds__(256) void train_assign_kernel(TrainArgs a) {
  HIP_DYNAMIC_SHARED(float, bx);
  __shared__ int hist[POINT_NUM_MAX_BOXES];
  const int b = a.b0 + blockIdx.y, M = a.num_gt[blockIdx.y];
  const float* box = a.gt_imu + (size_t)b * a.Mmax * 24;
  const float* ctr = a.gt_center + (size_t)b * a.Mmax * 3;
  for (int j = threadIdx.x; j < M; j += 256) {
    assign_stage_box(bx + j * ASSIGN_BOX_F, box + (size_t)j * 24, ctr + j * 3, a.radius);
    hist[j] = 0;
  }
  __syncthreads();
  const long npt = (long)a.H * a.W;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i < npt) {
    const int h = (int)(i / a.W), w = (int)(i - (long)h * a.W);
    float f[3], px, py, pz, rmask;
    in_source(a.ri + (size_t)b * npt * 4, a.pc + (size_t)b * npt * 3, a.W, h, w, f, px, py, pz, rmask);
    const float* lim = a.gt_limits + (size_t)b * 6;
    const AssignLimits l = {lim[0], lim[1], lim[2], lim[3], lim[4], lim[5], a.max_dist};
    const int res = assign_find_box(bx, M, px, py, pz, !(rmask < 0.5f), l);        // (no no-label zones: input.py:294)
    a.ind[(size_t)b * npt + i] = res;
    if (res >= 0) atomicAdd(&hist[res], 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < M; j += 256)
    if (hist[j]) atomicAdd(&a.counts[(size_t)b * POINT_NUM_MAX_BOXES + j], hist[j]);
}

// LDS per box: x y z  log w  log l  yaw  z - h/2  log h   (input.py:490-494: what a target needs of its box besides the point)
__global__ __launch_bounds__(256) void train_write_kernel(TrainArgs a) {
  RD_NOCONTRACT_A
  __shared__ float rows[POINT_NUM_MAX_BOXES * 8];
  const int b = a.b0 + blockIdx.y, M = a.num_gt[blockIdx.y];
  for (int j = threadIdx.x; j < M; j += 256) {
    const float* c = a.gt_csa + ((size_t)b * a.Mmax + j) * 7;
    float* r = rows + j * 8;
    r[0] = c[0]; r[1] = c[1]; r[2] = c[2];
    r[3] = logf(c[4]); r[4] = logf(c[3]);
    r[5] = c[6];
    r[6] = c[2] - c[5] / 2;
    r[7] = logf(c[5]);
  }
  __syncthreads();
  const long npx = (long)a.Hp * a.Wp;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= npx) return;
  const int h = (int)(i / a.Wp), w = (int)(i - (long)h * a.Wp);
  const long npt = (long)a.H * a.W;
  float f[3];
  float rmask = 0.f, unnorm = 0.f, az = 0.f;
  float d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float px = 0.f, py = 0.f, pz = 0.f;
  float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // regression target; zeros without a box and in the padding
  float nw = 0.f;                          // 1 / points of the pixel's box
  bool inbox = false;
  if (h < a.H && w < a.W) {
    const float* ri = a.ri + (size_t)b * npt * 4;
    if (in_source(ri, a.pc + (size_t)b * npt * 3, a.W, h, w, f, px, py, pz, rmask)) {
      f[0] = in_missing_range(ri, a.H, a.W, h, w); f[1] = 0.f; f[2] = 0.f;
    }
    in_channels(f, px, py, pz, a.incl[(size_t)b * a.H + h], a.n, d, unnorm, az);
    const int k = a.ind[(size_t)b * npt + (long)h * a.W + w];
    if (k >= 0) {                                                         // input.py:469-503, float32 throughout
      inbox = true;
      const float* r = rows + k * 8;
      const float ca = cosf(az), sa = sinf(az);
      const float dx = r[0] - px, dy = r[1] - py;
      const float rx = ca * dx + sa * dy, ry = -sa * dx + ca * dy;        // rotation into the point's azimuth frame (:509-519)
      t[0] = (rx > 0.f ? 1.f : rx < 0.f ? -1.f : 0.f) * sqrtf(fabsf(rx));
      t[1] = (ry > 0.f ? 1.f : ry < 0.f ? -1.f : 0.f) * sqrtf(fabsf(ry));
      t[2] = r[3]; t[3] = r[4];
      const float dyaw = r[5] - az;
      t[4] = cosf(dyaw); t[5] = sinf(dyaw);
      t[6] = r[6]; t[7] = r[7];
      nw = 1.f / (float)a.counts[(size_t)b * POINT_NUM_MAX_BOXES + k];    // IEEE divide (input.py:436)
    }
  }
  const rd_train_outputs_t& o = a.o;
  float* dp = o.input_data + (size_t)b * 8 * npx + i;
#pragma unroll
  for (int c = 0; c < 8; ++c) dp[(size_t)c * npx] = d[c];
  float* cp = o.coord_s1 + (size_t)b * 3 * npx + i;
  cp[0] = d[3]; cp[npx] = d[4]; cp[2 * npx] = d[5];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int s = 1 << l;
    if ((w & (s - 1)) != (s >> 1)) continue;                              // sampled columns s//2, s//2 + s, ...
    const long j = (long)h * (a.Wp / s) + (w >> l);
    const long ns = npx / s;
    const bool m = a.n.interval_lo[l] <= unnorm && unnorm < a.n.interval_hi[l];   // input.py:582-597
    o.mask[l][(size_t)b * ns + j] = rmask;                                // not range-masked in training (config:78-81)
    float* q = o.pc[l] + ((size_t)b * ns + j) * 3;
    q[0] = px; q[1] = py; q[2] = pz;
    o.cls_target[l][(size_t)b * ns + j] = inbox && m ? 1.f : 0.f;
    const size_t at = (size_t)b * 8 * ns + j;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      o.reg_target[l][at + (size_t)c * ns] = m ? t[c] : 0.f;
      o.reg_weight[l][at + (size_t)c * ns] = inbox && m ? a.reg_weight[c] : 0.f;
      o.reg_normalize_weight[l][at + (size_t)c * ns] = m ? nw : 0.f;
    }
  }
}

}  // namespace rd
