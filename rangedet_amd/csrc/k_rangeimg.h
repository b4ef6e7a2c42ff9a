// Range image from a raw spinning-LiDAR point cloud: the build's counterpart of get_range_image
// (datasets/create_range_image_in_kitti.py:107-137, mask :178 in the reference), which loops over the beams in NumPy, argsorts the
// points by range and scatters them with a fancy index.  Restated per point, operation by operation, FP contraction off:
//   row     first arg-min over the beams i of |incl[i] - atan2(height[i] - z, xy_norm)| in double; xy_norm = sqrtf(x*x + y*y) is float
//   column  float throughout: azi = atan2f(y, x) (the C library's: fdlibm_atan2f), c = (W - 0.5) - (azi + pi) / (2 pi) * W with pi and
//           2 pi rounded to float, rounded half to even, then == W -> W - 1 and < 0 -> 0
//   range   sqrtf((x*x + y*y) + z*z)
//   scatter the reference writes the points in order of decreasing range, so the NEAREST point of a cell stays.  Its argsort is not
//           stable: which of two points of one cell with the same range stays is unpinned there.  HERE THE HIGHER INDEX WINS, which is
//           what a stable argsort gives.  A point with a non-finite x, y or z (outside the reference's contract) is skipped.
// Two launches over a caller-owned key buffer (B*H*W 64-bit words, set to all-ones on the stream in every call):
//   project  one lane per point: row, column, range, then ONE 64-bit atomicMin of (float bits of range << 32) | ~index into the cell's
//            key.  Ranges are >= +0, so bit order is value order; the inverted index makes the higher index the smaller key.  An integer
//            minimum does not depend on arrival order: the result is deterministic.
//   resolve  one lane per cell: key -> winning point (one 16-byte load) -> [range, x, y, z, intensity] or five -1, staged in LDS so that
//            a workgroup's 256 cells leave as 16-byte stores; mask (0/1) and the point's index within its scan (-1 = empty).
// Row search: the plain form, H double atan2 per point (7.7 M for a 120 000-point scan at H = 64); DESIGN.md has the measured time.
#pragma once
#include <cmath>

#include "rd_common.h"

namespace rd {
constexpr int RI_MAX_BEAMS = 128;
constexpr int RI_MAX_WIDTH = 1 << 22;        // W - 0.5 is a float, H*W an int
constexpr int RI_SCANS_PER_LAUNCH = 64;   // scans whose offsets travel in one launch's arguments
constexpr unsigned long long RI_EMPTY = ~0ull;

struct RangeImgArgs {
  const float* points;                      // (sum N_b, 4)
  unsigned long long* key;                  // (B,H,W)
  long long off[RI_SCANS_PER_LAUNCH + 1];   // first point of scans b0 .. b0 + gridDim.y
  double incl[RI_MAX_BEAMS], height[RI_MAX_BEAMS];
  float* range_image;                       // (B,H,W,5)
  unsigned char* mask;                      // (B,H,W)
  int* point_index;                         // (B,H,W) or null
  int b0, H, W;
};

__global__ __launch_bounds__(256) void range_image_project_kernel(RangeImgArgs a) {
  _Pragma("clang fp contract(off)")
  const long long n = a.off[blockIdx.y + 1] - a.off[blockIdx.y];
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= n) return;
  const f32x4 p = *(const f32x4*)(a.points + (size_t)(a.off[blockIdx.y] + i) * 4);
  const float x = p[0], y = p[1], z = p[2];
  const unsigned expo = 0x7f800000u;
  if ((__builtin_bit_cast(unsigned, x) & expo) == expo || (__builtin_bit_cast(unsigned, y) & expo) == expo ||
      (__builtin_bit_cast(unsigned, z) & expo) == expo)
    return;
  const float xx = x * x, yy = y * y, zz = z * z;
  const float sxy = xx + yy;
  const double xy_norm = (double)sqrtf(sxy), zd = (double)z;
  int row = 0;
  double best = 0.0;
  for (int r = 0; r < a.H; ++r) {                                           // :112-118, the first minimum wins
    const double e = fabs(a.incl[r] - atan2(a.height[r] - zd, xy_norm));
    if (r == 0 || e < best) { best = e; row = r; }
  }
  const float fw = (float)a.W, pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  const float azi = fdlibm_atan2f(y, x);
  const float c = rintf(((float)((double)a.W - 1.0 + 0.5)) - (azi + pi) / two_pi * fw);   // :122-123
  const int col = c >= fw ? a.W - 1 : c < 0.f ? 0 : (int)c;                 // :124-125 (never outside 0 .. W-1, whatever the point)
  const float range = sqrtf(sxy + zz);                                      // :127, >= +0 (Inf for a huge point: still ordered)
  const unsigned long long k = ((unsigned long long)__builtin_bit_cast(unsigned, range) << 32) | (unsigned)~(unsigned)i;
  atomicMin(a.key + ((size_t)(a.b0 + blockIdx.y) * a.H + row) * a.W + col, k);
}

// One workgroup owns 256 cells of one scan = 1280 consecutive floats of range_image, which start at a multiple of 4 floats only when
// (b*H*W + c0) * 5 does: the slab is staged at the same offset within a 16-byte group (shift), every whole group leaves as one 16-byte
// store and the ragged ends as single floats.
__global__ __launch_bounds__(256) void range_image_resolve_kernel(RangeImgArgs a) {
  __shared__ __attribute__((aligned(16))) float slab[256 * 5 + 4];
  const long long hw = (long long)a.H * a.W, c0 = blockIdx.x * 256LL, c = c0 + threadIdx.x;
  const size_t cell0 = (size_t)(a.b0 + blockIdx.y) * hw + c0;                // first cell of this workgroup in (B,H,W)
  const int shift = (int)((cell0 * 5) & 3);
  if (c < hw) {
    const unsigned long long k = a.key[cell0 + threadIdx.x];
    f32x4 p = {-1.f, -1.f, -1.f, -1.f};
    float range = -1.f;
    int idx = -1;
    if (k != RI_EMPTY) {
      idx = (int)~(unsigned)k;
      range = __builtin_bit_cast(float, (unsigned)(k >> 32));
      p = *(const f32x4*)(a.points + (size_t)(a.off[blockIdx.y] + idx) * 4);
    }
    float* s = slab + shift + threadIdx.x * 5;
    s[0] = range; s[1] = p[0]; s[2] = p[1]; s[3] = p[2]; s[4] = p[3];
    a.mask[cell0 + threadIdx.x] = k != RI_EMPTY;
    if (a.point_index) a.point_index[cell0 + threadIdx.x] = idx;
  }
  __syncthreads();
  const long long left = hw - c0;
  const int end = shift + (int)(left < 256 ? left : 256) * 5;               // the slab holds floats [shift, end)
  float* out = a.range_image + cell0 * 5 - shift;                            // 16-byte aligned (range_image is)
  for (int j = threadIdx.x * 4; j < end; j += 1024) {
    if (j >= shift && j + 4 <= end) *(f32x4*)(out + j) = *(const f32x4*)(slab + j);
    else for (int t = j < shift ? shift : j; t < j + 4 && t < end; ++t) out[t] = slab[t];
  }
}

}  // namespace rd
