// Shared host/device helpers for librangedet_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include <atomic>
#include "../../include/rangedet_hip.h"

namespace rd {

// ---- error channel ---------------------------------------------------------------------------------
inline char* err_buf() {
  static thread_local char buf[512] = "";
  return buf;
}
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}
#define RD_REQUIRE(cond, code, ...) \
  do {                              \
    if (!(cond)) return rd::fail(code, __VA_ARGS__); \
  } while (0)

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RD_EHIP, "%s: %s", what, hipGetErrorString(e));
  return RD_OK;
}

// A kernel that takes more than 64 KB of dynamic LDS must say so once.  (A kernel with static LDS cannot take the full 160 KB as
// dynamic: the attribute call then fails while the launch with the size actually requested still works -- do not leave that
// status behind for the next check_launch.)
template <class K>
inline void allow_big_lds(K kernel) {
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    (void)hipGetLastError();
}
// The attribute is a property of the function ON A DEVICE: "once" means once per (kernel, device), so that a process which
// launches on a second GPU raises the limit there too (one process per GPU never sees more than one bit set).
// once_per_device(seen, f): runs f() unless this device's bit is already set, and sets the bit only AFTER f() has returned -- two host
// threads may both run f (the attribute call is idempotent), but none can see the bit and launch before some thread's call is
// complete.  Devices >= 64 and a failing hipGetDevice are never cached (f runs every time).
template <class F>
inline void once_per_device(std::atomic<unsigned long long>& seen, F f) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); f(); return; }
  if (dev < 0 || dev >= 64) { f(); return; }
  const unsigned long long bit = 1ull << dev;
  if (seen.load(std::memory_order_acquire) & bit) return;
  f();
  seen.fetch_or(bit, std::memory_order_release);
}

// Compute units of the current device: the grid of every persistent kernel (convs, fused block, Meta-Kernel) is a multiple of it.
// -DRD_BUILD_NUM_CUS=n fixes it at build time (k_conv3.h, build options).
inline int conv_num_cus() {
#ifdef RD_BUILD_NUM_CUS
  return RD_BUILD_NUM_CUS;
#else
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
  return v;
#endif
}

// ---- per-kind event profiling ------------------------------------------------------------------------
struct Prof {
  bool on = false;
  std::mutex mu;
  struct Span { hipEvent_t a, b; int kind; };
  std::vector<Span> spans;
  std::vector<hipEvent_t> pool;
  double total[RD_PROF_NKINDS] = {0};
  long count[RD_PROF_NKINDS] = {0};
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
  }
  void drain() {
    for (auto& s : spans) {
      hipEventSynchronize(s.b);
      float ms = 0;
      hipEventElapsedTime(&ms, s.a, s.b);
      total[s.kind] += ms;
      count[s.kind] += 1;
      pool.push_back(s.a);
      pool.push_back(s.b);
    }
    spans.clear();
  }
};
inline Prof& prof() {
  static Prof p;
  return p;
}
struct ProfScope {
  hipEvent_t a = nullptr;
  int kind;
  hipStream_t st;
  ProfScope(int k, hipStream_t s) : kind(k), st(s) {
    Prof& p = prof();
    if (!p.on) return;
    std::lock_guard<std::mutex> g(p.mu);
    a = p.get();
    hipEventRecord(a, st);
  }
  ~ProfScope() {
    if (!a) return;
    Prof& p = prof();
    std::lock_guard<std::mutex> g(p.mu);
    hipEvent_t b = p.get();
    hipEventRecord(b, st);
    p.spans.push_back({a, b, kind});
  }
};

// ---- element types -----------------------------------------------------------------------------------
typedef unsigned short bf16_t;  // raw bfloat16 bits
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ __forceinline__ bf16_t f32_to_bf16(float f) {  // round to nearest even
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(unsigned short, (__bf16)f);  // v_cvt_pk_bf16_f32 on gfx950
#endif
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_t)(u >> 16);
}
// two floats -> one dword of packed bf16 (lo = a, hi = b): a single v_cvt_pk_bf16_f32 on gfx950
__host__ __device__ __forceinline__ unsigned f32x2_to_bf16x2(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
#else
  return (unsigned)f32_to_bf16(a) | ((unsigned)f32_to_bf16(b) << 16);
#endif
}
__host__ __device__ __forceinline__ float bf16_to_f32(bf16_t h) {
  unsigned u = (unsigned)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// ---- fp16 (round 3: the reference's own arithmetic type, config fp16 = True) -------------------------------------------
typedef unsigned short f16_t;   // raw IEEE binary16 bits
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
__host__ __device__ __forceinline__ f16_t f32_to_f16(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }  // RNE
__host__ __device__ __forceinline__ float f16_to_f32(f16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__host__ __device__ __forceinline__ unsigned f32x2_to_f16x2(float a, float b) {   // one v_cvt_pk_f16_f32 on gfx950
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
#else
  return (unsigned)f32_to_f16(a) | ((unsigned)f32_to_f16(b) << 16);
#endif
}

// The two 16-bit activation / weight types share every layout (2 bytes, 8 channels per 16-byte slot, the same packed MFMA
// fragment orders); a kernel templated on DT differs only in these conversions and in the MFMA instruction.
typedef float f32x2_t_ __attribute__((ext_vector_type(2)));
template <int DT> struct H16;
template <> struct H16<RD_BF16> {
  static constexpr unsigned short ONE = 0x3F80;
  __host__ __device__ static __forceinline__ unsigned short from_f32(float v) { return f32_to_bf16(v); }
  __host__ __device__ static __forceinline__ float to_f32(unsigned short h) { return bf16_to_f32(h); }
  __host__ __device__ static __forceinline__ unsigned pk(float a, float b) { return f32x2_to_bf16x2(a, b); }
  __host__ __device__ static __forceinline__ f32x2_t_ unpk(unsigned u) {   // bf16 -> f32 is a 16-bit shift of the packed pair
    unsigned lo = u << 16, hi = u & 0xffff0000u;
    return f32x2_t_{__builtin_bit_cast(float, lo), __builtin_bit_cast(float, hi)};
  }
  __device__ static __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
  // 16 x 16 x 32: A[m][k] lane m + 16*(k/8) element k%8, B[k][n] lane n + 16*(k/8) element k%8, D[m][n] lane n + 16*(m/4) register m%4
  // (tools/micro/mfma16_probe.hip checks the map on the GPU; k_conv3.h M16 says why this shape)
  __device__ static __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct H16<RD_F16> {
  static constexpr unsigned short ONE = 0x3C00;
  __host__ __device__ static __forceinline__ unsigned short from_f32(float v) { return f32_to_f16(v); }
  __host__ __device__ static __forceinline__ float to_f32(unsigned short h) { return f16_to_f32(h); }
  __host__ __device__ static __forceinline__ unsigned pk(float a, float b) { return f32x2_to_f16x2(a, b); }
  __host__ __device__ static __forceinline__ f32x2_t_ unpk(unsigned u) {
    return f32x2_t_{f16_to_f32((unsigned short)(u & 0xffffu)), f16_to_f32((unsigned short)(u >> 16))};
  }
  __device__ static __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
};
inline bool is_h16(int dt) { return dt == RD_BF16 || dt == RD_F16; }
// Launch a kernel templated on the 16-bit type for a run-time dtype (checked with is_h16 before).  KERNEL names its instance with `DT`
// for the type, in parentheses: RD_LAUNCH_H16(dtype, (some_kernel<DT, 128>), grid, block, stream, args...).
#define RD_LAUNCH_H16(dtype, KERNEL, grid, block, stream, ...)                 \
  do {                                                                         \
    if ((dtype) == RD_F16) {                                                   \
      constexpr int DT = RD_F16;                                               \
      hipLaunchKernelGGL(KERNEL, grid, block, 0, stream, __VA_ARGS__);         \
    } else {                                                                   \
      constexpr int DT = RD_BF16;                                              \
      hipLaunchKernelGGL(KERNEL, grid, block, 0, stream, __VA_ARGS__);         \
    }                                                                          \
  } while (0)
inline unsigned short h16_from_f32(int dt, float v) { return dt == RD_F16 ? f32_to_f16(v) : f32_to_bf16(v); }
inline float h16_to_f32(int dt, unsigned short h) { return dt == RD_F16 ? f16_to_f32(h) : bf16_to_f32(h); }

template <int DT> struct Elem;
template <> struct Elem<RD_F32> {
  typedef float T;
  static constexpr int CH = 4;  // channels per 16-byte slot
  __host__ __device__ static float from_f32(float v) { return v; }
  __host__ __device__ static float to_f32(float v) { return v; }
};
template <> struct Elem<RD_BF16> {
  typedef bf16_t T;
  static constexpr int CH = 8;
  __host__ __device__ static bf16_t from_f32(float v) { return f32_to_bf16(v); }
  __host__ __device__ static float to_f32(bf16_t v) { return bf16_to_f32(v); }
};
template <> struct Elem<RD_F16> {
  typedef f16_t T;
  static constexpr int CH = 8;
  __host__ __device__ static f16_t from_f32(float v) { return f32_to_f16(v); }
  __host__ __device__ static float to_f32(f16_t v) { return f16_to_f32(v); }
};
inline int elem_size(int dt) { return dt == RD_F32 ? 4 : 2; }
inline int ch_per_slot(int dt) { return dt == RD_F32 ? 4 : 8; }
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

typedef unsigned Slot16 __attribute__((ext_vector_type(4)));  // one 16-byte LDS/global granule (register-resident)

// one slot of a 16-bit tensor <-> its eight channels in float32
template <int DT>
__device__ __forceinline__ void slot_unpack(const Slot16 v, float (&f)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x2_t_ t = H16<DT>::unpk(v[k]);
    f[2 * k] = t[0];
    f[2 * k + 1] = t[1];
  }
}
template <int DT>
__device__ __forceinline__ Slot16 slot_pack(const float (&f)[8]) {
  Slot16 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = H16<DT>::pk(f[2 * k], f[2 * k + 1]);
  return o;
}
// red[PL][C] in LDS, one row per pixel lane: the PL lane values of channel `tid` (tid < C) added in lane order
__device__ __forceinline__ float lane_sum(const float* red, int PL, int C, int tid) {
  _Pragma("clang fp contract(off)")
  float s = red[tid];
  for (int q = 1; q < PL; ++q) s += red[q * C + tid];
  return s;
}

// LDS-DMA of 16 bytes per lane: LDS[lds_dst_uniform + lane*16] <- *gsrc (per lane).  Issued through inline asm on the
// device so that hipcc's waitcnt pass does not see it: seen through the builtin, every later ds_read is preceded by
// s_waitcnt vmcnt(0) (the compiler cannot tell ring slots apart), which drains the prefetch ring each step.  The
// caller owns the ordering: counted s_waitcnt vmcnt(N) + workgroup barrier before any ds_read of the destination.
__device__ __forceinline__ void lds_dma16(const void* gsrc, void* lds_dst_uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned lds_addr = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)lds_dst_uniform);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
#else
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_dst_uniform, 16, 0, 0);
#endif
}

// ---- atan2f as the reference's host computes it ------------------------------------------------------------------------------------
// The weighted NMS takes the polar angle of every box edge with atan2 on float arguments (operator_cxx/src_cxx/nms.h:71), i.e. the
// C library's atan2f, and compares angles with a tolerance of 1e-5 (nms.h:58-64), so an ulp decides which half-plane survives a tie.
// glibc 2.35 (the image's, and what the compiled reference under oracle/_ref links) ships the fdlibm float routines
// (sysdeps/ieee754/flt-32/e_atan2f.c, s_atanf.c: argument reduction at 7/16, 11/16, 19/16, 39/16, an 11-term odd / even polynomial,
// hi + lo table values) -- NOT a correctly rounded function: it differs from float(atan2(double)) on 15 % of box-edge inputs
// (1e9 inputs, profiles/r05_atan2f_study.txt), so an fp64 evaluation rounded once would not reproduce it.  This is that published
// algorithm restated operation by operation in float arithmetic without contraction; the same text compiled for the host is
// bit-equal to glibc's atan2f on 2e9 inputs (box edges, random bit patterns incl. NaN / Inf / denormals, the reduction thresholds).
// A reference built against another C library may differ from it in the last bit.
__host__ __device__ inline float fdlibm_atanf(float x) {
  _Pragma("clang fp contract(off)")
  const float hi_[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
  const float lo_[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
  const float t0 = 3.3333334327e-01f, t1 = -2.0000000298e-01f, t2 = 1.4285714924e-01f, t3 = -1.1111110449e-01f, t4 = 9.0908870101e-02f,
              t5 = -7.6918758452e-02f, t6 = 6.6610731184e-02f, t7 = -5.8335702866e-02f, t8 = 4.9768779427e-02f, t9 = -3.6531571299e-02f,
              t10 = 1.6285819933e-02f;
  const int hx = __builtin_bit_cast(int, x), ix = hx & 0x7fffffff;
  int id;
  if (ix >= 0x4c000000) {                      // |x| >= 2^25
    if (ix > 0x7f800000) return x + x;         // NaN
    return hx > 0 ? hi_[3] + lo_[3] : -hi_[3] - lo_[3];
  }
  if (ix < 0x3ee00000) {                       // |x| < 7/16
    if (ix < 0x31000000) return x;             // |x| < 2^-29
    id = -1;
  } else {
    x = __builtin_fabsf(x);
    if (ix < 0x3f980000) {                     // |x| < 19/16
      if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
      else { id = 1; x = (x - 1.0f) / (x + 1.0f); }
    } else {
      if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
      else { id = 3; x = -1.0f / x; }
    }
  }
  const float z = x * x, w = z * z;
  const float s1 = z * (t0 + w * (t2 + w * (t4 + w * (t6 + w * (t8 + w * t10)))));
  const float s2 = w * (t1 + w * (t3 + w * (t5 + w * (t7 + w * t9))));
  if (id < 0) return x - x * (s1 + s2);
  const float r = hi_[id] - ((x * (s1 + s2) - lo_[id]) - x);
  return hx < 0 ? -r : r;
}
__host__ __device__ inline float fdlibm_atan2f(float y, float x) {
  _Pragma("clang fp contract(off)")
  const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
  const int hx = __builtin_bit_cast(int, x), ix = hx & 0x7fffffff;
  const int hy = __builtin_bit_cast(int, y), iy = hy & 0x7fffffff;
  if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;           // NaN
  if (hx == 0x3f800000) return fdlibm_atanf(y);                   // x == 1
  const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);              // 2 * sign(x) + sign(y)
  if (iy == 0) return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
  if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (ix == 0x7f800000) {
    if (iy == 0x7f800000) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny;
    return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? pi + tiny : -pi - tiny;
  }
  if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int k = (iy - ix) >> 23;
  float z;
  if (k > 60) z = pi_o_2 + 0.5f * pi_lo;                          // |y / x| > 2^60
  else if (hx < 0 && k < -60) z = 0.0f;                           // |y| / x < -2^60
  else z = fdlibm_atanf(__builtin_fabsf(y / x));
  switch (m) {
    case 0: return z;
    case 1: return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, z) ^ 0x80000000u);
    case 2: return pi - (z - pi_lo);
    default: return (z - pi_lo) - pi;
  }
}

}  // namespace rd
