// The parameter update of the head towers: multi-tensor SGD with momentum on float32 master weights, and the re-pack of the 16-bit conv
// weight images the persistent 3x3 conv reads, both on the device.  The reference creates `sgd` with momentum, wd, rescale_grad,
// clip_gradient and, under fp16, multi_precision (tools/train.py:306-365; config/rangedet/*.py OptimizeParam.optimizer: momentum = 0.9,
// wd = 0.00001, clip_gradient = 35, e.g. rangedet_veh_wo_aug_4_18e.py:179-184).  The per-element arithmetic is that of MXNet's
// mp_sgd_mom_update operator AS DOCUMENTED -- MXNet is not available to this project: not pinned by a run of the reference.
//
//   g   = rescale_grad * grad
//   g   = clip >= 0 ? (g > clip ? clip : (g < -clip ? -clip : g)) : g        a NaN fails both comparisons and passes through
//   mom = momentum * mom - (lr_t * wd_t) * w - lr_t * g                      evaluated left to right
//   w   = w + mom
// with lr_t = lr * lr_mult[t], wd_t = wd * wd_mult[t].  Every operation above is ONE float32 rounding in exactly that order; contraction is
// off in this file, there is no fused multiply-add.  lr_t, wd_t and lr_t * wd_t are float32 products of the step's by-value scalars with
// the table's multipliers; the kernel forms them once per workgroup (a workgroup never spans two tensors), which gives the bits a host
// would form -- so a new learning rate costs no upload.  NaN and inf in a gradient propagate (inf is clipped like any large value when
// clip >= 0).
//
// ---- the table ---------------------------------------------------------------------------------------------------------------------------
// Built on the host (sgd_table_build), uploaded once by the caller, read by every workgroup:
//   SgdHeader | SgdEntry[nt] | SgdChunk[n_chunks] | SgdPackChunk[n_pack]
// SgdChunk k = (tensor, chunk of SGD_CHUNK elements within it): sgd_mom_kernel runs one workgroup per chunk, 256 threads x one 16-byte
// vector of w, grad and mom each; the n % 4 last elements of a tensor are done one per thread by threads 0 .. 2 of its last chunk.
// SgdPackChunk k = (tensor, image, run of SGD_PACK_SLOTS 16-byte slots of that image): sgd_pack_kernel, the second and last launch of a
// step, one slot per thread.
//
// ---- the images ----------------------------------------------------------------------------------------------------------------------------
// A (cout, cin, 3, 3) weight with cin, cout in {64, 128} has up to two images in the layout of pack_taps_frag (k_conv3.h):
// [32-ch chunk c][tap t][ks][cb][lane][8], slot s = ((c * 9 + t) * 2 + ks) * ncb * 64 + cb * 64 + lane holding, for j = 0 .. 7,
//   row r = 32 cb + conv_row_perm(lane & 31), column q = 32 c + 16 ks + 8 (lane >> 5) + j
//   forward image        (ncb = cout / 32):  round16(fold_scale[r] * W[r][q][t])     (fold_scale NULL: 1.0f -- the product is still formed)
//   data-gradient image  (ncb = cin / 32):   round16(W[q][r][8 - t])                  channel axes swapped, taps flipped, no scale
// followed by RD_CONV_TAIL zero bytes, which the launch writes too.  No padding channels exist at these sizes, so every weight element
// lands at exactly one position of each image; a thread gathers its eight values (the weight was written by the launch before, it is in
// L2) and stores one 16-byte slot.  Rounding is round-to-nearest-even, what h16_from_f32 does on the host.
// A (cout, cin, 1, 1) weight of the same channel counts (the projection shortcut of a backbone BasicBlock) has the same two images with
// ONE tap instead of nine -- what rd_pack_conv_weight_host(w, cout, cin, 1, 1, dtype) writes for the weight and for its transpose: the
// table is unchanged, the tap count of an entry is n / (cout cin), 9 or 1.
// A (C, C, 3, 3) weight with stride_w == 2 (conv2 of a down-sampling BasicBlock, C = 64 or 128) has the images of the strided launches:
//   forward          what rd_pack_conv3x3_ex_host(w, fold, C, C, 2, C) writes: the pixel-pair view (2 C view channels) in the body form
//                    conv3_body_s2 selects -- per four 32-channel chunks the units [odd: 6 steps | even: 3 | even: 3 | odd: 6], one slab
//                    [ks][cb][lane][8] per step in program order (pack_body_frag, BODY 1): 18 C^2 bytes of weights, then zeros up to the
//                    24 C^2 + RD_CONV_TAIL bytes rd_conv3x3_ex_packed_bytes(C, C, 2, C) reports.  That packer chooses the body form only
//                    when it is given a fold scale (the form a RD_SCALE_FOLDED launch reads); without one it writes the six-tap form
//                    pack_taps_frag(6, 2 C, C), and so does the step -- pass a vector of ones to train an unscaled strided conv
//   data gradient    the two phase images of the transposed conv (3,4) / stride 2 / pad 1 whose weight is w read as (Cin, Cout, KH, KW)
//                    with a zero column kx = 3: pack_taps_frag(6, C, C) each with its own zero tail, phase 1 right after phase 0.  Phase 0
//                    holds, per tap row, [zero | kx 1], phase 1 [kx 2 | kx 0]; tap rows in the order ky = 2, 1, 0.
// The table's layout does not change: SgdPackChunk.image is 2 for the strided forward image and 3 / 4 for the two phases.
#pragma once
#include "k_conv.h"

namespace rd {
constexpr int SGD_CHUNK = 1024;        // elements of one workgroup: 256 threads x 4
constexpr int SGD_PACK_SLOTS = 256;    // 16-byte image slots of one workgroup: one per thread
constexpr unsigned SGD_MAGIC = 0x52445347u;

struct SgdHeader {
  unsigned magic;
  int nt, n_chunks, n_pack, dtype;
  unsigned off_entries, off_chunks, off_pack, bytes;
  unsigned pad[7];
};
struct SgdEntry {
  float* w;
  const float* g;
  float* m;
  long n;
  float lr_mult, wd_mult;
  int cout, cin;
  unsigned short *fwd, *bwd;
  const float* fold;
};
struct SgdChunk { int tensor, chunk; };
struct SgdPackChunk { int tensor, image, run, pad; };   // image 0: forward, 1: data gradient; stride 2: 2 forward, 3 / 4 phase 0 / 1
static_assert(sizeof(SgdHeader) == 64 && sizeof(SgdEntry) % 8 == 0, "table layout");

inline long sgd_image_slots(int cout, int cin, int ntaps = 9) { return (long)(ntaps * cout * cin * 2 + RD_CONV_TAIL) / 16; }
// taps of an entry that names images: 9 (n = 9 cout cin), 1 (n = cout cin), else 0
__host__ __device__ inline int sgd_ntaps(long n, int cout, int cin) { return n == 9L * cout * cin ? 9 : n == (long)cout * cin ? 1 : 0; }
inline bool sgd_pack_shape_ok(int cout, int cin) { return (cout == 64 || cout == 128) && (cin == 64 || cin == 128); }
// stride 2 (C -> C): slots of the forward image and of ONE phase image, zero fill and zero tails included
__host__ __device__ inline long sgd_s2_fwd_slots(int C) { return (long)(24 * C * C + (int)RD_CONV_TAIL) / 16; }
__host__ __device__ inline long sgd_s2_phase_slots(int C) { return (long)(12 * C * C + (int)RD_CONV_TAIL) / 16; }
inline bool sgd_is_s2(const rd_sgd_tensor_t& t) { return t.stride_w == 2 && (t.pack_fwd || t.pack_bwd); }
inline long sgd_runs(long slots) { return (slots + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS; }

// the checks of one tensor; -> RD_OK or the code, the message left in the error buffer
inline int sgd_check_tensor(const rd_sgd_tensor_t& t, int i) {
  RD_REQUIRE(t.weight && t.grad && t.mom, RD_EINVAL, "sgd_table: tensor %d: null pointer", i);
  RD_REQUIRE(t.n > 0 && t.n <= 0x7fffffffL, RD_EINVAL, "sgd_table: tensor %d: n %ld (at least 1)", i, t.n);
  RD_REQUIRE(((uintptr_t)t.weight | (uintptr_t)t.grad | (uintptr_t)t.mom | (uintptr_t)t.pack_fwd | (uintptr_t)t.pack_bwd) % 16 == 0 &&
             (uintptr_t)t.fold_scale % 4 == 0, RD_EINVAL, "sgd_table: tensor %d: weight, grad, mom and the images must be 16-byte aligned", i);
  if (t.pack_fwd || t.pack_bwd) {
    RD_REQUIRE(sgd_pack_shape_ok(t.cout, t.cin), RD_ESHAPE,
               "sgd_table: tensor %d: images of a (%d, %d, 3, 3) weight -- 64 or 128 channels on either side, stride 1 (not the <= 16-channel "
               "body form, the stride-2 pair view, M16 images or the 72-channel concat)", i, t.cout, t.cin);
    RD_REQUIRE(sgd_ntaps(t.n, t.cout, t.cin) != 0, RD_ESHAPE, "sgd_table: tensor %d: n %ld is not 9 x %d x %d (3x3) or 1 x that (1x1)", i, t.n, t.cout, t.cin);
  }
  RD_REQUIRE(!t.fold_scale || t.pack_fwd, RD_EINVAL, "sgd_table: tensor %d: a fold scale without a forward image", i);
  RD_REQUIRE(t.stride_w >= 0 && t.stride_w <= 2, RD_EINVAL, "sgd_table: tensor %d: stride_w %d (0 or 1: stride 1; 2: stride (1,2))", i, t.stride_w);
  if (sgd_is_s2(t))
    RD_REQUIRE(t.cin == t.cout && sgd_ntaps(t.n, t.cout, t.cin) == 9, RD_ESHAPE,
               "sgd_table: tensor %d: stride_w 2 images of a (%d, %d) weight with n %ld -- a (C, C, 3, 3) weight, C 64 or 128", i, t.cout, t.cin, t.n);
  return RD_OK;
}
inline long sgd_tensor_chunks(const rd_sgd_tensor_t& t) { return (t.n + SGD_CHUNK - 1) / SGD_CHUNK; }
inline long sgd_tensor_pack_chunks(const rd_sgd_tensor_t& t) {
  if (sgd_is_s2(t)) return (t.pack_fwd ? sgd_runs(sgd_s2_fwd_slots(t.cout)) : 0) + (t.pack_bwd ? 2 * sgd_runs(sgd_s2_phase_slots(t.cout)) : 0);
  const long per = (sgd_image_slots(t.cout, t.cin, sgd_ntaps(t.n, t.cout, t.cin)) + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS;
  return (t.pack_fwd ? per : 0) + (t.pack_bwd ? per : 0);
}
inline size_t sgd_table_size(long nt, long n_chunks, long n_pack) {
  return sizeof(SgdHeader) + (size_t)nt * sizeof(SgdEntry) + (size_t)n_chunks * sizeof(SgdChunk) + (size_t)n_pack * sizeof(SgdPackChunk);
}
inline void sgd_table_build(const rd_sgd_tensor_t* t, int nt, int dtype, long n_chunks, long n_pack, void* out) {
  SgdHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = SGD_MAGIC; h.nt = nt; h.n_chunks = (int)n_chunks; h.n_pack = (int)n_pack; h.dtype = dtype;
  h.off_entries = sizeof(SgdHeader);
  h.off_chunks = h.off_entries + (unsigned)(nt * sizeof(SgdEntry));
  h.off_pack = h.off_chunks + (unsigned)(n_chunks * sizeof(SgdChunk));
  h.bytes = (unsigned)sgd_table_size(nt, n_chunks, n_pack);
  unsigned char* base = (unsigned char*)out;
  memcpy(base, &h, sizeof(h));
  SgdEntry* e = (SgdEntry*)(base + h.off_entries);
  SgdChunk* c = (SgdChunk*)(base + h.off_chunks);
  SgdPackChunk* p = (SgdPackChunk*)(base + h.off_pack);
  for (int i = 0; i < nt; ++i) {
    memset(&e[i], 0, sizeof(SgdEntry));
    e[i].w = (float*)t[i].weight; e[i].g = (const float*)t[i].grad; e[i].m = (float*)t[i].mom; e[i].n = t[i].n;
    e[i].lr_mult = t[i].lr_mult; e[i].wd_mult = t[i].wd_mult; e[i].cout = t[i].cout; e[i].cin = t[i].cin;
    e[i].fwd = (unsigned short*)t[i].pack_fwd; e[i].bwd = (unsigned short*)t[i].pack_bwd; e[i].fold = t[i].fold_scale;
    for (long k = 0; k < sgd_tensor_chunks(t[i]); ++k) *c++ = SgdChunk{i, (int)k};
    if (sgd_is_s2(t[i])) {
      if (t[i].pack_fwd)
        for (long k = 0; k < sgd_runs(sgd_s2_fwd_slots(t[i].cout)); ++k) *p++ = SgdPackChunk{i, 2, (int)k, 0};
      for (int ph = 0; ph < 2 && t[i].pack_bwd; ++ph)
        for (long k = 0; k < sgd_runs(sgd_s2_phase_slots(t[i].cout)); ++k) *p++ = SgdPackChunk{i, 3 + ph, (int)k, 0};
      continue;
    }
    const long per = (sgd_image_slots(t[i].cout, t[i].cin, sgd_ntaps(t[i].n, t[i].cout, t[i].cin)) + SGD_PACK_SLOTS - 1) / SGD_PACK_SLOTS;
    for (int im = 0; im < 2; ++im)
      if (im == 0 ? t[i].pack_fwd : t[i].pack_bwd)
        for (long k = 0; k < per; ++k) *p++ = SgdPackChunk{i, im, (int)k, 0};
  }
}

struct SgdStep { float lr, momentum, wd, rescale, clip; };

__device__ __forceinline__ void sgd_one(float& w, float g, float& m, float lr_t, float lrwd, const SgdStep& s) {
  _Pragma("clang fp contract(off)")
  g = s.rescale * g;
  if (s.clip >= 0.f) g = g > s.clip ? s.clip : (g < -s.clip ? -s.clip : g);
  const float a = s.momentum * m;
  const float b = lrwd * w;
  const float c = lr_t * g;
  m = (a - b) - c;
  w = w + m;
}

__global__ __launch_bounds__(256) void sgd_mom_kernel(const unsigned char* __restrict__ table, SgdStep s) {
  _Pragma("clang fp contract(off)")
  const SgdHeader* h = (const SgdHeader*)table;
  const SgdChunk ck = ((const SgdChunk*)(table + h->off_chunks))[blockIdx.x];
  const SgdEntry e = ((const SgdEntry*)(table + h->off_entries))[ck.tensor];
  const float lr_t = s.lr * e.lr_mult, wd_t = s.wd * e.wd_mult, lrwd = lr_t * wd_t;
  const long base = (long)ck.chunk * SGD_CHUNK, i = base + 4 * (long)threadIdx.x, nv = e.n & ~3L;
  if (i < nv) {   // i is a multiple of 4: the whole vector lies below nv
    f32x4 w = *(const f32x4*)(e.w + i), m = *(const f32x4*)(e.m + i);
    const f32x4 g = *(const f32x4*)(e.g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = w[j], mj = m[j];
      sgd_one(wj, g[j], mj, lr_t, lrwd, s);
      w[j] = wj;
      m[j] = mj;
    }
    *(f32x4*)(e.m + i) = m;
    *(f32x4*)(e.w + i) = w;
  }
  // the scalar tail: elements nv .. n - 1 (at most three), by the first threads of the chunk that holds element nv
  const long t = nv + threadIdx.x;
  if (threadIdx.x < 3 && t < e.n && nv >= base && nv < base + SGD_CHUNK) {
    float wj = e.w[t], mj = e.m[t];
    sgd_one(wj, e.g[t], mj, lr_t, lrwd, s);
    e.m[t] = mj;
    e.w[t] = wj;
  }
}

// one 16-byte slot of one image of a (cout, cin, 3, 3) (nt 9) or (cout, cin, 1, 1) (nt 1) float32 weight; image 0: forward (fold may be
// NULL), 1: data gradient
template <int DT>
__device__ __forceinline__ void sgd_pack_slot(const float* __restrict__ w, const float* __restrict__ fold, int cout, int cin, int image,
                                              long slot, unsigned short* __restrict__ out, int nt = 9) {
  _Pragma("clang fp contract(off)")
  const long body = (long)nt * cout * cin / 8;
  if (slot >= body + (long)(RD_CONV_TAIL / 16)) return;
  Slot16 o = {0u, 0u, 0u, 0u};
  if (slot < body) {
    const int ncb = (image ? cin : cout) / 32, lg = ncb >> 1;   // ncb is 2 or 4: its logarithm
    const int s = (int)slot, lane = s & 63, cb = (s >> 6) & (ncb - 1);
    const int u = s >> (6 + lg);                             // (c * 9 + t) * 2 + ks
    const int ks = u & 1, t = (u >> 1) % nt, c = (u >> 1) / nt;
    const int r = 32 * cb + conv_row_perm(lane & 31), q0 = 32 * c + 16 * ks + 8 * (lane >> 5);
    float f[8];
    if (image == 0) {
      const float sc = fold ? fold[r] : 1.f;
      const float* src = w + ((long)r * cin + q0) * nt + t;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = sc * src[nt * j];
    } else {
      const float* src = w + ((long)q0 * cin + r) * nt + (nt - 1 - t);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = src[(long)nt * cin * j];
    }
    o = slot_pack<DT>(f);
  }
  *(Slot16*)(out + 8 * slot) = o;
}

// The eight values of one slot of a PHASE image of a transposed conv (3, KW) / stride (1, s) / pad (1, p) with KW = 2 s: pack_taps_frag(6,
// cin, cout) on the phase's six taps in ascending (dh, dw) order, i.e. tap rows kh = 2, 1, 0 and in each the columns kw_lo + s (dw = -1 or
// 0) then kw_lo = (phase + p) % s (one more).  w is a (Cin, Cout, 3, kwm) master; a column kw >= kwm does not exist and reads as zero (the
// strided conv's data gradient: kwm = 3 under KW = 4).  step = 6 * (32-channel chunk) + tap, q0 the first of the slot's eight input
// channels, r its output channel.  Shared by the optimizer's strided re-pack and rd_pack_deconv_dev.
__device__ __forceinline__ void deconv_phase_vals(const float* __restrict__ w, int cout, int kwm, int s, int p, int phase, int step, int q0,
                                                  int r, float (&f)[8]) {
  const int t = step % 6, kh = 2 - t / 2, kw = (phase + p) % s + ((t & 1) ? 0 : s);
  const float* src = w + (((long)q0 * cout + r) * 3 + kh) * kwm + (kw < kwm ? kw : 0);
#pragma unroll
  for (int q = 0; q < 8; ++q) f[q] = kw < kwm ? src[(long)3 * kwm * cout * q] : 0.f;
}

// one 16-byte slot of an image of a (C, C, 3, 3) weight with stride (1,2): image 2 the forward image (fold may be NULL), 3 / 4 the data
// gradient's phase 0 / 1; `out` is the start of that image
template <int DT>
__device__ __forceinline__ void sgd_pack_slot_s2(const float* __restrict__ w, const float* __restrict__ fold, int C, int image, long slot,
                                                 unsigned short* __restrict__ out) {
  _Pragma("clang fp contract(off)")
  const long total = image == 2 ? sgd_s2_fwd_slots(C) : sgd_s2_phase_slots(C);
  // the host packer takes the body form only with a fold scale (conv3_body_s2: the launch form of folded weights); without one it
  // writes the six-tap form pack_taps_frag(6, 2 C, C), which fills the image
  const long body = image == 2 ? (long)(fold ? 18 : 24) * C * C / 16 : (long)12 * C * C / 16;
  if (slot >= total) return;
  Slot16 o = {0u, 0u, 0u, 0u};
  if (slot < body) {
    const int ncb = C / 32, s = (int)slot, lane = s & 63, cb = (s >> 6) % ncb, u = s / (64 * ncb);   // u = step * 2 + ks
    const int ks = u & 1, step = u >> 1;
    const int r = 32 * cb + conv_row_perm(lane & 31);
    float f[8];
    if (image == 2 && !fold) {
      const int t = step % 6, c = step / 6, dh = t >> 1, c0 = 32 * c + 16 * ks + 8 * (lane >> 5);   // view tap (dh, dw2 = (t & 1) - 1)
      const bool odd = c0 >= C, zero = !odd && !(t & 1);
      const int kx = odd ? ((t & 1) ? 2 : 0) : 1;
      const float* src = w + (((long)r * C + (c0 - (odd ? C : 0))) * 3 + dh) * 3 + kx;
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = zero ? 0.f : 1.f * src[9 * q];
    } else if (image == 2) {
      // step -> (unit of the group of four, ordinal): units [6 | 3 | 3 | 6] steps on chunks [odd r2 | even r2 | even r2 + 1 | odd r2 + 1]
      const int grp = step / 18, gs = step % 18, j = gs < 6 ? 0 : gs < 9 ? 1 : gs < 12 ? 2 : 3, so = gs - (j == 0 ? 0 : j == 1 ? 6 : j == 2 ? 9 : 12);
      const int ne = C / 32, r2 = 2 * grp, chunk = j == 0 ? ne + r2 : j == 1 ? r2 : j == 2 ? r2 + 1 : ne + r2 + 1;
      const bool odd = j == 0 || j == 3;
      const int dh = odd ? so >> 1 : so, kx = odd ? ((so & 1) ? 2 : 0) : 1;     // odd pixel: view column -1 is kx 0, column 0 is kx 2
      const int ci0 = 32 * chunk + 16 * ks + 8 * (lane >> 5) - (odd ? C : 0);
      const float sc = fold ? fold[r] : 1.f;
      const float* src = w + (((long)r * C + ci0) * 3 + dh) * 3 + kx;
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = sc * src[9 * q];
    } else {
      // phase 0: [kx 3, the appended zero column | kx 1], phase 1: [kx 2 | kx 0]
      deconv_phase_vals(w, C, 3, 2, 1, image - 3, step, 32 * (step / 6) + 16 * ks + 8 * (lane >> 5), r, f);
    }
    o = slot_pack<DT>(f);
  }
  *(Slot16*)(out + 8 * slot) = o;
}

template <int DT>
__global__ __launch_bounds__(256) void sgd_pack_kernel(const unsigned char* __restrict__ table) {
  const SgdHeader* h = (const SgdHeader*)table;
  const SgdPackChunk pk = ((const SgdPackChunk*)(table + h->off_pack))[blockIdx.x];
  const SgdEntry e = ((const SgdEntry*)(table + h->off_entries))[pk.tensor];
  if (pk.image >= 2) {       // uniform over the workgroup
    unsigned short* out = pk.image == 2 ? e.fwd : e.bwd + (pk.image - 3) * 8 * sgd_s2_phase_slots(e.cout);
    sgd_pack_slot_s2<DT>(e.w, e.fold, e.cout, pk.image, (long)pk.run * SGD_PACK_SLOTS + threadIdx.x, out);
    return;
  }
  sgd_pack_slot<DT>(e.w, e.fold, e.cout, e.cin, pk.image, (long)pk.run * SGD_PACK_SLOTS + threadIdx.x, pk.image ? e.bwd : e.fwd,
                    sgd_ntaps(e.n, e.cout, e.cin));
}

// ---- the images of a transposed conv (3, KW) / stride (1, s) / pad (1, p), KW = 2 s, from its (Cin, Cout, 3, KW) float32 master -------------
// mode 0: the s forward phase images, pack_taps_frag(6, cin, cout) each with its zero tail (rd_pack_deconv_weight_folded_host without a
//         scale), phase ph at ph * phase_stride elements of `out`
// mode 1: the data-gradient image: pack_taps_frag(9, s cout, cin) of Wv[ci][e cout + co][kh][dwv + 1] = W[ci][co][kh][s dwv + e + p] (zero
//         where that column does not exist) -- the 3x3 stride-1 conv over the gradient read as [H][Win][s Cout] -- and its zero tail
// One thread per 16-byte slot; grid = ceil(slots / 256).
__host__ __device__ inline long deconv_phase_slots(int cin, int cout) { return (long)(12 * cin * cout + (int)RD_CONV_TAIL) / 16; }
__host__ __device__ inline long deconv_dgrad_slots(int cin, int cout, int s) { return (long)(18 * s * cin * cout + (int)RD_CONV_TAIL) / 16; }
template <int DT>
__global__ __launch_bounds__(256) void pack_deconv_dev_kernel(const float* __restrict__ w, int cin, int cout, int kw, int s, int p, int mode,
                                                              long phase_stride, unsigned short* __restrict__ out) {
  _Pragma("clang fp contract(off)")
  const long g = (long)blockIdx.x * SGD_PACK_SLOTS + threadIdx.x;
  const long per = mode ? deconv_dgrad_slots(cin, cout, s) : deconv_phase_slots(cin, cout);
  const long body = mode ? (long)18 * s * cin * cout / 16 : (long)12 * cin * cout / 16;
  if (g >= (mode ? per : per * s)) return;
  const int phase = mode ? 0 : (int)(g / per);
  const long slot = g - phase * per;
  Slot16 o = {0u, 0u, 0u, 0u};
  if (slot < body) {
    const int ncb = (mode ? cin : cout) / 32, sl = (int)slot, lane = sl & 63, cb = (sl >> 6) % ncb, u = sl / (64 * ncb);
    const int ks = u & 1, step = u >> 1;           // step = (32-channel chunk) * taps + tap
    const int r = 32 * cb + conv_row_perm(lane & 31);
    float f[8];
    if (mode == 0) {
      deconv_phase_vals(w, cout, kw, s, p, phase, step, 32 * (step / 6) + 16 * ks + 8 * (lane >> 5), r, f);
    } else {
      const int t = step % 9, q0 = 32 * (step / 9) + 16 * ks + 8 * (lane >> 5);      // q0: view channel e cout + co
      const int e = q0 / cout, co = q0 - e * cout, kx = s * (t % 3 - 1) + e + p;
      const bool in = kx >= 0 && kx < kw;
      const float* src = w + (((long)r * cout + co) * 3 + t / 3) * kw + (in ? kx : 0);
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = in ? src[(long)3 * kw * q] : 0.f;
    }
    o = slot_pack<DT>(f);
  }
  *(Slot16*)(out + phase * phase_stride + 8 * slot) = o;
}

// the single-tensor form: grid = ceil(slots / 256)
template <int DT>
__global__ __launch_bounds__(256) void pack_conv3x3_dev_kernel(const float* __restrict__ w, const float* __restrict__ fold, int cout, int cin,
                                                               int flip, unsigned short* __restrict__ out) {
  sgd_pack_slot<DT>(w, fold, cout, cin, flip, (long)blockIdx.x * SGD_PACK_SLOTS + threadIdx.x, out);
}
}  // namespace rd
