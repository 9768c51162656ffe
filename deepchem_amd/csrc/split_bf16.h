// Three-way bf16 split of fp32 operands for the bf16 matrix cores, and what every matrix-core kernel does with the
// pieces: the six-product sequence, the 32x32 accumulator layout, the prepared fragment images.
#pragma once
#include "common.h"

namespace gcmi {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The tile row that register `reg` of a 32x32 MFMA accumulator holds in the lanes of half `half` (lane >> 5); the
// column is lane & 31.  The same for the bf16 and the fp32 instruction (gemm.hip).
constexpr int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }
constexpr bool acc_row_is_a_permutation() {
  unsigned seen = 0;
  for (int half = 0; half < 2; ++half)
    for (int reg = 0; reg < 16; ++reg) {
      const int row = acc_row(reg, half);
      if (row < 0 || row > 31 || (seen >> row & 1u)) return false;
      seen |= 1u << row;
    }
  return seen == 0xFFFFFFFFu;
}
static_assert(acc_row_is_a_permutation(), "acc_row must hit every row 0..31 exactly once");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Round-to-nearest three-way split, two values at a time (v_cvt_pk_bf16_f32 packs the pair):
// x = p1 + p2 + p3 + r3 with |p2| <= 2^-8 |x|, |p3| <= 2^-16 |x|, |r3| <= 2^-24 |x| and signed,
// unbiased residuals.  The six products kept below drop p2*q3 + p3*q2 + p3*q3 <= 2^-23 |x||y|.
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& p1, unsigned& p2, unsigned& p3) {
  f32x2 v = {x0, x1};
  p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  const f32x2 f1 = {__uint_as_float(p1 << 16), __uint_as_float(p1 & 0xFFFF0000u)};
  const f32x2 r1 = v - f1;  // exact
  p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
  const f32x2 f2 = {__uint_as_float(p2 << 16), __uint_as_float(p2 & 0xFFFF0000u)};
  const f32x2 r2 = r1 - f2;  // exact
  p3 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}

// one value: the three bf16 pieces in the low halves of p1..p3
__device__ __forceinline__ void split3(float x, unsigned& p1, unsigned& p2, unsigned& p3) {
  unsigned q1, q2, q3;
  split3_pair(x, 0.f, q1, q2, q3);
  p1 = q1 << 16;  // callers take the piece from the HIGH half
  p2 = q2 << 16;
  p3 = q3 << 16;
}

// ---- bfloat16 activation storage (gcmi_model_desc.storage == 1): raw 16-bit patterns in HBM, fp32 everywhere else
typedef unsigned short bf16_t;

// two floats -> one dword of two bf16 (round to nearest even, v_cvt_pk_bf16_f32; a NaN stays a NaN): low half = a
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
// the value a float has after one trip through bf16 storage
__device__ __forceinline__ float round_bf16(float a) { return bf16_lo(pack_bf16x2(a, 0.f)); }
// 8 (4) bf16 of a 16-byte (8-byte) piece -> floats
__device__ __forceinline__ void widen8(const uint4 r, float (&v)[8]) {
  v[0] = bf16_lo(r.x); v[1] = bf16_hi(r.x); v[2] = bf16_lo(r.y); v[3] = bf16_hi(r.y);
  v[4] = bf16_lo(r.z); v[5] = bf16_hi(r.z); v[6] = bf16_lo(r.w); v[7] = bf16_hi(r.w);
}
__device__ __forceinline__ float4 widen4(const uint2 r) {
  return make_float4(bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y));
}
__device__ __forceinline__ uint2 narrow4(float a, float b, float c, float d) {
  return make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}
// two floats that ARE bf16 values (low 16 bits zero) -> their packed pair, exactly (one v_perm_b32)
__device__ __forceinline__ unsigned pack_exact_bf16x2(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}

struct Frag3 {
  u32x4 p[3];
};

__device__ __forceinline__ Frag3 split_frag(const float (&v)[8]) {
  Frag3 f;
  unsigned q[3][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split3_pair(v[2 * i], v[2 * i + 1], q[0][i], q[1][i], q[2][i]);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    f.p[s].x = q[s][0];
    f.p[s].y = q[s][1];
    f.p[s].z = q[s][2];
    f.p[s].w = q[s][3];
  }
  return f;
}

__device__ __forceinline__ Frag3 split_frag(const float4 lo, const float4 hi) {
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return split_frag(v);
}

__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) {
  return __builtin_bit_cast(bf16x8, v);
}

// acc += A . B, both operands split three ways: six of the nine piece products, in two halves.  The three left out,
// A2 B3 + A3 B2 + A3 B3, are below 2^-23 |a||b| (split3_pair): under the rounding of the fp32 accumulation itself.  The
// small terms go first, so that they are summed among themselves before the leading product swamps them.  The order is
// part of the numerics that the tests pin to float32 accuracy: a kernel takes it from here.  (The one exception,
// bwd_fused.hip's interleaved path, spells the same six out between its scheduling barriers.)
// ... the terms of order 2^-16: A3 B1, A1 B3, A2 B2
__device__ __forceinline__ void mfma_split3_small(f32x16& acc, const Frag3& a, const Frag3& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[2]), as_bf16x8(b.p[0]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[0]), as_bf16x8(b.p[2]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[1]), as_bf16x8(b.p[1]), acc, 0, 0, 0);
}
// ... the terms of order 2^-8 and 1: A2 B1, A1 B2, A1 B1.  On their own (they read p[0] and p[1] only): a product
// whose result goes to bf16 storage, which rounds away more than the small terms add (bwd_fused.hip)
__device__ __forceinline__ void mfma_split3_large(f32x16& acc, const Frag3& a, const Frag3& b) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[1]), as_bf16x8(b.p[0]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[0]), as_bf16x8(b.p[1]), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a.p[0]), as_bf16x8(b.p[0]), acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_split6(f32x16& acc, const Frag3& a, const Frag3& b) {
  mfma_split3_small(acc, a, b);
  mfma_split3_large(acc, a, b);
}

__device__ __forceinline__ f32x16 zero_acc() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// The prepared fragment image [...][piece][lane]: 16-byte entries, the three pieces of a lane's fragment 64 entries (one
// wave's lanes) apart.  `entry` points at the caller's lane in piece 0.
__device__ __forceinline__ void store_frag3(u32x4* entry, const Frag3& f) {
  entry[0] = f.p[0];
  entry[64] = f.p[1];
  entry[128] = f.p[2];
}
__device__ __forceinline__ Frag3 load_frag3(const u32x4* entry) { return {{entry[0], entry[64], entry[128]}}; }

// Floats per row of a 32 x 64 transposition tile in LDS: 17 16-byte pieces, so that the fragment reads down a column
// and the float4 writes along a row are both free of bank conflicts.
constexpr int kTilePitch = 68;

}  // namespace gcmi
