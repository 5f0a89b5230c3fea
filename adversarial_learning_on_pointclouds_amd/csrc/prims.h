// Device primitives shared by every kernel file (gfx950 / CDNA4 only), each
// defined once: vector types, MFMA wrappers, the f32 -> bf16 plane split, DPP
// and butterfly reductions, the argmax order and the screening keys.
// Included through common.h.
#pragma once
#include <hip/hip_runtime.h>

namespace pcadv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// MFMA wrappers
// ---------------------------------------------------------------------------
// 32x32x2 f32 MFMA: exact f32 (k-ordered fma chain), 64 cycles / SIMD.
// lane l supplies A[i=l&31][k=l>>5], B[k=l>>5][j=l&31];
// D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5).
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int acc_row(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
// 16x16x4 f32 MFMA (exact f32): lane l supplies A[i=l&15][k=l>>4] and
// B[k=l>>4][j=l&15]; D: col = l&15, row = 4*(l>>4) + r.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// the bf16 forms (f32 accumulators laid out as above): 32x32x16 and 16x16x32,
// eight consecutive k per lane
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// f32 -> NPL bf16 planes whose sum is the f32 value (round-to-nearest splits:
// each residual is exact in f32).  NPL = 2 (hi, lo): 16 significant bits;
// NPL = 3 (hi, mid, lo): the whole significand, the last residual fits 8 bits.
// Six products of two 3-plane splits (l h, m m, h l, m h, h m, h h; the dropped
// terms are < 2^-23 of |a b|) give an f32-level product on the bf16 matrix pipe.
// ---------------------------------------------------------------------------
template <int NPL>
__device__ __forceinline__ void split_planes(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
  hi = (__bf16)v;
  const float r1 = v - (float)hi;
  mid = (__bf16)r1;
  if (NPL == 3) lo = (__bf16)(r1 - (float)mid);
}

// ---------------------------------------------------------------------------
// DPP moves and cross-lane reductions.  Every lane of a group adds the same
// operands in the same order, so all get bitwise the same total.
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}
// Sum over each octet of lanes (8 k .. 8 k + 7), the total in all eight
__device__ __forceinline__ float octet_sum(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]: xor 1
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]: xor 2
  v += dpp<0x141>(v);  // row_half_mirror: lane i <- 7 - i within 8 (the other quad)
  return v;
}
// Sum over the 32 lanes of each half-wave: the octet ladder, the row mirror,
// then one swizzle across the two rows
__device__ __forceinline__ float half_sum(float v) {
  v = octet_sum(v);
  v += dpp<0x140>(v);  // row_mirror: lane i <- 15 - i within 16 (the other 8)
  v += __shfl_xor(v, 16);
  return v;
}
// 64-lane butterflies: the sum (float, double, int, long long) or the maximum
// over the wave, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---------------------------------------------------------------------------
// The argmax order, stated once: (va, ia) ranks before (vb, ib) when va is the
// larger value, a NaN ranking above every number (+inf included), and on equal
// values (two NaNs are equal here) when ia is the lower index.  It is the order
// of torch.max and np.argmax, so every pooled index and every predicted label
// agrees with them.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool ranks_before(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}
// The same order where candidates arrive by increasing index: v replaces best
// only when strictly above it, so the earlier index keeps a tie.
__device__ __forceinline__ bool beats(float v, float best) {
  return v > best || (v != v && best == best);
}

// ---------------------------------------------------------------------------
// Screening keys: the f32 value mapped to an order-preserving int32 whose low
// LOW bits are replaced by 2^LOW - 1 - row (row < 2^LOW: the value's row in its
// tile), so v_max_i32 / v_med3_i32 keep the top-2 (value, row) of a lane with
// the lower row first on equal truncated values.  The dropped bits (2^(LOW-23)
// relative) only order the candidates, which an exact re-evaluation then ranks
// by their f32 values; NaN maps above +inf, as the argmax order ranks it.
// ---------------------------------------------------------------------------
template <int LOW>
__device__ __forceinline__ int screen_key(float v, int row) {
  const int b = __float_as_int(v);
  const int ord = b ^ ((b >> 31) & 0x7fffffff);  // int order == float order
  return (ord & ~((1 << LOW) - 1)) | ((1 << LOW) - 1 - row);
}
template <int LOW>
__device__ __forceinline__ float key_value(int k) {
  const int ord = k & ~((1 << LOW) - 1);
  return __int_as_float(ord ^ ((ord >> 31) & 0x7fffffff));
}
constexpr int KEY_NONE = (int)0x80000000;  // below every real key

}  // namespace pcadv
