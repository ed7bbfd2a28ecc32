// Device helpers shared by the kernel translation units
// (decode_kernels.hip, attn_mha_kernels.hip): bf16 / fp8 conversions, wave
// reductions, the rope element and the decode-attention block constants.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define DEVINL __device__ __forceinline__

using bf16 = __hip_bfloat16;

DEVINL float b2f(bf16 v) { return __bfloat162float(v); }
DEVINL bf16 f2b(float v) { return __float2bfloat16(v); }

// 8 bf16 loaded as one int4 (16 B)
struct bf16x8 {
  bf16 v[8];
};

DEVINL bf16x8 load8(const bf16* p) {
  bf16x8 r;
  *reinterpret_cast<int4*>(r.v) = *reinterpret_cast<const int4*>(p);
  return r;
}

// nontemporal variant for streamed-once weight reads (no L2 retention);
// the builtin needs a clang ext_vector type, not HIP's int4 struct
using i32x4_t = __attribute__((ext_vector_type(4))) int;

DEVINL bf16x8 load8_nt(const bf16* p) {
  bf16x8 r;
  *reinterpret_cast<i32x4_t*>(r.v) =
      __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(p));
  return r;
}

DEVINL i32x4_t load16_nt_u8(const unsigned char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(p));
}

using i32x2_t = __attribute__((ext_vector_type(2))) int;

DEVINL i32x2_t load8_nt_u8(const unsigned char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const i32x2_t*>(p));
}

using f32x4 = __attribute__((__vector_size__(16))) float;
using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;

DEVINL float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- fp8 (OCP e4m3) KV cache -------------------------------------------
// Rows are stored per-row-scaled (one fp32 scale per cached (slot, layer,
// kv-head, position) row, absmax/448 — same scheme as the fp8 weights).
// gfx950 cvt builtins convert packed pairs; KV8 kernel variants load 8
// bytes instead of 16 per fragment and dequantize in registers.
using u8kv = unsigned char;
typedef float v2fkv __attribute__((ext_vector_type(2)));

DEVINL u8kv f32_to_fp8(float f) {
  const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(f, 0.f, 0, false);
  return (u8kv)(packed & 0xFF);
}

DEVINL float fp8_to_f32(u8kv v) {
  return __builtin_amdgcn_cvt_f32_fp8((int)v, 0);
}

DEVINL bf16x8_t fp8x8_to_bf16(const u8kv* p, float scl) {
  const int lo = *reinterpret_cast<const int*>(p);
  const int hi = *reinterpret_cast<const int*>(p + 4);
  const v2fkv a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
  const v2fkv b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  const v2fkv c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
  const v2fkv d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  bf16x8_t r;
  r[0] = (__bf16)(a.x * scl);
  r[1] = (__bf16)(a.y * scl);
  r[2] = (__bf16)(b.x * scl);
  r[3] = (__bf16)(b.y * scl);
  r[4] = (__bf16)(c.x * scl);
  r[5] = (__bf16)(c.y * scl);
  r[6] = (__bf16)(d.x * scl);
  r[7] = (__bf16)(d.y * scl);
  return r;
}

// 8 fp8 bytes (k ascending: lo then hi) -> 8 bf16, unscaled.  e4m3 has 3
// mantissa bits, so the fp32 convert is exact and its low 16 bits are
// zero: keeping the high halves IS the bf16 value (no rounding step).
DEVINL unsigned bf16_pair_hi(float a, float b) {
  return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);
}

DEVINL bf16x8_t fp8x8_to_bf16_exact(int lo, int hi) {
  const v2fkv a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
  const v2fkv b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  const v2fkv c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
  const v2fkv d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  unsigned w[4] = {bf16_pair_hi(a.x, a.y), bf16_pair_hi(b.x, b.y),
                   bf16_pair_hi(c.x, c.y), bf16_pair_hi(d.x, d.y)};
  return *reinterpret_cast<const bf16x8_t*>(w);
}

// PV accumulate straight from the fp8 pairs (skips the bf16 round trip
// the MFMA-operand path needs)
DEVINL void fp8x8_fma(float* o, float pw, const u8kv* p, float scl) {
  const int lo = *reinterpret_cast<const int*>(p);
  const int hi = *reinterpret_cast<const int*>(p + 4);
  const v2fkv a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false);
  const v2fkv b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  const v2fkv c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false);
  const v2fkv d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  const float ps = pw * scl;
  o[0] += ps * a.x;
  o[1] += ps * a.y;
  o[2] += ps * b.x;
  o[3] += ps * b.y;
  o[4] += ps * c.x;
  o[5] += ps * c.y;
  o[6] += ps * d.x;
  o[7] += ps * d.y;
}

// atomicMax for a non-negative float held in LDS as its uint bits
DEVINL void lds_fmax_u(unsigned* addr, float v) {
  atomicMax(addr, __float_as_uint(v));
}

DEVINL float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

#define ATTN_WAVES 4  // waves per block, each fully independent
// max_seq at/below which the one-launch block-local variant is used; the
// choice is static per engine (max_seq), so hipGraph shapes never change
#define ATTN_BLOCK_MAX_SEQ 4096

// rotate-half rope of one element d of a head row (raw pointer into qkv)
DEVINL float rope_elem(const bf16* row, int d, int ne,
                       const float* __restrict__ cos_t,
                       const float* __restrict__ sin_t, int pos) {
  float x = b2f(row[d]);
  if (d >= ne) return x;
  const int half = ne >> 1;
  const float c = cos_t[(size_t)pos * ne + d];
  const float s = sin_t[(size_t)pos * ne + d];
  if (d < half) return x * c - b2f(row[d + half]) * s;
  return x * c + b2f(row[d - half]) * s;
}
