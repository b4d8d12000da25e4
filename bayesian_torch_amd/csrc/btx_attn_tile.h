// btx_attn_tile.h — what the attention kernels share (btx_attn.hip, btx_attn_bwd.hip): the vector types of the MFMA operands, the
// element loads of an activation tensor and the 16-byte LDS unit of the operand type.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/btx_attn_bias.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

namespace {

__device__ __forceinline__ uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {  // v_cvt_pk_bf16_f32, round to nearest even
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// N (4 or 8) consecutive elements at element offset `off` of an ACT tensor, as f32 (exact)
template <int ACT, int N>
__device__ __forceinline__ void load_elems(const void* base, int64_t off, bool vec, float (&f)[N]) {
  if constexpr (ACT == BTX_ACT_F32) {
    const float* p = (const float*)base + off;
    if (vec) {
#pragma unroll
      for (int i = 0; i < N / 4; ++i) {
        const f32x4 t = *(const f32x4*)(p + 4 * i);
        f[4 * i] = t[0]; f[4 * i + 1] = t[1]; f[4 * i + 2] = t[2]; f[4 * i + 3] = t[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = p[i];
    }
  } else {
    const uint16_t* p = (const uint16_t*)base + off;
    if (vec) {
      uint32_t w[N / 2];
      if constexpr (N == 8) {
        const u32x4 t = *(const u32x4*)p;
        w[0] = t[0]; w[1] = t[1]; w[2] = t[2]; w[3] = t[3];
      } else {
        const u32x2 t = *(const u32x2*)p;
        w[0] = t[0]; w[1] = t[1];
      }
#pragma unroll
      for (int i = 0; i < N / 2; ++i) { f[2 * i] = u2f(w[i] << 16); f[2 * i + 1] = u2f(w[i] & 0xffff0000u); }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) f[i] = u2f((uint32_t)p[i] << 16);
    }
  }
}

// one 16-byte LDS unit of the operand type: 8 bf16 (PREC 1) or 4 f32 (PREC 0)
template <int PREC, int N>
__device__ __forceinline__ u32x4 pack_unit(const float (&f)[N]) {
  if constexpr (PREC == BTX_PREC_BF16) return (u32x4){pk_bf16(f[0], f[1]), pk_bf16(f[2], f[3]), pk_bf16(f[4], f[5]), pk_bf16(f[6], f[7])};
  else return (u32x4){f2u(f[0]), f2u(f[1]), f2u(f[2]), f2u(f[3])};
}

// four consecutive f32 results stored as ACT elements at element offset `off` (16-byte / 8-byte store on the grid, else per element)
template <int ACT>
__device__ __forceinline__ void store4(void* base, int64_t off, bool vec, const float (&r4)[4]) {
  if constexpr (ACT == BTX_ACT_F32) {
    float* p = (float*)base + off;
    if (vec) *(f32x4*)p = (f32x4){r4[0], r4[1], r4[2], r4[3]};
    else { p[0] = r4[0]; p[1] = r4[1]; p[2] = r4[2]; p[3] = r4[3]; }
  } else {
    uint16_t* p = (uint16_t*)base + off;
    const uint32_t w0 = pk_bf16(r4[0], r4[1]), w1 = pk_bf16(r4[2], r4[3]);
    if (vec) *(u32x2*)p = (u32x2){w0, w1};
    else { p[0] = (uint16_t)w0; p[1] = (uint16_t)(w0 >> 16); p[2] = (uint16_t)w1; p[3] = (uint16_t)(w1 >> 16); }
  }
}

// ---- the additive score bias of the BIAS instantiations (include/btx_attn_bias.h) -------------------------
constexpr float BIAS_LOG2E = 1.44269504088896340736f;

struct BiasOp {
  const void* p;
  int64_t s[3];  // (row, head, query) strides in elements; the key axis is contiguous
  int rows, dtype;
  uint32_t vec;  // base and strides on the grid of the four-key load (16 / 8 / 4 bytes)
};

// n (1..4) consecutive bias elements at element offset `off` as f32: f32 as it is, bf16 widened, bytes as 0 / -inf.  The element type
// is the same in every lane (a wave-uniform branch); elements n..3 are not read and stay 0.
__device__ __forceinline__ void load_bias4(const BiasOp& b, int64_t off, int n, float (&f)[4]) {
  const bool v4 = b.vec && n == 4;
  f[0] = f[1] = f[2] = f[3] = 0.f;
  if (b.dtype == BTX_BIAS_F32) {
    const float* p = (const float*)b.p + off;
    if (v4) {
      const f32x4 t = *(const f32x4*)p;
      f[0] = t[0]; f[1] = t[1]; f[2] = t[2]; f[3] = t[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) f[e] = p[e];
    }
  } else if (b.dtype == BTX_BIAS_BF16) {
    const uint16_t* p = (const uint16_t*)b.p + off;
    if (v4) {
      const u32x2 t = *(const u32x2*)p;
      f[0] = u2f(t[0] << 16); f[1] = u2f(t[0] & 0xffff0000u); f[2] = u2f(t[1] << 16); f[3] = u2f(t[1] & 0xffff0000u);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) f[e] = u2f((uint32_t)p[e] << 16);
    }
  } else {
    const uint8_t* p = (const uint8_t*)b.p + off;
    uint32_t w = 0;
    if (v4) {
      w = *(const uint32_t*)p;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) w |= (uint32_t)p[e] << (8 * e);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = ((w >> (8 * e)) & 0xffu) ? -__builtin_huge_valf() : 0.f;
  }
}

// the checks of the bias arguments, before any launch; fills `b`
inline int bias_operand(const void* bias, int dtype, int rows, const int64_t strides[3], BiasOp& b) {
  if (!strides) return BTX_E_NULL;
  if (dtype != BTX_BIAS_F32 && dtype != BTX_BIAS_BF16 && dtype != BTX_BIAS_U8) return BTX_E_DTYPE;
  if (rows <= 0 || strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return BTX_E_SHAPE;
  const int64_t esz = dtype == BTX_BIAS_F32 ? 4 : dtype == BTX_BIAS_BF16 ? 2 : 1;
  if ((uintptr_t)bias % esz) return BTX_E_ALIGN;  // below the element's own alignment
  b.p = bias;
  b.rows = rows;
  b.dtype = dtype;
  b.vec = (uintptr_t)bias % (4 * esz) == 0;
  for (int i = 0; i < 3; ++i) {
    b.s[i] = strides[i];
    if (strides[i] % 4) b.vec = 0;
  }
  return 0;
}

}  // namespace
