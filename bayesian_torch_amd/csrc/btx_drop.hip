// btx_drop.hip — BTX-DROP v1: Monte-Carlo dropout on BTX-RNG v1 (include/btx_drop.h).  One launch per call, forward
// and backward alike (dx = drop(dy): the mask is regenerated from the key, nothing is saved).  Two kernels:
//   drop_group_kernel   memory order == index order in runs of 8 (BTX_DROP_CL: element mode; channel mode with C % 8 == 0): one
//                       Philox4x32-10 call per 8 consecutive elements per thread, 16-byte accesses when the lane's two base
//                       addresses are on the 16-byte grid, element-wise accesses otherwise and for the last n % 8 elements
//   drop_index_kernel   everything else (BTX_DROP_NCS, channel mode with a ragged C): one element per thread per step, its
//                       index derived from its memory offset, one Philox call per element
// Lanes are grid.y; every lane reads its own sample word.  A workgroup owns BTX_DROP_CHUNK elements of one lane: the grid follows
// the element count, not the machine.  HBM-bound by design (4 to 8 bytes per element against ~1/8 Philox call).  gfx950 only.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/btx_drop.h"
#include "btx_rng.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int DROP_BLOCK = 256;
constexpr int DROP_CHUNK = BTX_DROP_CHUNK;
static_assert(DROP_CHUNK % (DROP_BLOCK * 8) == 0, "a chunk is a whole number of sweeps of 8 elements per thread");

struct DropArgs {
  const void* x;
  void* out;
  uint64_t n;          // elements of one lane
  uint64_t x_stride;   // elements between the lanes of x: n, or 0 (broadcast)
  uint64_t S, C;
  uint32_t T;
  float scale;
  uint32_t k0, k1, sample, layer;
  const uint32_t* sample_ptr;
};

__device__ __forceinline__ float bf16_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// RNE; NaN -> the canonical quiet NaN 0x7fc0 (what torch's conversion gives)
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ uint32_t drop_bits(const BtxPhilox4& p, uint32_t j) {  // j = i & 7
  const uint32_t w = j >> 1;
  const uint32_t v = w == 0 ? p.x[0] : (w == 1 ? p.x[1] : (w == 2 ? p.x[2] : p.x[3]));
  return (v >> (16u * (j & 1u))) & 0xffffu;
}

__device__ __forceinline__ float drop_f32(float v, bool keep, float scale) { return keep ? v * scale : 0.0f; }
__device__ __forceinline__ uint16_t drop_bf16(uint16_t v, bool keep, float scale) {
  return keep ? f32_to_bf16(bf16_to_f32(v) * scale) : (uint16_t)0;
}

__device__ __forceinline__ uint32_t lane_sample(const DropArgs& a, uint32_t lane) {
  const uint32_t s = a.sample_ptr ? a.sample_ptr[lane] : a.sample + lane;  // BtxRng.sample_idx_dev: one word per lane
  return __builtin_amdgcn_readfirstlane(s);
}

// CH: channel mode on BTX_DROP_CL memory with C % 8 == 0 — the 8 elements at memory offset e (a multiple of 8) are channels
// c0 .. c0 + 7 of one (n, s), so their indices n * C + c0 + j are one aligned Philox group as well
template <bool BF, bool CH>
__global__ __launch_bounds__(DROP_BLOCK) void drop_group_kernel(const DropArgs a) {
  typedef typename std::conditional<BF, uint16_t, float>::type E;
  const uint32_t lane = blockIdx.y;
  const uint32_t smp = lane_sample(a, lane);
  const E* xb = (const E*)a.x + (uint64_t)lane * a.x_stride;
  E* ob = (E*)a.out + (uint64_t)lane * a.n;  // (no __restrict__: out may alias x)
  const uint64_t lo = (uint64_t)blockIdx.x * DROP_CHUNK;
  const uint64_t end = lo + DROP_CHUNK;
  const uint64_t hi = end < a.n ? end : a.n;
  const bool vec = (((uintptr_t)xb | (uintptr_t)ob) & 15) == 0;  // lo is a multiple of 8 elements: the alignment carries over
  const uint64_t SC = a.S * a.C;
  for (uint64_t e = lo + (uint64_t)threadIdx.x * 8; e < hi; e += (uint64_t)DROP_BLOCK * 8) {
    const uint64_t g = CH ? (((e / SC) * a.C + (e % a.C)) >> 3) : (e >> 3);
    const BtxPhilox4 p = btx_philox4x32_10((uint32_t)g, smp, a.layer, BTX_STREAM_DROP, a.k0, a.k1);
    if (vec && e + 8 <= hi) {
      if (BF) {
        u32x4 v = *(const u32x4*)(xb + e);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const uint16_t lo16 = drop_bf16((uint16_t)(v[w] & 0xffffu), (p.x[w] & 0xffffu) < a.T, a.scale);
          const uint16_t hi16 = drop_bf16((uint16_t)(v[w] >> 16), (p.x[w] >> 16) < a.T, a.scale);
          v[w] = (uint32_t)lo16 | ((uint32_t)hi16 << 16);
        }
        *(u32x4*)(ob + e) = v;
      } else {
        f32x4 v0 = *(const f32x4*)(xb + e);
        f32x4 v1 = *(const f32x4*)(xb + e + 4);
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          v0[2 * w] = drop_f32(v0[2 * w], (p.x[w] & 0xffffu) < a.T, a.scale);
          v0[2 * w + 1] = drop_f32(v0[2 * w + 1], (p.x[w] >> 16) < a.T, a.scale);
          v1[2 * w] = drop_f32(v1[2 * w], (p.x[2 + w] & 0xffffu) < a.T, a.scale);
          v1[2 * w + 1] = drop_f32(v1[2 * w + 1], (p.x[2 + w] >> 16) < a.T, a.scale);
        }
        *(f32x4*)(ob + e) = v0;
        *(f32x4*)(ob + e + 4) = v1;
      }
    } else {  // lanes off the 16-byte grid, and the last n % 8 elements of a lane
      E r[8] = {};
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        if (e + j < hi) r[j] = xb[e + j];   // every read of the group before its first write: out may alias x
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        if (e + j < hi) {
          const bool keep = drop_bits(p, j) < a.T;
          if (BF) ob[e + j] = (E)drop_bf16((uint16_t)r[j], keep, a.scale);
          else ob[e + j] = (E)drop_f32((float)r[j], keep, a.scale);
        }
      }
    }
  }
}

// one element per thread per step: m is the element's memory offset inside its lane
template <bool BF>
__global__ __launch_bounds__(DROP_BLOCK) void drop_index_kernel(const DropArgs a, int mode, int layout) {
  typedef typename std::conditional<BF, uint16_t, float>::type E;
  const uint32_t lane = blockIdx.y;
  const uint32_t smp = lane_sample(a, lane);
  const E* xb = (const E*)a.x + (uint64_t)lane * a.x_stride;
  E* ob = (E*)a.out + (uint64_t)lane * a.n;  // (no __restrict__: out may alias x)
  const uint64_t lo = (uint64_t)blockIdx.x * DROP_CHUNK;
  const uint64_t end = lo + DROP_CHUNK;
  const uint64_t hi = end < a.n ? end : a.n;
  for (uint64_t m = lo + threadIdx.x; m < hi; m += DROP_BLOCK) {
    uint64_t n, c, s;
    if (layout == BTX_DROP_CL) {
      const uint64_t t = m / a.C;
      c = m - t * a.C; n = t / a.S; s = t - n * a.S;
    } else {
      const uint64_t t = m / a.S;
      s = m - t * a.S; n = t / a.C; c = t - n * a.C;
    }
    const uint64_t i = mode == BTX_DROP_CHANNEL ? n * a.C + c : (n * a.S + s) * a.C + c;
    const BtxPhilox4 p = btx_philox4x32_10((uint32_t)(i >> 3), smp, a.layer, BTX_STREAM_DROP, a.k0, a.k1);
    const bool keep = drop_bits(p, (uint32_t)i & 7u) < a.T;
    const E v = xb[m];
    if (BF) ob[m] = (E)drop_bf16((uint16_t)v, keep, a.scale);
    else ob[m] = (E)drop_f32((float)v, keep, a.scale);
  }
}

int drop_run(const void* x, void* out, int act_dtype, int64_t N, int64_t C, int64_t S, int mode, int layout, uint32_t T,
             float scale, int lanes, int64_t in_rows, const BtxRng* rng, void* stream) {
  if (!x || !out || !rng) return BTX_E_NULL;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if ((mode != BTX_DROP_ELEMENT && mode != BTX_DROP_CHANNEL) || (layout != BTX_DROP_CL && layout != BTX_DROP_NCS))
    return BTX_E_UNSUPPORTED;
  if (N < 1 || C < 1 || S < 1 || lanes < 1 || T > 65536u) return BTX_E_SHAPE;
  if (lanes > 65535) return BTX_E_UNSUPPORTED;
  const uint64_t MAXE = BTX_DROP_MAX_ELEMENTS;
  if ((uint64_t)N > MAXE || (uint64_t)C > MAXE || (uint64_t)S > MAXE) return BTX_E_UNSUPPORTED;
  if ((uint64_t)S > MAXE / (uint64_t)C) return BTX_E_UNSUPPORTED;  // (S * C would pass 2^64 before it could be compared)
  const uint64_t sc = (uint64_t)S * (uint64_t)C;
  if ((uint64_t)N > MAXE / sc) return BTX_E_UNSUPPORTED;
  const uint64_t n = (uint64_t)N * sc;
  if (in_rows != N && in_rows != (int64_t)lanes * N) return BTX_E_SHAPE;
  const uintptr_t emask = act_dtype == BTX_ACT_BF16 ? 1 : 3;
  if ((((uintptr_t)x | (uintptr_t)out) & emask) || (rng->sample_idx_dev && ((uintptr_t)rng->sample_idx_dev & 3))) return BTX_E_ALIGN;
  DropArgs a;
  a.x = x; a.out = out; a.n = n;
  a.x_stride = (in_rows == (int64_t)lanes * N) ? n : 0;
  a.S = (uint64_t)S; a.C = (uint64_t)C;
  a.T = T; a.scale = scale;
  a.k0 = (uint32_t)rng->seed; a.k1 = (uint32_t)(rng->seed >> 32);
  a.sample = rng->sample_idx; a.layer = rng->layer_id;
  a.sample_ptr = rng->sample_idx_dev;
  const dim3 grid((uint32_t)((n + DROP_CHUNK - 1) / DROP_CHUNK), (uint32_t)lanes);  // <= 2^22 x 65535
  const dim3 block(DROP_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  const bool bf = act_dtype == BTX_ACT_BF16;
  // where memory order and index order agree: BTX_DROP_CL, or a layout with nothing to permute (S == 1 or C == 1)
  const bool in_order = layout == BTX_DROP_CL || S == 1 || C == 1;
  // S == 1: the channel index n * C + c IS the element index
  if ((mode == BTX_DROP_ELEMENT || S == 1) && in_order) {
    if (bf) hipLaunchKernelGGL((drop_group_kernel<true, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((drop_group_kernel<false, false>), grid, block, 0, st, a);
  } else if (mode == BTX_DROP_CHANNEL && layout == BTX_DROP_CL && C % 8 == 0) {
    if (bf) hipLaunchKernelGGL((drop_group_kernel<true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((drop_group_kernel<false, true>), grid, block, 0, st, a);
  } else {
    if (bf) hipLaunchKernelGGL((drop_index_kernel<true>), grid, block, 0, st, a, mode, layout);
    else hipLaunchKernelGGL((drop_index_kernel<false>), grid, block, 0, st, a, mode, layout);
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int btx_dropout_fwd(const void* x, void* out, int act_dtype, int64_t N, int64_t C, int64_t S, int mode, int layout,
                    uint32_t T, float scale, int lanes, int64_t in_rows, const BtxRng* rng, void* stream) {
  return drop_run(x, out, act_dtype, N, C, S, mode, layout, T, scale, lanes, in_rows, rng, stream);
}

int btx_dropout_bwd(const void* dy, void* dx, int act_dtype, int64_t N, int64_t C, int64_t S, int mode, int layout,
                    uint32_t T, float scale, const BtxRng* rng, void* stream) {
  return drop_run(dy, dx, act_dtype, N, C, S, mode, layout, T, scale, 1, N, rng, stream);
}

}  // extern "C"
