// btx_heads.h — what the loss and evaluation heads on a model's output share (btx_calib.hip, btx_mcloss.hip, btx_mceval.hip,
// btx_reg.hip): the 16-byte row access, the wave and workgroup reductions, the layout of the calibration
// workspace and the host-side launch helpers (btx_small.hip takes launch_by_act from here as well).
// Everything but btx::launch_avu_fold is internal to the including unit (anonymous namespace, inlined), so no unit's code object
// depends on another's.
// Contraction: btx_mceval and btx_reg are built with -ffp-contract=off, btx_calib and btx_mcloss pin their arithmetic with
// `#pragma clang fp contract(off)` inside the kernels.  A helper in this header may therefore hold a multiply that feeds an add
// only if its own body carries that pragma; none here does (loads, stores, adds and maxima only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/btx.h"

// ---- the calibration workspace (floats): header, then one record per batch row -------------------------------------------------
// Written by the fold of btx_calib.hip, read by the backward kernels of btx_calib.hip and btx_mcloss.hip.
#define CALIB_K_AREA 21        // thresholds of the area form
#define CALIB_HDR_FLOATS 160   // the header, slots below
#define CALIB_ROW_FLOATS 8     // per-row record: conf, uncertainty, tanh(uncertainty), code, then unit-specific (calib: the row max)
#define CALIB_FOLD_THREADS 1024
#define CALIB_FOLD_WAVES 16

#define HDR_LOSS 0
#define HDR_R 1
#define HDR_DLDR 2      // d loss / d r
#define HDR_K 3         // number of thresholds, as int bits
#define HDR_THA 4       // EaU / EaC: the error threshold the forward used
#define HDR_G 8         // [K][4] d r / d n_q, quadrant q = (good ? 0 : 2) + (certain ? 0 : 1)
#define HDR_TH 96       // [K] thresholds, double (8-byte aligned: 96 * 4 = 384)

namespace btx {
// Launches the one-workgroup AvU fold (calib_fold_kernel<0>, btx_calib.hip) on a workspace whose row records are filled: thresholds
// (one, or the 21 of the area form), quadrant sums in double, out = (loss, r) and the header.  No error is read or cleared.
void launch_avu_fold(int B, int area, float th, const float* th_dev, float beta, float* out, float* ws, hipStream_t st);
}  // namespace btx

namespace {

// ---- V consecutive elements, V = 16 bytes of ACT ---------------------------------------------------------------------------------
template <typename ACT> struct Vw;
template <> struct Vw<float> { static constexpr int V = 4; };
template <> struct Vw<__bf16> { static constexpr int V = 8; };

// V consecutive elements of a row of C from element c0 on: one 16-byte load when `vec` (row + c0 on the 16-byte grid and all V
// inside the row), else element by element with the tail left at 0.  A caller that holds a pointer to the first element passes
// c0 = 0 and C = the number of valid elements.  The bound stays `c0 + j < C`, the form the callers' own tail guards have: written as
// `j < C - c0` the compiler no longer merges the two and the MC-loss kernels come out up to 8 % slower.
template <typename ACT>
__device__ __forceinline__ void load_v(const ACT* __restrict__ row, int c0, int C, bool vec, float* v) {
  constexpr int V = Vw<ACT>::V;
  if (vec) {
    if constexpr (sizeof(ACT) == 4) {
      const float4 q = *reinterpret_cast<const float4*>(row + c0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      const uint4 q = *reinterpret_cast<const uint4*>(row + c0);
      const unsigned int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[2 * j] = __uint_as_float(w[j] << 16);
        v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = (c0 + j < C) ? (float)row[c0 + j] : 0.f;
  }
}

template <typename ACT>
__device__ __forceinline__ void store_v(ACT* __restrict__ row, int c0, int C, bool vec, const float* v) {
  constexpr int V = Vw<ACT>::V;
  if (vec) {
    if constexpr (sizeof(ACT) == 4) {
      *reinterpret_cast<float4*>(row + c0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      union { uint4 q; __bf16 h[8]; } u;
#pragma unroll
      for (int j = 0; j < 8; ++j) u.h[j] = (__bf16)v[j];
      *reinterpret_cast<uint4*>(row + c0) = u.q;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (c0 + j < C) row[c0 + j] = (ACT)v[j];
  }
}

// ---- inside a wave: a xor butterfly; both partners combine the same two numbers, so all 64 lanes hold the same bits ---------------
template <typename T>  // float, double or int
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- over a workgroup of 256 threads (four waves).  The shapes differ and the names say which: do not merge them. ----------------
// f32, the four wave partials added in index order, ((w0 + w1) + w2) + w3; every thread returns the same bits.  `red`: 4 floats of LDS.
__device__ __forceinline__ float block_sum_inorder4(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) t += red[w];
  return t;
}
__device__ __forceinline__ float block_max_inorder4(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) t = fmaxf(t, red[w]);
  return t;
}
// f64, pairwise (w0 + w1) + (w2 + w3); valid in thread 0.  `part`: 4 doubles of LDS.
__device__ __forceinline__ double block_sum_pairwise4(double v, double* part) {
  v = wave_sum(v);
  __syncthreads();  // part may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// bytes per element behind a BTX_ACT_* code; 0: not an activation dtype (the caller returns BTX_E_DTYPE)
inline int act_esize(int dtype) { return dtype == BTX_ACT_F32 ? 4 : dtype == BTX_ACT_BF16 ? 2 : 0; }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// rows of n elements from p on all start on the 16-byte grid and hold whole 16-byte vectors
inline bool on_grid(const void* p, int n, int esize) { return aligned16(p) && (n % (16 / esize)) == 0; }

// launches through f(T()), T the element type behind a BTX_ACT_* code
template <typename F>
inline int launch_by_act(int dtype, F f) {
  if (dtype == BTX_ACT_BF16) f((__bf16)0.f);
  else if (dtype == BTX_ACT_F32) f(0.f);
  else return BTX_E_DTYPE;
  return (int)hipGetLastError();
}

}  // namespace
