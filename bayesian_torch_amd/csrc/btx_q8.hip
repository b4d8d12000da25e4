// K10: INT8 inference (BTX-Q8 v1) for Linear / Conv2d Reparameterization layers.
// Reference op chain (CPU quantized engines): layers/variational_layers/quantize_linear_variational.py:134-224 and
// quantize_conv_variational.py:457-552 — quantize eps, quantized.mul, quantized.add, quantized linear / conv2d.
//
// Three kernels:
//   q8_quantize_act_kernel   f32 / bf16 activations of any 4-D strides -> uint8 channels-last
//   q8_sample_kernel         one launch per layer: eps -> eps_i -> d_i -> W_i (int8, [N][Kp], k = tap * Cp + c, Cp = C rounded up
//                            to 16, Kp = taps * Cp rounded up to 64, padding zero), the row sums S_n and the int32 bias b_i
//   q8_contract_kernel       implicit GEMM on v_mfma_i32_16x16x64_i8.  Activations stay uint8 in memory and become x - 128 (int8)
//                            with one xor on the way into LDS; the epilogue adds (128 - z_x) * S_n, which makes every input zero
//                            point exact on the signed x signed instruction; out-of-image taps and the K tail hold the byte z_x
//                            (value 0 after the correction; the tail meets zero weights).
//
// Network ops (§13 "between the layers"): q8_add_kernel (two uint8 tensors -> one, requantized), the same add as the residual
// epilogue of the contraction (q8_contract_kernel<true>), q8_maxpool_cl_kernel and q8_avgpool_cl_kernel on uint8 channels-last.
//
// Numerics: every floating step is ONE f32 operation, round to nearest even, never contracted (__fmul_rn / __fadd_rn, and this unit is
// built with -ffp-contract=off); rintf is half-to-even.  The integer sums are exact, so their order does not matter.
//
// The MFMA computes D^T = W * X^T: the weight tile is the A operand (row = output channel), the activation tile the B operand
// (column = output pixel).  A lane then owns 4 CONSECUTIVE output channels of one pixel (C/D map: col = lane & 15,
// row = 4 * (lane >> 4) + reg), i.e. one 4-byte (uint8) or 16-byte (f32) store.  Both operands are read with the same
// (lane >> 4, byte) -> k map (16 consecutive k per lane), so the product does not depend on how the instruction orders k inside a step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/btx.h"
#include "btx_rng.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int Q8_BM = 64;     // output pixels per workgroup
constexpr int Q8_BN = 64;     // output channels per workgroup
constexpr int Q8_BK = 64;     // one MFMA K step
constexpr int Q8_LDS_ROW = 80;  // 64 bytes of k + 16 of padding: 16-byte aligned rows that do not all start in one bank

__device__ __forceinline__ float q8_round_clamp(float v, float inv_s, float z, float lo, float hi) {
  return fminf(fmaxf(__fadd_rn(rintf(__fmul_rn(v, inv_s)), z), lo), hi);
}

// ---------------------------------------------------------------------------------------------------------------------
// activation quantize
// ---------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float q8_ldf(const T* p);
template <> __device__ __forceinline__ float q8_ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float q8_ldf<uint16_t>(const uint16_t* p) { return __uint_as_float((uint32_t)(*p) << 16); }

template <typename T>
__global__ __launch_bounds__(256) void q8_quantize_act_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, int C, int H, int W,
                                                              long long sn, long long sc, long long sh, long long sw, size_t total,
                                                              float inv_s, float zp) {
  // one thread per 4 consecutive output bytes (channels-last order); total is the element count
  const size_t ngrp = (total + 3) >> 2;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * 256) {
    uint32_t pack = 0;
    const size_t base = g << 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t i = base + e;
      if (i < total) {
        const int c = (int)(i % (size_t)C);
        size_t p = i / (size_t)C;
        const int w = (int)(p % (size_t)W); p /= (size_t)W;
        const int h = (int)(p % (size_t)H);
        const size_t n = p / (size_t)H;
        const float v = q8_ldf<T>(x + (long long)n * sn + (long long)c * sc + (long long)h * sh + (long long)w * sw);
        pack |= (uint32_t)(int)q8_round_clamp(v, inv_s, zp, 0.0f, 255.0f) << (8 * e);
      }
    }
    if (base + 4 <= total) {
      *reinterpret_cast<uint32_t*>(out + base) = pack;
    } else {
      for (int e = 0; base + e < total; ++e) out[base + e] = (uint8_t)(pack >> (8 * e));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight sampling pre-pass: one workgroup per output channel
// ---------------------------------------------------------------------------------------------------------------------
struct Q8SampleArgs {
  const int8_t* mu_i; const int8_t* sigma_i;   // [N][taps][C]
  const float* mu_b; const float* sigma_b;     // [N] or NULL
  const float* eps_w; const float* eps_b;      // explicit noise ([N][taps][C] / [N]) or NULL -> BTX-RNG v1
  int8_t* W; int32_t* S; int32_t* b_i;
  int N, taps, C, eps_C, Cp, Kp;
  BtxQ8Chain ch;
  uint32_t k0, k1, sample, layer;
  const uint32_t* sample_ptr;
};

__global__ __launch_bounds__(256) void q8_sample_kernel(const Q8SampleArgs a) {
  __shared__ int red[256];
  uint32_t sample = a.sample;
  if (a.sample_ptr) sample = __builtin_amdgcn_readfirstlane(*a.sample_ptr);  // BtxRng.sample_idx_dev (captured graphs)
  const int n = blockIdx.x;
  const int8_t* mu = a.mu_i + (size_t)n * a.taps * a.C;
  const int8_t* sg = a.sigma_i + (size_t)n * a.taps * a.C;
  int8_t* wrow = a.W + (size_t)n * a.Kp;
  int sum = 0;
  for (int p = threadIdx.x * 4; p < a.Kp; p += 256 * 4) {  // 4 consecutive k per thread: one Philox block, one 4-byte store
    const int tap = p / a.Cp, c0 = p - tap * a.Cp;
    uint32_t pack = 0;
    if (tap < a.taps && c0 < a.C) {
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!a.eps_w)  // the float layer's index space: [N][taps][eps_C], eps_C a multiple of 8 -> c0 .. c0+3 share a block
        btx_normal4((uint32_t)((((size_t)n * a.taps + tap) * a.eps_C + c0) >> 2), sample, a.layer, BTX_STREAM_EPS_W, a.k0, a.k1, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + e;
        if (c < a.C) {
          const size_t src = (size_t)tap * a.C + c;
          const float eps = a.eps_w ? a.eps_w[(size_t)n * a.taps * a.C + src] : z[e];
          const float eps_i = q8_round_clamp(eps, a.ch.inv_s_eps, 0.0f, -128.0f, 127.0f);
          const float t = __fmul_rn(__fmul_rn((float)sg[src], a.ch.s_sigma), __fmul_rn(eps_i, a.ch.s_eps));
          const float d_i = q8_round_clamp(t, a.ch.inv_s_d, 0.0f, -128.0f, 127.0f);
          const float u = __fadd_rn(__fmul_rn(d_i, a.ch.s_d), __fmul_rn((float)mu[src], a.ch.s_mu));
          const int w = (int)q8_round_clamp(u, a.ch.inv_s_w, 0.0f, -128.0f, 127.0f);
          sum += w;
          pack |= ((uint32_t)w & 0xffu) << (8 * e);
        }
      }
    }
    *reinterpret_cast<uint32_t*>(wrow + p) = pack;  // padding (c >= C, k >= taps * Cp) is written as zero
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.S[n] = red[0];
    int bi = 0;
    if (a.mu_b) {
      float b = a.mu_b[n];
      if (a.sigma_b) {
        const float eb = a.eps_b ? a.eps_b[n] : btx_normal1((uint64_t)n, sample, a.layer, BTX_STREAM_EPS_B, a.k0, a.k1);
        b = __fadd_rn(b, __fmul_rn(a.sigma_b[n], eb));
      }
      bi = (int)rint((double)b / a.ch.bias_div);
    }
    a.b_i[n] = bi;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// i8 implicit GEMM
// ---------------------------------------------------------------------------------------------------------------------
struct Q8ContractArgs {
  const uint8_t* x; const int8_t* W; const int32_t* S; const int32_t* b_i; void* out;
  int NB, H, Wd, C, N, KH, KW, sh, sw, ph, pw, dh, dw, OH, OW;
  int Cp, Kp, taps;
  long long M;        // NB * OH * OW
  int z_x, z_o, lo;   // lo: lower clamp (z_o with ReLU, else 0)
  float mult, s_o;
  int out_f32, x_vec, out_vec;
};

// the add of two quantized tensors: da = fma(s_a, a, pre_a), pre_a = f32(s_a * f32(-z_a)) (torch's vector kernel dequantizes with one
// fused multiply-add), db alike, o = clamp(rint((da + db) * inv_s) + z, lo, 255)
struct Q8AddArgs {
  float s_a, pre_a, s_b, pre_b, inv_s, z, lo;
};

__device__ __forceinline__ float q8_add1(float a, float b, const Q8AddArgs& p) {
  const float da = __fmaf_rn(p.s_a, a, p.pre_a);
  const float db = __fmaf_rn(p.s_b, b, p.pre_b);
  return fminf(fmaxf(__fadd_rn(rintf(__fmul_rn(__fadd_rn(da, db), p.inv_s)), p.z), p.lo), 255.0f);
}

// the residual operand of q8_contract_kernel<true>: uint8 [M][N] like the output; res_vec: 4-byte loads are in range and aligned
struct Q8ResArgs {
  const uint8_t* res;
  Q8AddArgs add;
  int res_vec;
};

// RES: the epilogue adds a residual tensor to the requantized output (a = the conv's output at (s_o, z_o), b = the residual) and
// stores the sum's uint8.  RES = false never touches `ra`.
template <bool RES>
__global__ __launch_bounds__(256) void q8_contract_kernel(const Q8ContractArgs a, const Q8ResArgs ra) {
  // two stages of each tile: step i + 1 is written while slower waves still read step i, so one barrier per step is enough (the
  // write of step i + 2 into this stage comes after barrier i + 1, which every wave reaches only after its reads of step i)
  __shared__ __attribute__((aligned(16))) uint8_t lds_w[2][Q8_BN * Q8_LDS_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t lds_x[2][Q8_BM * Q8_LDS_ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * Q8_BM;
  const int n0 = blockIdx.y * Q8_BN;

  // the 16-byte chunk of each tile this thread stages: row = tid / 4, bytes [16 * (tid & 3), +16)
  const int lrow = tid >> 2, lq = tid & 3;
  const long long lm = m0 + lrow;
  const bool m_ok = lm < a.M;
  int img = 0, ih0 = 0, iw0 = 0;
  if (m_ok) {
    const int ow = (int)(lm % a.OW);
    const long long t = lm / a.OW;
    const int oh = (int)(t % a.OH);
    img = (int)(t / a.OH);
    ih0 = oh * a.sh - a.ph;
    iw0 = ow * a.sw - a.pw;
  }
  const int ln = n0 + lrow;
  const uint32_t zfill = (uint32_t)(a.z_x & 0xff) * 0x01010101u;

  v4i acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (v4i){0, 0, 0, 0};

  // one K step's 16-byte chunks of this thread: the weight chunk (rows of W are Kp bytes, 16-byte aligned; rows >= N read as zero) and
  // the activation chunk (k = tap * Cp + c; a chunk lies inside one tap because Cp is a multiple of 16), already xor-ed to int8
  auto load_chunks = [&](int k0, uint4& wv, uint4& xv) {
    wv = make_uint4(0u, 0u, 0u, 0u);
    if (ln < a.N) wv = *reinterpret_cast<const uint4*>(a.W + (size_t)ln * a.Kp + k0 + 16 * lq);
    xv = make_uint4(zfill, zfill, zfill, zfill);
    const int k = k0 + 16 * lq;
    const int tap = k / a.Cp, c0 = k - tap * a.Cp;
    if (m_ok && tap < a.taps && c0 < a.C) {
      const int kh = tap / a.KW, kw = tap - kh * a.KW;
      const int ih = ih0 + kh * a.dh, iw = iw0 + kw * a.dw;
      if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.Wd) {
        const uint8_t* src = a.x + (((size_t)img * a.H + ih) * a.Wd + iw) * a.C + c0;
        if (a.x_vec) {  // C % 16 == 0 and a 16-byte aligned base: the whole chunk is in range and aligned
          xv = *reinterpret_cast<const uint4*>(src);
        } else {
          uint32_t wds[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t wd = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = c0 + 4 * q + e;
              const uint32_t byte = (c < a.C) ? (uint32_t)src[4 * q + e] : (uint32_t)(a.z_x & 0xff);
              wd |= byte << (8 * e);
            }
            wds[q] = wd;
          }
          xv = make_uint4(wds[0], wds[1], wds[2], wds[3]);
        }
      }
    }
    xv.x ^= 0x80808080u; xv.y ^= 0x80808080u; xv.z ^= 0x80808080u; xv.w ^= 0x80808080u;  // uint8 x -> int8 (x - 128)
  };

  uint4 wv, xv;
  load_chunks(0, wv, xv);
  int stage = 0;
  for (int k0 = 0; k0 < a.Kp; k0 += Q8_BK, stage ^= 1) {
    const uint8_t* sw = lds_w[stage];
    const uint8_t* sx = lds_x[stage];
    *reinterpret_cast<uint4*>(lds_w[stage] + lrow * Q8_LDS_ROW + 16 * lq) = wv;
    *reinterpret_cast<uint4*>(lds_x[stage] + lrow * Q8_LDS_ROW + 16 * lq) = xv;
    __syncthreads();
    if (k0 + Q8_BK < a.Kp) load_chunks(k0 + Q8_BK, wv, xv);  // the next step's global loads fly under this step's MFMAs
    // ---- wave `wave` owns pixels [16 * wave, +16) and all 64 channels: 4 MFMAs per step
    const v4i xf = *reinterpret_cast<const v4i*>(sx + (16 * wave + (lane & 15)) * Q8_LDS_ROW + 16 * (lane >> 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const v4i wf = *reinterpret_cast<const v4i*>(sw + (16 * j + (lane & 15)) * Q8_LDS_ROW + 16 * (lane >> 4));
      acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, xf, acc[j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds channels n = n0 + 16 j + 4 (lane >> 4) + r of pixel m = m0 + 16 wave + (lane & 15)
  const long long m = m0 + 16 * wave + (lane & 15);
  if (m >= a.M) return;
  const int zc = 128 - a.z_x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nb = n0 + 16 * j + 4 * (lane >> 4);
    if (nb >= a.N) continue;
    float of[4];
    uint32_t pack = 0;
    const size_t off = (size_t)m * a.N + nb;
    uint32_t rpack = 0;
    if (RES) {  // the residual's four bytes of this lane, at the offset of its own four outputs
      const uint8_t* rp = ra.res + off;
      if (ra.res_vec && nb + 4 <= a.N) {
        rpack = *reinterpret_cast<const uint32_t*>(rp);
      } else {
        for (int r = 0; r < 4 && nb + r < a.N; ++r) rpack |= (uint32_t)rp[r] << (8 * r);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nb + r;
      float o = 0.0f;
      if (n < a.N) {
        const int v = acc[j][r] + zc * a.S[n] + a.b_i[n];
        o = fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)v, a.mult)), (float)a.z_o), (float)a.lo), 255.0f);
        if (RES) o = q8_add1(o, (float)((rpack >> (8 * r)) & 0xffu), ra.add);
      }
      pack |= (uint32_t)(int)o << (8 * r);
      of[r] = __fmul_rn(o - (float)a.z_o, a.s_o);  // o and z_o are small integers: the difference is exact
    }
    if (a.out_f32) {
      float* o = reinterpret_cast<float*>(a.out) + off;
      if (a.out_vec && nb + 4 <= a.N) {
        *reinterpret_cast<float4*>(o) = make_float4(of[0], of[1], of[2], of[3]);
      } else {
        for (int r = 0; r < 4 && nb + r < a.N; ++r) o[r] = of[r];
      }
    } else {
      uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + off;
      if (a.out_vec && nb + 4 <= a.N) {
        *reinterpret_cast<uint32_t*>(o) = pack;
      } else {
        for (int r = 0; r < 4 && nb + r < a.N; ++r) o[r] = (uint8_t)(pack >> (8 * r));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Flipout (DESIGN.md §13 "Flipout"): the delta pre-pass and the two-GEMM contraction
// ---------------------------------------------------------------------------------------------------------------------
// quantized.mul of two quantized values: c = (a - z_a) * (b - z_b) in int32 (formed by the caller),
// o = clamp(rint(f32(c) * m) + z_o, lo, hi), m = f32(f32(s_a) * f32(s_b)) * (f32(1) / f32(s_o)) computed once on the host
__device__ __forceinline__ float q8_mul1(int c, float m, float z, float lo, float hi) {
  return fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)c, m)), z), lo), hi);
}

struct Q8DeltaArgs {
  const int8_t* sigma_i;                       // [N][taps][C]
  const float* mu_b; const float* sigma_b;     // [N] or NULL
  const float* eps_w; const float* eps_b;      // explicit noise or NULL -> BTX-RNG v1
  int8_t* D; int32_t* S; int32_t* bm_i; int32_t* bp_i;
  int N, taps, C, eps_C, Cp, Kp;
  int mean_bias, pert_bias;                    // BTX_Q8_BIAS_*
  float inv_s_eps, mult;
  double div_mean, div_pert;
  uint32_t k0, k1, sample, layer;
  const uint32_t* sample_ptr;
};

__global__ __launch_bounds__(256) void q8_delta_kernel(const Q8DeltaArgs a) {
  __shared__ int red[256];
  uint32_t sample = a.sample;
  if (a.sample_ptr) sample = __builtin_amdgcn_readfirstlane(*a.sample_ptr);
  const int n = blockIdx.x;
  const int8_t* sg = a.sigma_i + (size_t)n * a.taps * a.C;
  int8_t* drow = a.D + (size_t)n * a.Kp;
  int sum = 0;
  for (int p = threadIdx.x * 4; p < a.Kp; p += 256 * 4) {
    const int tap = p / a.Cp, c0 = p - tap * a.Cp;
    uint32_t pack = 0;
    if (tap < a.taps && c0 < a.C) {
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!a.eps_w)
        btx_normal4((uint32_t)((((size_t)n * a.taps + tap) * a.eps_C + c0) >> 2), sample, a.layer, BTX_STREAM_EPS_W, a.k0, a.k1, z);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + e;
        if (c < a.C) {
          const size_t src = (size_t)tap * a.C + c;
          const float eps = a.eps_w ? a.eps_w[(size_t)n * a.taps * a.C + src] : z[e];
          const int eps_i = (int)q8_round_clamp(eps, a.inv_s_eps, 0.0f, -128.0f, 127.0f);
          const int d = (int)q8_mul1((int)sg[src] * eps_i, a.mult, 0.0f, -128.0f, 127.0f);
          sum += d;
          pack |= ((uint32_t)d & 0xffu) << (8 * e);
        }
      }
    }
    *reinterpret_cast<uint32_t*>(drow + p) = pack;
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.S[n] = red[0];
    float bs = 0.0f;
    if (a.mean_bias == BTX_Q8_BIAS_SIGMA_EPS || a.pert_bias == BTX_Q8_BIAS_SIGMA_EPS) {
      const float eb = a.eps_b ? a.eps_b[n] : btx_normal1((uint64_t)n, sample, a.layer, BTX_STREAM_EPS_B, a.k0, a.k1);
      bs = __fmul_rn(a.sigma_b[n], eb);
    }
    const float bm = a.mean_bias == BTX_Q8_BIAS_MU ? a.mu_b[n] : bs, bp = a.pert_bias == BTX_Q8_BIAS_MU ? a.mu_b[n] : bs;
    a.bm_i[n] = a.mean_bias == BTX_Q8_BIAS_NONE ? 0 : (int)rint((double)bm / a.div_mean);
    a.bp_i[n] = a.pert_bias == BTX_Q8_BIAS_NONE ? 0 : (int)rint((double)bp / a.div_pert);
  }
}

struct Q8FlipArgs {
  const uint8_t* x; const int8_t* Wm; const int8_t* D;
  const int32_t* Sm; const int32_t* Sd; const int32_t* bm_i; const int32_t* bp_i;
  const int8_t* sign_in; const int8_t* sign_out;   // explicit +1 / -1 (channels-last like x / out) or NULL -> BTX-RNG v1
  void* out;
  int NB, H, Wd, C, N, KH, KW, sh, sw, ph, pw, dh, dw, OH, OW;
  int Cp, Kp, taps, sign_C;
  long long M;
  BtxQ8Flipout f;
  Q8AddArgs add;
  int out_f32, x_vec, out_vec;
  uint32_t k0, k1, sample, layer;
  const uint32_t* sample_ptr;
};

__global__ __launch_bounds__(256) void q8_flipout_kernel(const Q8FlipArgs a) {
  // q8_contract_kernel's tiling and staging with four tiles per step: W_mu, D, x, x'
  __shared__ __attribute__((aligned(16))) uint8_t lds_w[2][Q8_BN * Q8_LDS_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t lds_d[2][Q8_BN * Q8_LDS_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t lds_x[2][Q8_BM * Q8_LDS_ROW];
  __shared__ __attribute__((aligned(16))) uint8_t lds_p[2][Q8_BM * Q8_LDS_ROW];
  // x' (as int8: xor 0x80) for every (sign, x byte): 512 entries kept in the 16 padding bytes of the first 32 rows of lds_w[0], which
  // the staging never writes (a 513th LDS KB would cost the fourth workgroup per CU)
  auto lut = [&](uint32_t i) -> uint8_t& { return lds_w[0][(i >> 4) * Q8_LDS_ROW + 64 + (i & 15u)]; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * Q8_BM;
  const int n0 = blockIdx.y * Q8_BN;

  uint32_t kin_a = 0, kin_b = 0, kout_a = 0, kout_b = 0;
  if (!a.sign_in || !a.sign_out) {  // the sign keys of this sample (BtxRng.sample_idx_dev: resolved here, at run time)
    uint32_t sample = a.sample;
    if (a.sample_ptr) sample = __builtin_amdgcn_readfirstlane(*a.sample_ptr);
    const BtxPhilox4 ki = btx_philox4x32_10(0u, sample, a.layer, BTX_STREAM_SIGN_IN, a.k0, a.k1);
    const BtxPhilox4 ko = btx_philox4x32_10(0u, sample, a.layer, BTX_STREAM_SIGN_OUT, a.k0, a.k1);
    kin_a = __builtin_amdgcn_readfirstlane(ki.x[0]); kin_b = __builtin_amdgcn_readfirstlane(ki.x[1]);
    kout_a = __builtin_amdgcn_readfirstlane(ko.x[0]); kout_b = __builtin_amdgcn_readfirstlane(ko.x[1]);
  }

  const int lrow = tid >> 2, lq = tid & 3;
  const long long lm = m0 + lrow;
  const bool m_ok = lm < a.M;
  int img = 0, ih0 = 0, iw0 = 0;
  if (m_ok) {
    const int ow = (int)(lm % a.OW);
    const long long t = lm / a.OW;
    const int oh = (int)(t % a.OH);
    img = (int)(t / a.OH);
    ih0 = oh * a.sh - a.ph;
    iw0 = ow * a.sw - a.pw;
  }
  const int ln = n0 + lrow;
  const uint32_t zfill = (uint32_t)(a.f.z_x & 0xff) * 0x01010101u;
  const uint32_t pfill = ((uint32_t)(a.f.z_xp & 0xff) * 0x01010101u) ^ 0x80808080u;   // the x' tile is staged as int8
  const float zp6 = (float)a.f.z_xp;
  lut((uint32_t)tid) = (uint8_t)((int)q8_mul1((tid - a.f.z_x) * a.f.sin_pos, a.f.mult_xp, zp6, 0.0f, 255.0f) ^ 0x80);
  lut(256u + (uint32_t)tid) = (uint8_t)((int)q8_mul1((tid - a.f.z_x) * a.f.sin_neg, a.f.mult_xp, zp6, 0.0f, 255.0f) ^ 0x80);
  __syncthreads();

  v4i acc[4], accd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { acc[j] = (v4i){0, 0, 0, 0}; accd[j] = (v4i){0, 0, 0, 0}; }

  // one K step's four 16-byte chunks of this thread.  x' is formed here from the loaded x bytes and the element's sign: the sign of
  // element (pixel, c) does not depend on the tap that reads it, so every tap sees the same x' as a materialised tensor would give
  auto load_chunks = [&](int k0, uint4& wv, uint4& dv, uint4& xv, uint4& pv) {
    wv = make_uint4(0u, 0u, 0u, 0u);
    dv = make_uint4(0u, 0u, 0u, 0u);
    if (ln < a.N) {
      wv = *reinterpret_cast<const uint4*>(a.Wm + (size_t)ln * a.Kp + k0 + 16 * lq);
      dv = *reinterpret_cast<const uint4*>(a.D + (size_t)ln * a.Kp + k0 + 16 * lq);
    }
    xv = make_uint4(zfill, zfill, zfill, zfill);
    pv = make_uint4(pfill, pfill, pfill, pfill);
    const int k = k0 + 16 * lq;
    const int tap = k / a.Cp, c0 = k - tap * a.Cp;
    if (m_ok && tap < a.taps && c0 < a.C) {
      const int kh = tap / a.KW, kw = tap - kh * a.KW;
      const int ih = ih0 + kh * a.dh, iw = iw0 + kw * a.dw;
      if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.Wd) {
        const size_t pix = ((size_t)img * a.H + ih) * a.Wd + iw;
        const uint8_t* src = a.x + pix * a.C + c0;
        uint32_t xs[4];
        if (a.x_vec) {
          const uint4 v = *reinterpret_cast<const uint4*>(src);
          xs[0] = v.x; xs[1] = v.y; xs[2] = v.z; xs[3] = v.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t wd = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = c0 + 4 * q + e;
              const uint32_t byte = (c < a.C) ? (uint32_t)src[4 * q + e] : (uint32_t)(a.f.z_x & 0xff);
              wd |= byte << (8 * e);
            }
            xs[q] = wd;
          }
        }
        xv = make_uint4(xs[0], xs[1], xs[2], xs[3]);
        // 16 sign bits, bit e = 1 for a negative sign of channel c0 + e
        uint32_t neg = 0;
        if (a.sign_in) {
          const int8_t* sp = a.sign_in + pix * a.C + c0;
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (c0 + e < a.C && sp[e] < 0) neg |= 1u << e;
        } else {
          // the float layer's index space: rows of sign_C channels.  sign_C and c0 are multiples of 8, so the chunk is two aligned
          // groups of 8 signs; group g of a 32-sign word keeps its even elements in bits 15 - 4g .. 12 - 4g and its odd ones in
          // bits 31 - 4g .. 28 - 4g, first element highest (btx_sign_bitpos)
          const unsigned long long i0 = (unsigned long long)pix * (unsigned)a.sign_C + (unsigned)c0;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned long long i = i0 + 8u * h;
            const uint32_t w = btx_sign_word((uint32_t)(i >> 5), kin_a, kin_b);
            const int g4 = 4 * (int)(((uint32_t)i & 31u) >> 3);
            const uint32_t ev = (w >> (12 - g4)) & 0xfu, od = (w >> (28 - g4)) & 0xfu;
#pragma unroll
            for (int j = 0; j < 8; ++j) neg |= ((((j & 1) ? od : ev) >> (3 - (j >> 1))) & 1u) << (8 * h + j);
          }
        }
        // x' = mul(x, sign byte) depends on the x byte and the sign only: one of 512 table entries (already xor-ed to int8).
        // Channels >= C of a chunk meet zero weights in D, so whatever byte they get contributes nothing.
        uint32_t ps[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t wd = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t idx = ((xs[q] >> (8 * e)) & 0xffu) | (((neg >> (4 * q + e)) & 1u) << 8);
            wd |= (uint32_t)lut(idx) << (8 * e);
          }
          ps[q] = wd;
        }
        pv = make_uint4(ps[0], ps[1], ps[2], ps[3]);
      }
    }
    xv.x ^= 0x80808080u; xv.y ^= 0x80808080u; xv.z ^= 0x80808080u; xv.w ^= 0x80808080u;   // pv is int8 already
  };

  uint4 wv, dv, xv, pv;
  load_chunks(0, wv, dv, xv, pv);
  int stage = 0;
  for (int k0 = 0; k0 < a.Kp; k0 += Q8_BK, stage ^= 1) {
    const int so = lrow * Q8_LDS_ROW + 16 * lq;
    *reinterpret_cast<uint4*>(lds_w[stage] + so) = wv;
    *reinterpret_cast<uint4*>(lds_d[stage] + so) = dv;
    *reinterpret_cast<uint4*>(lds_x[stage] + so) = xv;
    *reinterpret_cast<uint4*>(lds_p[stage] + so) = pv;
    __syncthreads();
    if (k0 + Q8_BK < a.Kp) load_chunks(k0 + Q8_BK, wv, dv, xv, pv);
    const int xo = (16 * wave + (lane & 15)) * Q8_LDS_ROW + 16 * (lane >> 4);
    const v4i xf = *reinterpret_cast<const v4i*>(lds_x[stage] + xo);
    const v4i pf = *reinterpret_cast<const v4i*>(lds_p[stage] + xo);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int wo = (16 * j + (lane & 15)) * Q8_LDS_ROW + 16 * (lane >> 4);
      const v4i wf = *reinterpret_cast<const v4i*>(lds_w[stage] + wo);
      const v4i df = *reinterpret_cast<const v4i*>(lds_d[stage] + wo);
      acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, xf, acc[j], 0, 0, 0);
      accd[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(df, pf, accd[j], 0, 0, 0);
    }
  }

  // ---- store: requantize both accumulators, sign-multiply the perturbation, add, clamp
  const long long m = m0 + 16 * wave + (lane & 15);
  if (m >= a.M) return;
  const int zc = 128 - a.f.z_x, zcp = 128 - a.f.z_xp;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nb = n0 + 16 * j + 4 * (lane >> 4);
    if (nb >= a.N) continue;
    float of[4];
    uint32_t pack = 0;
    const size_t off = (size_t)m * a.N + nb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nb + r;
      float o = 0.0f;
      if (n < a.N) {
        const int v1 = acc[j][r] + zc * a.Sm[n] + a.bm_i[n];
        const float o1 = fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)v1, a.f.mult_mean)), (float)a.f.z_mean), 0.0f), 255.0f);
        const int v2 = accd[j][r] + zcp * a.Sd[n] + a.bp_i[n];
        const float p = fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)v2, a.f.mult_pert)), (float)a.f.z_pert), 0.0f), 255.0f);
        bool negs;
        if (a.sign_out) {
          negs = a.sign_out[off + r] < 0;
        } else {
          const unsigned long long io = (unsigned long long)(off + r);
          const uint32_t w = btx_sign_word((uint32_t)(io >> 5), kout_a, kout_b);
          negs = ((w >> btx_sign_bitpos((uint32_t)io & 31u)) & 1u) != 0;
        }
        const float p2 = q8_mul1(((int)p - a.f.z_pert) * (negs ? a.f.sout_neg : a.f.sout_pos), a.f.mult_p2, (float)a.f.z_p2, 0.0f, 255.0f);
        o = q8_add1(o1, p2, a.add);
      }
      pack |= (uint32_t)(int)o << (8 * r);
      of[r] = __fmul_rn(o - a.add.z, a.f.out_scale);
    }
    if (a.out_f32) {
      float* o = reinterpret_cast<float*>(a.out) + off;
      if (a.out_vec && nb + 4 <= a.N) {
        *reinterpret_cast<float4*>(o) = make_float4(of[0], of[1], of[2], of[3]);
      } else {
        for (int r = 0; r < 4 && nb + r < a.N; ++r) o[r] = of[r];
      }
    } else {
      uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + off;
      if (a.out_vec && nb + 4 <= a.N) {
        *reinterpret_cast<uint32_t*>(o) = pack;
      } else {
        for (int r = 0; r < 4 && nb + r < a.N; ++r) o[r] = (uint8_t)(pack >> (8 * r));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// between the layers: add, max-pool, avg-pool on uint8
// ---------------------------------------------------------------------------------------------------------------------
// one thread per 16 consecutive bytes; vec: the three bases are 16-byte aligned.  The last group (n % 16 bytes) and every group of
// an unaligned call go byte by byte.
__global__ __launch_bounds__(256) void q8_add_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                     uint8_t* __restrict__ out, size_t n, const Q8AddArgs p, int vec) {
  const size_t ngrp = (n + 15) >> 4;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngrp; g += (size_t)gridDim.x * 256) {
    const size_t base = g << 4;
    if (vec && base + 16 <= n) {
      const uint4 va = *reinterpret_cast<const uint4*>(a + base);
      const uint4 vb = *reinterpret_cast<const uint4*>(b + base);
      const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
      uint32_t wo[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t pack = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pack |= (uint32_t)(int)q8_add1((float)((wa[q] >> (8 * e)) & 0xffu), (float)((wb[q] >> (8 * e)) & 0xffu), p) << (8 * e);
        wo[q] = pack;
      }
      *reinterpret_cast<uint4*>(out + base) = make_uint4(wo[0], wo[1], wo[2], wo[3]);
    } else {
      for (size_t i = base; i < base + 16 && i < n; ++i) out[i] = (uint8_t)(int)q8_add1((float)a[i], (float)b[i], p);
    }
  }
}

// Channels-last pooling, window and grid conventions of maxpool2d_cl_kernel (btx_small.hip): one thread per VEC channels of one
// output pixel, grid-stride over `total` = NB * Ho * Wo * (C / VEC).  VEC = 16: one 16-byte load per window element (C % 16 == 0,
// aligned bases); VEC = 1: bytewise.  AVG: no padding, the window is always whole (cnt = k * k).
template <int VEC, bool AVG>
__global__ __launch_bounds__(256) void q8_pool_cl_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ out, int NB, int H, int W,
                                                         int C, int Ho, int Wo, int k, int s, int pad, long long total, int zcnt,
                                                         float rcp, float z) {
  const int cgs = C / VEC;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % cgs);
    long long r = t / cgs;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    int m[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) m[j] = 0;
    for (int kh = 0; kh < k; ++kh) {
      const int h = ho * s - pad + kh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int w = wo * s - pad + kw;
        if ((unsigned)w >= (unsigned)W) continue;
        const uint8_t* src = x + (((long long)n * H + h) * W + w) * C + (long long)cg * VEC;
        if (VEC == 16) {
          const uint4 v = *reinterpret_cast<const uint4*>(src);
          const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const int e = (int)((wd[j >> 2] >> (8 * (j & 3))) & 0xffu);
            m[j] = AVG ? m[j] + e : max(m[j], e);
          }
        } else {
          const int e = (int)src[0];
          m[0] = AVG ? m[0] + e : max(m[0], e);
        }
      }
    }
    if (AVG) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        m[j] = (int)fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)(m[j] - zcnt), rcp)), z), 0.0f), 255.0f);
    }
    uint8_t* dst = out + (((long long)n * Ho + ho) * Wo + wo) * C + (long long)cg * VEC;
    if (VEC == 16) {
      uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < VEC; ++j) wd[j >> 2] |= (uint32_t)m[j] << (8 * (j & 3));
      *reinterpret_cast<uint4*>(dst) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    } else {
      dst[0] = (uint8_t)m[0];
    }
  }
}

inline int q8_out_extent(int in, int k, int s, int p, int d) { return (in + 2 * p - d * (k - 1) - 1) / s + 1; }

// geometry checks shared by the size query and the launch: 0 or a BTX_E_* code
inline int q8_check_geom(const BtxGeom* g) {
  if (g->NB <= 0 || g->H <= 0 || g->W <= 0 || g->C <= 0 || g->N <= 0 || g->KH <= 0 || g->KW <= 0) return BTX_E_SHAPE;
  if (g->sh <= 0 || g->sw <= 0 || g->dh <= 0 || g->dw <= 0 || g->ph < 0 || g->pw < 0) return BTX_E_SHAPE;
  if (g->D != 1 || g->KD != 1) return BTX_E_UNSUPPORTED;   // Linear and Conv2d only
  if (g->groups != 1) return BTX_E_UNSUPPORTED;
  if (q8_out_extent(g->H, g->KH, g->sh, g->ph, g->dh) <= 0 || q8_out_extent(g->W, g->KW, g->sw, g->pw, g->dw) <= 0) return BTX_E_SHAPE;
  return 0;
}

inline int q8_cp(int C) { return (C + 15) / 16 * 16; }
inline long long q8_kp(int taps, int C) { return ((long long)taps * q8_cp(C) + 63) / 64 * 64; }

// BtxQ8Add (host) -> the kernels' constants; 0 or BTX_E_SHAPE
inline int q8_add_args(const BtxQ8Add* h, Q8AddArgs* p) {
  if (!(h->s_a > 0.0f) || !(h->s_b > 0.0f) || !(h->inv_s > 0.0f) || h->zero_point < 0 || h->zero_point > 255) return BTX_E_SHAPE;
  p->s_a = h->s_a; p->pre_a = h->pre_a; p->s_b = h->s_b; p->pre_b = h->pre_b; p->inv_s = h->inv_s;
  p->z = (float)h->zero_point;
  p->lo = h->relu ? (float)h->zero_point : 0.0f;
  return 0;
}

// what btx_q8_contract and btx_q8_contract_res share: the checks in their order of precedence, the kernel's arguments, the grid
inline int q8_contract_setup(const BtxGeom* g, const uint8_t* x, int x_zero_point, const int8_t* W, const int32_t* S, const int32_t* b_i,
                             float multiplier, int out_zero_point, int relu, int out_f32, float out_scale, void* out, Q8ContractArgs* pa,
                             dim3* grid) {
  if (!g || !x || !W || !S || !b_i || !out) return BTX_E_NULL;
  const int rc = q8_check_geom(g);
  if (rc) return rc;
  if (x_zero_point < 0 || x_zero_point > 255 || out_zero_point < 0 || out_zero_point > 255 || !(multiplier > 0.0f)) return BTX_E_SHAPE;
  if (out_f32 && !(out_scale > 0.0f)) return BTX_E_SHAPE;
  const long long kp = q8_kp(g->KH * g->KW, g->C);
  if (kp > 0x7fffffc0LL) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)W & 15u) || ((uintptr_t)S & 3u) || ((uintptr_t)b_i & 3u)) return BTX_E_ALIGN;
  Q8ContractArgs& a = *pa;
  a.x = x; a.W = W; a.S = S; a.b_i = b_i; a.out = out;
  a.NB = g->NB; a.H = g->H; a.Wd = g->W; a.C = g->C; a.N = g->N; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->sh; a.sw = g->sw; a.ph = g->ph; a.pw = g->pw; a.dh = g->dh; a.dw = g->dw;
  a.OH = q8_out_extent(g->H, g->KH, g->sh, g->ph, g->dh);
  a.OW = q8_out_extent(g->W, g->KW, g->sw, g->pw, g->dw);
  a.taps = g->KH * g->KW; a.Cp = q8_cp(g->C); a.Kp = (int)kp;
  a.M = (long long)g->NB * a.OH * a.OW;
  const long long mblocks = (a.M + Q8_BM - 1) / Q8_BM;
  if (mblocks > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  a.z_x = x_zero_point; a.z_o = out_zero_point; a.lo = relu ? out_zero_point : 0;
  a.mult = multiplier; a.s_o = out_scale;
  a.out_f32 = out_f32 ? 1 : 0;
  a.x_vec = (g->C % 16 == 0 && ((uintptr_t)x & 15u) == 0) ? 1 : 0;
  a.out_vec = out_f32 ? ((g->N % 4 == 0 && ((uintptr_t)out & 15u) == 0) ? 1 : 0) : ((g->N % 4 == 0 && ((uintptr_t)out & 3u) == 0) ? 1 : 0);
  *grid = dim3((unsigned)mblocks, (unsigned)((g->N + Q8_BN - 1) / Q8_BN));
  return 0;
}

// the two pooling entry points: checks, output extent, grid (the conventions of maxpool_grid in btx_small.hip)
template <bool AVG>
int q8_pool_launch(const uint8_t* x, uint8_t* out, int NB, int H, int W, int C, int k, int stride, int pad, int zero_point, void* stream) {
  if (!x || !out) return BTX_E_NULL;
  if (NB <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0 || pad < 0 || 2 * pad > k) return BTX_E_SHAPE;
  if (zero_point < 0 || zero_point > 255) return BTX_E_SHAPE;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if (H + 2 * pad < k || W + 2 * pad < k || Ho <= 0 || Wo <= 0) return BTX_E_SHAPE;
  if (AVG && (long long)k * k > 8000000LL) return BTX_E_UNSUPPORTED;   // the int32 window sum: 255 * k * k
  const bool vec = C % 16 == 0 && ((((uintptr_t)x | (uintptr_t)out) & 15u) == 0);
  const long long total = (long long)NB * Ho * Wo * (vec ? C / 16 : C);
  long long blocks = (total + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  const int cnt = k * k;
  const float rcp = (float)(1.0 / (double)cnt);   // double reciprocal, rounded once
  if (vec)
    hipLaunchKernelGGL((q8_pool_cl_kernel<16, AVG>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, NB, H, W, C, Ho, Wo,
                       k, stride, pad, total, cnt * zero_point, rcp, (float)zero_point);
  else
    hipLaunchKernelGGL((q8_pool_cl_kernel<1, AVG>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, NB, H, W, C, Ho, Wo,
                       k, stride, pad, total, cnt * zero_point, rcp, (float)zero_point);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t btx_q8_weight_row_bytes(int taps, int C) {
  if (taps <= 0 || C <= 0) return 0;
  const long long kp = q8_kp(taps, C);
  return kp > 0x7fffffc0LL ? 0 : (size_t)kp;
}

int btx_q8_quantize_act(const void* x, int act_dtype, const int64_t* strides_host, uint8_t* out, int NB, int C, int H, int W,
                        float scale, int zero_point, void* stream) {
  if (!x || !strides_host || !out) return BTX_E_NULL;
  if (NB <= 0 || C <= 0 || H <= 0 || W <= 0 || !(scale > 0.0f) || zero_point < 0 || zero_point > 255) return BTX_E_SHAPE;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if ((uintptr_t)out & 3u) return BTX_E_ALIGN;
  const size_t total = (size_t)NB * C * H * W;
  size_t blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const float inv_s = 1.0f / scale;
  const long long sn = strides_host[0], sc = strides_host[1], sh = strides_host[2], sw = strides_host[3];
  if (act_dtype == BTX_ACT_F32)
    hipLaunchKernelGGL(q8_quantize_act_kernel<float>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x, out, C, H, W,
                       sn, sc, sh, sw, total, inv_s, (float)zero_point);
  else
    hipLaunchKernelGGL(q8_quantize_act_kernel<uint16_t>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, out, C,
                       H, W, sn, sc, sh, sw, total, inv_s, (float)zero_point);
  return (int)hipGetLastError();
}

int btx_q8_sample_weights(const int8_t* mu_i, const int8_t* sigma_i, const float* mu_b, const float* sigma_b, int N, int taps, int C,
                          int eps_C, const BtxQ8Chain* chain_host, const BtxRng* rng, const float* eps_w, const float* eps_b,
                          int8_t* W, int32_t* S, int32_t* b_i, void* stream) {
  if (!mu_i || !sigma_i || !chain_host || !W || !S || !b_i) return BTX_E_NULL;
  if (!rng && !eps_w) return BTX_E_NULL;                       // the noise comes from somewhere
  if (sigma_b && !mu_b) return BTX_E_NULL;
  if (mu_b && sigma_b && !rng && !eps_b) return BTX_E_NULL;
  if (N <= 0 || taps <= 0 || C <= 0) return BTX_E_SHAPE;
  if (eps_C < C || (eps_C & 7)) {
    if (!eps_w || eps_C != C) return BTX_E_SHAPE;              // the RNG index space has rows of a multiple of 8 channels
  }
  const long long kp = q8_kp(taps, C);
  if (kp > 0x7fffffc0LL || (long long)N * taps * (long long)eps_C > 0xfffffffcLL) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)W & 15u) || ((uintptr_t)S & 3u) || ((uintptr_t)b_i & 3u)) return BTX_E_ALIGN;
  const BtxQ8Chain& ch = *chain_host;
  if (!(ch.s_sigma > 0.0f) || !(ch.s_mu > 0.0f) || !(ch.s_eps > 0.0f) || !(ch.s_d > 0.0f) || !(ch.inv_s_eps > 0.0f) ||
      !(ch.inv_s_d > 0.0f) || !(ch.inv_s_w > 0.0f) || !(ch.bias_div > 0.0))
    return BTX_E_SHAPE;
  Q8SampleArgs a;
  a.mu_i = mu_i; a.sigma_i = sigma_i; a.mu_b = mu_b; a.sigma_b = sigma_b; a.eps_w = eps_w; a.eps_b = eps_b;
  a.W = W; a.S = S; a.b_i = b_i;
  a.N = N; a.taps = taps; a.C = C; a.eps_C = eps_C; a.Cp = q8_cp(C); a.Kp = (int)kp;
  a.ch = ch;
  a.k0 = rng ? (uint32_t)rng->seed : 0u;
  a.k1 = rng ? (uint32_t)(rng->seed >> 32) : 0u;
  a.sample = rng ? rng->sample_idx : 0u;
  a.layer = rng ? rng->layer_id : 0u;
  a.sample_ptr = rng ? (const uint32_t*)rng->sample_idx_dev : nullptr;
  hipLaunchKernelGGL(q8_sample_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int btx_q8_contract(const BtxGeom* g, const uint8_t* x, int x_zero_point, const int8_t* W, const int32_t* S, const int32_t* b_i,
                    float multiplier, int out_zero_point, int relu, int out_f32, float out_scale, void* out, void* stream) {
  Q8ContractArgs a;
  dim3 grid;
  const int rc = q8_contract_setup(g, x, x_zero_point, W, S, b_i, multiplier, out_zero_point, relu, out_f32, out_scale, out, &a, &grid);
  if (rc) return rc;
  Q8ResArgs ra = {};
  hipLaunchKernelGGL(q8_contract_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, ra);
  return (int)hipGetLastError();
}

int btx_q8_contract_res(const BtxGeom* g, const uint8_t* x, int x_zero_point, const int8_t* W, const int32_t* S, const int32_t* b_i,
                        float multiplier, int out_zero_point, int relu, int out_f32, const uint8_t* residual, const BtxQ8Add* add_host,
                        void* out, void* stream) {
  if (!residual || !add_host) return BTX_E_NULL;
  Q8ContractArgs a;
  dim3 grid;
  const int rc = q8_contract_setup(g, x, x_zero_point, W, S, b_i, multiplier, out_zero_point, relu, 0, add_host->s_a, out, &a, &grid);
  if (rc) return rc;
  if (out_f32) return BTX_E_UNSUPPORTED;   // the sum leaves as uint8 at the add's (s, z)
  Q8ResArgs ra;
  const int rc2 = q8_add_args(add_host, &ra.add);
  if (rc2) return rc2;
  ra.res = residual;
  ra.res_vec = (g->N % 4 == 0 && ((uintptr_t)residual & 3u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(q8_contract_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, ra);
  return (int)hipGetLastError();
}

int btx_q8_add(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, const BtxQ8Add* add_host, void* stream) {
  if (!a || !b || !out || !add_host) return BTX_E_NULL;
  if (n == 0) return BTX_E_SHAPE;
  Q8AddArgs p;
  const int rc = q8_add_args(add_host, &p);
  if (rc) return rc;
  size_t blocks = ((n + 15) / 16 + 255) / 256;
  if (blocks > 262144) blocks = 262144;
  const int vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(q8_add_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, out, n, p, vec);
  return (int)hipGetLastError();
}

int btx_q8_maxpool2d_cl(const uint8_t* x, uint8_t* out, int NB, int H, int W, int C, int k, int stride, int pad, void* stream) {
  return q8_pool_launch<false>(x, out, NB, H, W, C, k, stride, pad, 0, stream);
}

int btx_q8_avgpool2d_cl(const uint8_t* x, uint8_t* out, int NB, int H, int W, int C, int k, int stride, int pad, int ceil_mode,
                        int zero_point, void* stream) {
  if (!x || !out) return BTX_E_NULL;
  if (pad < 0) return BTX_E_SHAPE;
  if (pad != 0 || ceil_mode) return BTX_E_UNSUPPORTED;
  return q8_pool_launch<true>(x, out, NB, H, W, C, k, stride, 0, zero_point, stream);
}

int btx_q8_sample_delta(const int8_t* sigma_i, const float* mu_b, const float* sigma_b, int N, int taps, int C, int eps_C,
                        const BtxQ8Delta* delta_host, const BtxRng* rng, const float* eps_w, const float* eps_b, int8_t* D, int32_t* S_d,
                        int32_t* b_mean_i, int32_t* b_pert_i, void* stream) {
  if (!sigma_i || !delta_host || !D || !S_d || !b_mean_i || !b_pert_i) return BTX_E_NULL;
  if (!rng && !eps_w) return BTX_E_NULL;
  const BtxQ8Delta& d = *delta_host;
  if (d.mean_bias < BTX_Q8_BIAS_NONE || d.mean_bias > BTX_Q8_BIAS_SIGMA_EPS || d.pert_bias < BTX_Q8_BIAS_NONE ||
      d.pert_bias > BTX_Q8_BIAS_SIGMA_EPS)
    return BTX_E_SHAPE;
  const bool need_mu = d.mean_bias == BTX_Q8_BIAS_MU || d.pert_bias == BTX_Q8_BIAS_MU;
  const bool need_sigma = d.mean_bias == BTX_Q8_BIAS_SIGMA_EPS || d.pert_bias == BTX_Q8_BIAS_SIGMA_EPS;
  if ((need_mu && !mu_b) || (need_sigma && !sigma_b)) return BTX_E_NULL;
  if (need_sigma && !rng && !eps_b) return BTX_E_NULL;
  if (N <= 0 || taps <= 0 || C <= 0) return BTX_E_SHAPE;
  if (eps_C < C || (eps_C & 7)) {
    if (!eps_w || eps_C != C) return BTX_E_SHAPE;
  }
  if (!(d.inv_s_eps > 0.0f) || !(d.mult > 0.0f) || !(d.div_mean > 0.0) || !(d.div_pert > 0.0)) return BTX_E_SHAPE;
  const long long kp = q8_kp(taps, C);
  if (kp > 0x7fffffc0LL || (long long)N * taps * (long long)eps_C > 0xfffffffcLL) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)D & 15u) || ((uintptr_t)S_d & 3u) || ((uintptr_t)b_mean_i & 3u) || ((uintptr_t)b_pert_i & 3u)) return BTX_E_ALIGN;
  Q8DeltaArgs a;
  a.sigma_i = sigma_i; a.mu_b = mu_b; a.sigma_b = sigma_b; a.eps_w = eps_w; a.eps_b = eps_b;
  a.D = D; a.S = S_d; a.bm_i = b_mean_i; a.bp_i = b_pert_i;
  a.N = N; a.taps = taps; a.C = C; a.eps_C = eps_C; a.Cp = q8_cp(C); a.Kp = (int)kp;
  a.mean_bias = d.mean_bias; a.pert_bias = d.pert_bias;
  a.inv_s_eps = d.inv_s_eps; a.mult = d.mult; a.div_mean = d.div_mean; a.div_pert = d.div_pert;
  a.k0 = rng ? (uint32_t)rng->seed : 0u;
  a.k1 = rng ? (uint32_t)(rng->seed >> 32) : 0u;
  a.sample = rng ? rng->sample_idx : 0u;
  a.layer = rng ? rng->layer_id : 0u;
  a.sample_ptr = rng ? (const uint32_t*)rng->sample_idx_dev : nullptr;
  hipLaunchKernelGGL(q8_delta_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int btx_q8_contract_flipout(const BtxGeom* g, const uint8_t* x, const int8_t* W_mu, const int32_t* S_mu, const int32_t* b_mean_i,
                            const int8_t* D, const int32_t* S_d, const int32_t* b_pert_i, const BtxQ8Flipout* flip_host,
                            const BtxQ8Add* add_host, const BtxRng* rng, int sign_C, const int8_t* sign_in, const int8_t* sign_out,
                            int out_f32, void* out, void* stream) {
  if (!g || !x || !W_mu || !S_mu || !b_mean_i || !D || !S_d || !b_pert_i || !flip_host || !add_host || !out) return BTX_E_NULL;
  if (!rng && (!sign_in || !sign_out)) return BTX_E_NULL;   // the signs come from somewhere
  const int rc = q8_check_geom(g);
  if (rc) return rc;
  const BtxQ8Flipout& f = *flip_host;
  const int zs[5] = {f.z_x, f.z_xp, f.z_mean, f.z_pert, f.z_p2};
  for (int i = 0; i < 5; ++i)
    if (zs[i] < 0 || zs[i] > 255) return BTX_E_SHAPE;
  if (!(f.mult_xp > 0.0f) || !(f.mult_mean > 0.0f) || !(f.mult_pert > 0.0f) || !(f.mult_p2 > 0.0f)) return BTX_E_SHAPE;
  if (f.sin_pos < -255 || f.sin_pos > 255 || f.sin_neg < -255 || f.sin_neg > 255 || f.sout_pos < -255 || f.sout_pos > 255 ||
      f.sout_neg < -255 || f.sout_neg > 255)
    return BTX_E_SHAPE;
  if (out_f32 && !(f.out_scale > 0.0f)) return BTX_E_SHAPE;
  if (!sign_in && (sign_C < g->C || (sign_C & 7))) return BTX_E_SHAPE;   // the hash index space has rows of a multiple of 8 signs
  Q8FlipArgs a;
  const int rc2 = q8_add_args(add_host, &a.add);
  if (rc2) return rc2;
  const long long kp = q8_kp(g->KH * g->KW, g->C);
  if (kp > 0x7fffffc0LL) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)W_mu & 15u) || ((uintptr_t)D & 15u) || ((uintptr_t)S_mu & 3u) || ((uintptr_t)S_d & 3u) || ((uintptr_t)b_mean_i & 3u) ||
      ((uintptr_t)b_pert_i & 3u))
    return BTX_E_ALIGN;
  a.x = x; a.Wm = W_mu; a.D = D; a.Sm = S_mu; a.Sd = S_d; a.bm_i = b_mean_i; a.bp_i = b_pert_i;
  a.sign_in = sign_in; a.sign_out = sign_out; a.out = out;
  a.NB = g->NB; a.H = g->H; a.Wd = g->W; a.C = g->C; a.N = g->N; a.KH = g->KH; a.KW = g->KW;
  a.sh = g->sh; a.sw = g->sw; a.ph = g->ph; a.pw = g->pw; a.dh = g->dh; a.dw = g->dw;
  a.OH = q8_out_extent(g->H, g->KH, g->sh, g->ph, g->dh);
  a.OW = q8_out_extent(g->W, g->KW, g->sw, g->pw, g->dw);
  a.taps = g->KH * g->KW; a.Cp = q8_cp(g->C); a.Kp = (int)kp;
  a.sign_C = sign_in ? g->C : sign_C;
  a.M = (long long)g->NB * a.OH * a.OW;
  const long long mblocks = (a.M + Q8_BM - 1) / Q8_BM;
  if (mblocks > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  a.f = f;
  a.out_f32 = out_f32 ? 1 : 0;
  a.x_vec = (g->C % 16 == 0 && ((uintptr_t)x & 15u) == 0) ? 1 : 0;
  a.out_vec = out_f32 ? ((g->N % 4 == 0 && ((uintptr_t)out & 15u) == 0) ? 1 : 0) : ((g->N % 4 == 0 && ((uintptr_t)out & 3u) == 0) ? 1 : 0);
  a.k0 = rng ? (uint32_t)rng->seed : 0u;
  a.k1 = rng ? (uint32_t)(rng->seed >> 32) : 0u;
  a.sample = rng ? rng->sample_idx : 0u;
  a.layer = rng ? rng->layer_id : 0u;
  a.sample_ptr = rng ? (const uint32_t*)rng->sample_idx_dev : nullptr;
  const dim3 grid((unsigned)mblocks, (unsigned)((g->N + Q8_BN - 1) / Q8_BN));
  hipLaunchKernelGGL(q8_flipout_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
