// K13: the bias gradient of a variational layer,  db_mu[n] = sum_m dy[m][n]  and (Flipout)  db_delta[n] = sum_m dy[m][n] * s_out[m][n],
// with a FIXED summation order.  The weight-gradient kernels (btx_wgrad.hip) can form these sums as a by-product, but their pixel
// chunks add into db with f32 atomics, so the last bit follows the arrival order of the workgroups; the weight gradient itself is
// reduced from slabs in chunk order, and a training step is only bit-reproducible if its bias gradients are too.
// dy: [M][N] pixel-major (channels-last), f32 or bf16.  s_out: the int8 tensor when given, else the hashed BTX-RNG v1 sign of element
// index m * N + n — the index and the keys btx_wgrad.hip uses (stream SIGN_OUT; SIGN_IN under BTX_FLAG_SWAP_SIGNS), the sample index read
// from the device word when the BtxRng carries one.
// Launch 1: workgroup (64 channels, part p) — thread (row r, channel c) adds the pixels m0 + r, m0 + r + 4, ... of its part in order, the
// four rows are added in index order; launch 2 (more than one part): one thread per (kind, channel) adds the parts in index order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/btx.h"
#include "btx_rng.h"

#define BG_THREADS 256
#define BG_ROWS 4
#define BG_PART_PX 1024
#define BG_MAX_PARTS 128

namespace {

template <typename ACT, int KIND>
__global__ __launch_bounds__(BG_THREADS) void bias_partial_kernel(const ACT* __restrict__ dy, long long M, int N, long long part_px,
                                                                 const int8_t* __restrict__ sign_out, uint32_t seed_lo, uint32_t seed_hi,
                                                                 uint32_t sample, const uint32_t* __restrict__ sample_ptr, uint32_t layer,
                                                                 uint32_t rng_stream, float* __restrict__ out_m, float* __restrict__ out_d) {
  __shared__ float red[2][BG_ROWS][64];
  const int cl = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  uint32_t ka = 0, kb = 0;
  if (KIND == 1 && !sign_out) {
    const uint32_t smp = sample_ptr ? *sample_ptr : sample;
    const BtxPhilox4 k = btx_philox4x32_10(0u, smp, layer, rng_stream, seed_lo, seed_hi);
    ka = k.x[0];
    kb = k.x[1];
  }
  const long long m0 = (long long)blockIdx.y * part_px, m1 = min(M, m0 + part_px);
  float sm = 0.f, sd = 0.f;
  if (c < N) {
    for (long long m = m0 + r; m < m1; m += BG_ROWS) {
      const unsigned long long i = (unsigned long long)m * (unsigned long long)N + (unsigned long long)c;
      const float v = (float)dy[i];
      sm += v;
      if (KIND == 1) {
        const bool neg = sign_out ? (sign_out[i] < 0)
                                  : (((btx_sign_word((uint32_t)(i >> 5), ka, kb) >> btx_sign_bitpos((uint32_t)i & 31u)) & 1u) != 0);
        sd += neg ? -v : v;
      }
    }
  }
  red[0][r][cl] = sm;
  red[1][r][cl] = sd;
  __syncthreads();
  if (r == 0 && c < N) {
    float a = red[0][0][cl], b = red[1][0][cl];
#pragma unroll
    for (int q = 1; q < BG_ROWS; ++q) { a += red[0][q][cl]; b += red[1][q][cl]; }
    out_m[(size_t)blockIdx.y * N + c] = a;
    if (KIND == 1) out_d[(size_t)blockIdx.y * N + c] = b;
  }
}

__global__ __launch_bounds__(BG_THREADS) void bias_finish_kernel(const float* __restrict__ part, int parts, int nk, int N,
                                                                float* __restrict__ db_mu, float* __restrict__ db_delta) {
  const int t = blockIdx.x * BG_THREADS + threadIdx.x;
  if (t >= nk * N) return;
  const int k = t / N, n = t - k * N;
  const float* src = part + (size_t)k * parts * N + n;
  float a = src[0];
  for (int p = 1; p < parts; ++p) a += src[(size_t)p * N];
  (k ? db_delta : db_mu)[n] = a;
}

inline int bias_parts(long long M) {
  const long long p = (M + BG_PART_PX - 1) / BG_PART_PX;
  return (int)(p < 1 ? 1 : (p > BG_MAX_PARTS ? BG_MAX_PARTS : p));
}

}  // namespace

extern "C" {

size_t btx_bias_grad_workspace_bytes(int64_t M, int N) {
  if (M < 1 || N < 1) return 16;
  const int parts = bias_parts(M);
  return parts > 1 ? (size_t)2 * parts * N * sizeof(float) : 16;
}

int btx_bias_grad(int kind, const void* dy, int64_t M, int N, int act_dtype, float* db_mu, float* db_delta, const BtxRng* rng,
                  const int8_t* sign_out, uint32_t flags, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !db_mu) return BTX_E_NULL;
  if (kind != BTX_KIND_REPARAM && kind != BTX_KIND_FLIPOUT) return BTX_E_UNSUPPORTED;
  if (kind == BTX_KIND_FLIPOUT && (!db_delta || (!rng && !sign_out))) return BTX_E_NULL;
  if (M < 1 || N < 1) return BTX_E_SHAPE;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  const int parts = bias_parts(M);
  const int nk = kind == BTX_KIND_FLIPOUT ? 2 : 1;
  if (parts > 1) {
    if (!ws) return BTX_E_NULL;
    if (ws_bytes < btx_bias_grad_workspace_bytes(M, N)) return BTX_E_WORKSPACE;
    if (((uintptr_t)ws) & 3) return BTX_E_ALIGN;
  }
  long long part_px = (M + parts - 1) / parts;
  part_px = (part_px + BG_ROWS - 1) / BG_ROWS * BG_ROWS;
  float* out_m = parts > 1 ? (float*)ws : db_mu;
  float* out_d = parts > 1 ? (float*)ws + (size_t)parts * N : db_delta;
  const uint32_t rs = (flags & BTX_FLAG_SWAP_SIGNS) ? BTX_STREAM_SIGN_IN : BTX_STREAM_SIGN_OUT;
  const uint32_t seed_lo = rng ? (uint32_t)rng->seed : 0u, seed_hi = rng ? (uint32_t)(rng->seed >> 32) : 0u;
  const uint32_t sample = rng ? rng->sample_idx : 0u, layer = rng ? rng->layer_id : 0u;
  const uint32_t* sp = rng ? rng->sample_idx_dev : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + 63) / 64, parts);
#define BTX_BG_LAUNCH(ACT, KIND)                                                                                                   \
  hipLaunchKernelGGL((bias_partial_kernel<ACT, KIND>), grid, dim3(BG_THREADS), 0, st, (const ACT*)dy, (long long)M, N, part_px,     \
                     sign_out, seed_lo, seed_hi, sample, sp, layer, rs, out_m, out_d)
  if (act_dtype == BTX_ACT_F32) {
    if (nk == 2) BTX_BG_LAUNCH(float, 1); else BTX_BG_LAUNCH(float, 0);
  } else {
    if (nk == 2) BTX_BG_LAUNCH(__bf16, 1); else BTX_BG_LAUNCH(__bf16, 0);
  }
#undef BTX_BG_LAUNCH
  if (parts > 1)
    hipLaunchKernelGGL(bias_finish_kernel, dim3((nk * N + BG_THREADS - 1) / BG_THREADS), dim3(BG_THREADS), 0, st, (const float*)ws,
                       parts, nk, N, db_mu, db_delta);
  return (int)hipGetLastError();
}

}  // extern "C"
