// btx_small.hip — the small HBM-bound kernels of libbtx.so with their C entry points (include/btx.h): KL reduce, noise
// materialisation, the stem's data-format pass, pooling, MC predictive accumulation.  gfx950 only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/btx.h"
#include "btx_contract.h"
#include "btx_heads.h"  // launch_by_act
#include "btx_rng.h"

using namespace btx;

// ========================================================================================================
// K1: KL(q||p) mean.  Reference: layers/base_variational_layer.py:65-68 (kl_div), sigma = log1p(exp(rho))
// from e.g. layers/flipout_layers/conv_flipout.py:362-368.  Each term is evaluated in f32 exactly as the
// reference spells it; the sum is carried in f64 and reduced in a fixed order (deterministic, no atomics).
// HBM-bound: 8 B/element read once.
// ========================================================================================================
constexpr int KL_BLOCK = 256;
constexpr int KL_MAX_BLOCKS = 1024;

__device__ __forceinline__ float kl_term(float mu, float rho, float pmu, float psig) {
  const float sig = log1pf(expf(rho));
  const float dm = mu - pmu;
  return logf(psig) - logf(sig) + (sig * sig + dm * dm) / (2.0f * (psig * psig)) - 0.5f;
}

// The sum of kl_term over elements [0, n) that fall to thread `t` of `nthreads`, reduced over the workgroup: the block's sum,
// valid in thread 0.
__device__ __forceinline__ double kl_block_sum(const float* __restrict__ mu, const float* __restrict__ rho, size_t n,
                                               const float* __restrict__ pmu_t, const float* __restrict__ psig_t, float pmu,
                                               float psig, size_t t, size_t nthreads) {
  double acc = 0.0;
  const size_t n4 = n >> 2;
  const bool vec_ok = ((((uintptr_t)mu | (uintptr_t)rho) & 15) == 0) && !pmu_t && !psig_t;
  if (vec_ok) {
    for (size_t i = t; i < n4; i += nthreads) {
      const f32x4 m = ((const f32x4*)mu)[i];
      const f32x4 r = ((const f32x4*)rho)[i];
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s += kl_term(m[e], r[e], pmu, psig);
      acc += (double)s;
    }
    for (size_t i = (n4 << 2) + t; i < n; i += nthreads) acc += (double)kl_term(mu[i], rho[i], pmu, psig);
  } else {
    for (size_t i = t; i < n; i += nthreads)
      acc += (double)kl_term(mu[i], rho[i], pmu_t ? pmu_t[i] : pmu, psig_t ? psig_t[i] : psig);
  }
  // wave64 shuffle reduce -> LDS -> one value per block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double wsum[KL_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < KL_BLOCK / 64; ++w) s += wsum[w];
  }
  return s;
}

__global__ __launch_bounds__(KL_BLOCK) void kl_partial_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                                              size_t n, const float* __restrict__ pmu_t,
                                                              const float* __restrict__ psig_t, float pmu, float psig,
                                                              double* __restrict__ partials) {
  const double s = kl_block_sum(mu, rho, n, pmu_t, psig_t, pmu, psig, (size_t)blockIdx.x * KL_BLOCK + threadIdx.x,
                                (size_t)gridDim.x * KL_BLOCK);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void kl_final_kernel(const double* __restrict__ partials, int nblocks, double inv_n,
                                                      float* __restrict__ out, int accumulate) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) acc += partials[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) {
    const float kl = (float)(acc * inv_n);
    out[0] = accumulate ? out[0] + kl : kl;
  }
}

// Batched form: every parameter tensor of a model in ONE launch (+ one final reduce).  get_kl_loss() of ResNet18 is 22
// tensors; launched one by one (2 launches each) the reduction ran at ~3 % of the HBM roofline, launch-bound.
constexpr int KL_MAX_ITEMS = 48;
struct KlItemDev {
  const float* mu; const float* rho; const float* pmu_t; const float* psig_t;
  float* dmu; float* drho;  // backward only
  float pmu, psig;
  uint32_t n, first_block;
};
struct KlBatchDev {
  KlItemDev it[KL_MAX_ITEMS];
  int n;
  uint32_t total_blocks;
};
__global__ __launch_bounds__(KL_BLOCK) void kl_model_partial_kernel(const KlBatchDev b, double* __restrict__ partials) {
  int i = 0;
  for (int j = 1; j < b.n; ++j)
    if (blockIdx.x >= b.it[j].first_block) i = j;
  const KlItemDev& it = b.it[i];
  const uint32_t nblk = (i + 1 < b.n ? b.it[i + 1].first_block : b.total_blocks) - it.first_block;
  const size_t n = it.n;
  const double s = kl_block_sum(it.mu, it.rho, n, it.pmu_t, it.psig_t, it.pmu, it.psig,
                                (size_t)(blockIdx.x - it.first_block) * KL_BLOCK + threadIdx.x, (size_t)nblk * KL_BLOCK);
  // the reference takes the MEAN of each tensor, rounds it to f32 and sums the means: keep the mean scaling per tensor
  if (threadIdx.x == 0) partials[blockIdx.x] = s / (double)n;
}
// d(mean KL)/d(mu, rho) of every tensor, scaled by the upstream gradient (a device scalar: no host sync)
__global__ __launch_bounds__(KL_BLOCK) void kl_model_bwd_kernel(const KlBatchDev b, const float* __restrict__ gout) {
  int i = 0;
  for (int j = 1; j < b.n; ++j)
    if (blockIdx.x >= b.it[j].first_block) i = j;
  const KlItemDev& it = b.it[i];
  const uint32_t nblk = (i + 1 < b.n ? b.it[i + 1].first_block : b.total_blocks) - it.first_block;
  const float g = gout[0] / (float)it.n;
  for (size_t k = (size_t)(blockIdx.x - it.first_block) * KL_BLOCK + threadIdx.x; k < it.n; k += (size_t)nblk * KL_BLOCK) {
    const float mu = it.mu[k], rho = it.rho[k];
    const float pm = it.pmu_t ? it.pmu_t[k] : it.pmu, ps = it.psig_t ? it.psig_t[k] : it.psig;
    const float sig = log1pf(expf(rho));
    const float dsig = 1.0f / (1.0f + expf(-rho));  // d softplus / d rho
    const float ips2 = 1.0f / (ps * ps);
    it.dmu[k] = g * (mu - pm) * ips2;
    it.drho[k] = g * (sig * ips2 - 1.0f / sig) * dsig;
  }
}

extern "C" {
size_t btx_kl_workspace_bytes(size_t n) {
  (void)n;
  return (size_t)KL_MAX_BLOCKS * sizeof(double);
}

int btx_kl_gauss(const float* mu, const float* rho, size_t n, const float* prior_mu_t, const float* prior_sigma_t,
                 float prior_mu, float prior_sigma, float* kl_out, uint32_t flags, void* ws, size_t ws_bytes,
                 void* stream) {
  if (!mu || !rho || !kl_out || !ws) return BTX_E_NULL;
  if (n == 0) return BTX_E_SHAPE;
  if (ws_bytes < btx_kl_workspace_bytes(n)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  size_t want = (n + (size_t)KL_BLOCK * 8 - 1) / ((size_t)KL_BLOCK * 8);
  int nblocks = (int)(want < 1 ? 1 : (want > KL_MAX_BLOCKS ? KL_MAX_BLOCKS : want));
  hipLaunchKernelGGL(kl_partial_kernel, dim3(nblocks), dim3(KL_BLOCK), 0, st, mu, rho, n, prior_mu_t, prior_sigma_t,
                     prior_mu, prior_sigma, (double*)ws);
  hipLaunchKernelGGL(kl_final_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nblocks, 1.0 / (double)n, kl_out,
                     (flags & BTX_FLAG_KL_ACCUM) ? 1 : 0);
  return (int)hipGetLastError();
}

static int kl_fill_batch(const BtxKlItem* items, int base, int n_items, bool bwd, KlBatchDev* b) {
  memset(b, 0, sizeof(*b));
  b->n = n_items - base < KL_MAX_ITEMS ? n_items - base : KL_MAX_ITEMS;
  uint32_t blocks = 0;
  for (int i = 0; i < b->n; ++i) {
    const BtxKlItem& s = items[base + i];
    if (!s.mu || !s.rho || (bwd && (!s.dmu || !s.drho))) return BTX_E_NULL;
    if (s.n == 0 || s.n > 0xffffffffull) return BTX_E_SHAPE;
    KlItemDev& it = b->it[i];
    it.mu = s.mu; it.rho = s.rho; it.pmu_t = s.prior_mu_t; it.psig_t = s.prior_sigma_t; it.dmu = s.dmu; it.drho = s.drho;
    it.pmu = s.prior_mu; it.psig = s.prior_sigma; it.n = (uint32_t)s.n; it.first_block = blocks;
    uint32_t nb = (uint32_t)((s.n + (size_t)KL_BLOCK * 8 - 1) / ((size_t)KL_BLOCK * 8));
    if (nb < 1) nb = 1;
    if (nb > 256u) nb = 256u;
    blocks += nb;
  }
  b->total_blocks = blocks;
  return 0;
}

size_t btx_kl_model_workspace_bytes(int n_items) {
  if (n_items <= 0) return 0;
  return (size_t)((n_items + KL_MAX_ITEMS - 1) / KL_MAX_ITEMS) * KL_MAX_ITEMS * 256 * sizeof(double);
}

int btx_kl_gauss_model(const BtxKlItem* items, int n_items, float* kl_out, void* ws, size_t ws_bytes, void* stream) {
  if (!items || !kl_out || !ws) return BTX_E_NULL;
  if (n_items <= 0) return BTX_E_SHAPE;
  if (ws_bytes < btx_kl_model_workspace_bytes(n_items)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  int total = 0;
  for (int base = 0; base < n_items; base += KL_MAX_ITEMS) {
    KlBatchDev b;
    int rc = kl_fill_batch(items, base, n_items, false, &b);
    if (rc) return rc;
    hipLaunchKernelGGL(kl_model_partial_kernel, dim3(b.total_blocks), dim3(KL_BLOCK), 0, st, b, part + total);
    total += (int)b.total_blocks;
  }
  hipLaunchKernelGGL(kl_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, total, 1.0, kl_out, 0);
  return (int)hipGetLastError();
}

int btx_kl_gauss_model_bwd(const BtxKlItem* items, int n_items, const float* grad_out, void* stream) {
  if (!items || !grad_out) return BTX_E_NULL;
  if (n_items <= 0) return BTX_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < n_items; base += KL_MAX_ITEMS) {
    KlBatchDev b;
    int rc = kl_fill_batch(items, base, n_items, true, &b);
    if (rc) return rc;
    hipLaunchKernelGGL(kl_model_bwd_kernel, dim3(b.total_blocks), dim3(KL_BLOCK), 0, st, b, grad_out);
  }
  return (int)hipGetLastError();
}
}  // extern "C"

// ========================================================================================================
// noise materialisation (BTX-RNG v1)
// ========================================================================================================
__global__ __launch_bounds__(256) void fill_eps_kernel(float* __restrict__ out, size_t n, uint32_t k0, uint32_t k1,
                                                       uint32_t sample, uint32_t layer, uint32_t stream,
                                                       const uint32_t* __restrict__ sample_ptr) {
  if (sample_ptr) sample = __builtin_amdgcn_readfirstlane(*sample_ptr);  // BtxRng.sample_idx_dev (captured steps)
  const size_t nblk = (n + 3) >> 2;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (size_t)gridDim.x * 256) {
    float z[4];
    btx_normal4((uint32_t)b, sample, layer, stream, k0, k1, z);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((b << 2) + e < n) out[(b << 2) + e] = z[e];
  }
}

// drho = dw * eps * sigmoid(rho): the elementwise follow-up of the weight gradient, eps regenerated (never materialised)
__global__ __launch_bounds__(256) void rho_grad_kernel(const float* __restrict__ dw, const float* __restrict__ rho,
                                                       float* __restrict__ drho, size_t n, uint32_t k0, uint32_t k1,
                                                       uint32_t sample, uint32_t layer, uint32_t stream,
                                                       const uint32_t* __restrict__ sample_ptr) {
  if (sample_ptr) sample = __builtin_amdgcn_readfirstlane(*sample_ptr);
  const size_t nblk = (n + 3) >> 2;
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (size_t)gridDim.x * 256) {
    float z[4];
    btx_normal4((uint32_t)b, sample, layer, stream, k0, k1, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t i = (b << 2) + e;
      if (i < n) drho[i] = dw[i] * z[e] * (1.0f / (1.0f + expf(-rho[i])));
    }
  }
}

__global__ __launch_bounds__(256) void fill_sign_kernel(int8_t* __restrict__ out, size_t n, uint32_t ka, uint32_t kb) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const uint32_t w = btx_sign_word((uint32_t)(i >> 5), ka, kb);
    out[i] = ((w >> btx_sign_bitpos((uint32_t)i & 31u)) & 1u) ? (int8_t)-1 : (int8_t)1;
  }
}

extern "C" {
int btx_fill_eps(float* out, size_t n, const BtxRng* rng, uint32_t rng_stream, void* stream) {
  if (!out || !rng) return BTX_E_NULL;
  if (n == 0) return 0;
  size_t blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(fill_eps_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, out, n,
                     (uint32_t)rng->seed, (uint32_t)(rng->seed >> 32), rng->sample_idx, rng->layer_id, rng_stream,
                     (const uint32_t*)rng->sample_idx_dev);
  return (int)hipGetLastError();
}

int btx_rho_grad(const float* dw, const float* rho, float* drho, size_t n, const BtxRng* rng, uint32_t rng_stream,
                 void* stream) {
  if (!dw || !rho || !drho || !rng) return BTX_E_NULL;
  if (n == 0) return 0;
  if (n > 0xfffffffcULL) return BTX_E_UNSUPPORTED;  // BTX-RNG v1 block index is 32 bits
  size_t blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(rho_grad_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, dw, rho, drho, n,
                     (uint32_t)rng->seed, (uint32_t)(rng->seed >> 32), rng->sample_idx, rng->layer_id, rng_stream,
                     (const uint32_t*)rng->sample_idx_dev);
  return (int)hipGetLastError();
}

int btx_fill_sign(int8_t* out, size_t n, const BtxRng* rng, uint32_t rng_stream, void* stream) {
  if (!out || !rng) return BTX_E_NULL;
  if (n == 0) return 0;
  uint32_t ka, kb;
  sign_keys(rng, rng_stream, &ka, &kb);
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(fill_sign_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, out, n, ka, kb);
  return (int)hipGetLastError();
}
}  // extern "C"

// ========================================================================================================
// btx_rowfuse_pack: the data-format step in front of the small-C stem path (BTX_FLAG_ROWFUSE) — logical [N,C,H,W]
// activations in any strides/dtype -> zero-padded channels-last [N][Hp][Wp][cp] in the MFMA dtype, one pass
// (replaces a fill + a strided copy + a cast).  One thread per output pixel.
// ========================================================================================================
template <typename IN, typename OUT, int CP>
__global__ __launch_bounds__(256) void rowfuse_pack_kernel(const IN* __restrict__ x, OUT* __restrict__ out, int NB, int C,
                                                           int H, int W, int Hp, int Wp, int ph, int pw, long long sn,
                                                           long long sc, long long sh, long long sw, long long total) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int wp = (int)(t % Wp);
    const long long r = t / Wp;
    const int hp = (int)(r % Hp);
    const int n = (int)(r / Hp);
    const int h = hp - ph, w = wp - pw;
    struct alignas(sizeof(OUT) * CP) Px { OUT v[CP]; };
    Px px;
    OUT* v = px.v;
#pragma unroll
    for (int c = 0; c < CP; ++c) v[c] = (OUT)0.f;
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
      const IN* src = x + n * sn + h * sh + w * sw;
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) v[c] = (OUT)(float)src[c * sc];
    }
    *(Px*)(out + t * CP) = px;  // one 8/16/32-byte store per pixel
  }
}
template <typename IN, typename OUT>
static int launch_rowfuse_pack(const void* x, void* out, int NB, int C, int H, int W, int Hp, int Wp, int cp, int ph,
                               int pw, const int64_t* st, hipStream_t stream) {
  const long long total = (long long)NB * Hp * Wp;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (cp == 4)
    hipLaunchKernelGGL((rowfuse_pack_kernel<IN, OUT, 4>), dim3((int)blocks), dim3(256), 0, stream, (const IN*)x, (OUT*)out,
                       NB, C, H, W, Hp, Wp, ph, pw, (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3], total);
  else
    hipLaunchKernelGGL((rowfuse_pack_kernel<IN, OUT, 8>), dim3((int)blocks), dim3(256), 0, stream, (const IN*)x, (OUT*)out,
                       NB, C, H, W, Hp, Wp, ph, pw, (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3], total);
  return (int)hipGetLastError();
}

extern "C" {
int btx_rowfuse_pack(const void* x, int in_dtype, const int64_t* strides_ncHW, int NB, int C, int H, int W, void* out,
                     int out_dtype, int Hp, int Wp, int cp, int ph, int pw, void* stream) {
  if (!x || !out || !strides_ncHW) return BTX_E_NULL;
  if (NB <= 0 || C <= 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0 || Hp < H + ph || Wp < W + pw) return BTX_E_SHAPE;
  if ((cp != 4 && cp != 8) || C > cp) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)out) & 15) return BTX_E_ALIGN;  // one store per padded pixel (8 / 16 / 32 bytes); x is read element by element
  hipStream_t st = (hipStream_t)stream;
  const bool ib = in_dtype == BTX_ACT_BF16, ob = out_dtype == BTX_ACT_BF16;
  if ((!ib && in_dtype != BTX_ACT_F32) || (!ob && out_dtype != BTX_ACT_F32)) return BTX_E_DTYPE;
  if (ib && ob) return launch_rowfuse_pack<__bf16, __bf16>(x, out, NB, C, H, W, Hp, Wp, cp, ph, pw, strides_ncHW, st);
  if (ib && !ob) return launch_rowfuse_pack<__bf16, float>(x, out, NB, C, H, W, Hp, Wp, cp, ph, pw, strides_ncHW, st);
  if (!ib && ob) return launch_rowfuse_pack<float, __bf16>(x, out, NB, C, H, W, Hp, Wp, cp, ph, pw, strides_ncHW, st);
  return launch_rowfuse_pack<float, float>(x, out, NB, C, H, W, Hp, Wp, cp, ph, pw, strides_ncHW, st);
}
}  // extern "C"

// ========================================================================================================
// pooling of channels-last activations.  Every thread owns 8 channels (16 B bf16 / 32 B f32) of a pixel:
// ========================================================================================================
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ src, float* v) {  // 16-byte loads
  if constexpr (sizeof(T) == 2) {
    const u32x4 q = *(const u32x4*)src;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = u2f(q[j] << 16); v[2 * j + 1] = u2f(q[j] & 0xffff0000u); }
  } else {
    const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
}
// ROUND: bf16 by round to nearest even, as torch's float -> bfloat16; else by truncation — exact where the values are bf16 already
template <bool ROUND, typename T>
__device__ __forceinline__ void store8(T* __restrict__ dst, const float* v) {
  if constexpr (sizeof(T) == 2) {
    if constexpr (ROUND) {
      *(u32x4*)dst = pack_granule<1>(v);
    } else {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (f2u(v[2 * j]) >> 16) | (f2u(v[2 * j + 1]) & 0xffff0000u);
      *(u32x4*)dst = o;
    }
  } else {
    *(f32x4*)dst = (f32x4){v[0], v[1], v[2], v[3]};
    *(f32x4*)(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  }
}

// btx_maxpool2d_cl: channels-last max pooling, the op between the stem and layer1 of a ResNet (reference
// models/deterministic/resnet_large.py: self.maxpool).  HBM-bound: every thread owns 8 channels (16 B bf16 / 32 B
// f32) of one output pixel, reads its window with 16-byte loads, writes once.
template <typename T>
__global__ __launch_bounds__(256) void maxpool2d_cl_kernel(const T* __restrict__ x, T* __restrict__ out, int NB, int H,
                                                           int W, int C, int Ho, int Wo, int k, int s, int pad,
                                                           long long total) {
  const int cgs = C >> 3;  // groups of 8 channels
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % cgs);
    long long r = t / cgs;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int kh = 0; kh < k; ++kh) {
      const int h = ho * s - pad + kh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int w = wo * s - pad + kw;
        if ((unsigned)w >= (unsigned)W) continue;
        float v[8];
        load8(x + (((long long)n * H + h) * W + w) * C + cg * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[j]);
      }
    }
    store8<false>(out + (((long long)n * Ho + ho) * Wo + wo) * C + cg * 8, m);  // exact: inputs are bf16
  }
}

// Training form (the reference's training loop runs nn.MaxPool2d under autograd: resnet_large.py self.maxpool): the same pass also
// writes, per output element, the position kh * k + kw of its maximum inside the window — the FIRST maximum in scan order, as
// torch's max_pool2d_with_indices picks it (`val > max || isnan(val)`: post-ReLU maps are full of ties at 0) — one byte instead of
// ATen's int64 index; the backward routes dy with it.  (Not the kernel above with an index: that one takes fmaxf and drops NaN.)
template <typename T>
__global__ __launch_bounds__(256) void maxpool2d_cl_idx_kernel(const T* __restrict__ x, T* __restrict__ out, uint8_t* __restrict__ idx,
                                                               int NB, int H, int W, int C, int Ho, int Wo, int k, int s, int pad,
                                                               long long total) {
  const int cgs = C >> 3;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % cgs);
    long long r = t / cgs;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float m[8];
    uint32_t id[8];
    bool first = true;
    for (int kh = 0; kh < k; ++kh) {
      const int h = ho * s - pad + kh;
      if ((unsigned)h >= (unsigned)H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int w = wo * s - pad + kw;
        if ((unsigned)w >= (unsigned)W) continue;
        float v[8];
        load8(x + (((long long)n * H + h) * W + w) * C + cg * 8, v);
        const uint32_t pos = (uint32_t)(kh * k + kw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool take = first || v[j] > m[j] || v[j] != v[j];
          m[j] = take ? v[j] : m[j];
          id[j] = take ? pos : id[j];
        }
        first = false;
      }
    }
    if (first) {  // a window entirely in the padding (2 * pad <= k rules it out; kept total)
#pragma unroll
      for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; id[j] = 0u; }
    }
    store8<false>(out + (((long long)n * Ho + ho) * Wo + wo) * C + cg * 8, m);  // exact: inputs are bf16
    u32x2 ib;
    ib[0] = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
    ib[1] = id[4] | (id[5] << 8) | (id[6] << 16) | (id[7] << 24);
    *(u32x2*)(idx + t * 8) = ib;
  }
}

// dx[n][h][w][c] = sum of dy over the (at most ceil(k/s)^2) windows that cover (h, w) and whose recorded maximum sits there; f32
// accumulation, one rounding (as ATen's max_pool_backward_nhwc).  A thread owns 8 channels of one INPUT pixel: no atomics.
template <typename T>
__global__ __launch_bounds__(256) void maxpool2d_cl_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                               T* __restrict__ dx, int NB, int H, int W, int C, int Ho, int Wo, int k,
                                                               int s, int pad, long long total) {
  const int cgs = C >> 3;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % cgs);
    long long r = t / cgs;
    const int w = (int)(r % W);
    r /= W;
    const int h = (int)(r % H);
    const int n = (int)(r / H);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const int th = h + pad - k + 1, tw = w + pad - k + 1;
    const int ho_lo = th <= 0 ? 0 : (th + s - 1) / s, ho_hi = min(Ho - 1, (h + pad) / s);
    const int wo_lo = tw <= 0 ? 0 : (tw + s - 1) / s, wo_hi = min(Wo - 1, (w + pad) / s);
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      const int kh = h + pad - ho * s;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        const uint32_t pos = (uint32_t)(kh * k + (w + pad - wo * s));
        const long long o = (((long long)n * Ho + ho) * Wo + wo) * cgs + cg;
        const u32x2 ib = *(const u32x2*)(idx + o * 8);
        float g[8];
        load8(dy + o * 8, g);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (((ib[j >> 2] >> (8 * (j & 3))) & 0xffu) == pos) ? g[j] : 0.f;
      }
    }
    store8<true>(dx + t * 8, acc);  // round to nearest even, as torch's float -> bfloat16
  }
}

// btx_avgpool_global_cl: global average pooling of channels-last activations ([NB][HW][C] -> [NB][C], f32 accumulate),
// the op in front of the classifier of the reference's ResNets (resnet_large.py: avgpool).  One workgroup per image and
// 64-channel slab: 8 lanes cover the slab with 16-byte loads, 32 pixel groups run in parallel, LDS tree at the end.
template <typename T>
__global__ __launch_bounds__(256) void avgpool_global_cl_kernel(const T* __restrict__ x, T* __restrict__ out, int HW, int C,
                                                                float inv) {
  const int n = blockIdx.y, slab = blockIdx.x;
  const int cg = threadIdx.x & 7, pg = threadIdx.x >> 3;  // 8 channel groups x 32 pixel groups
  const int c0 = slab * 64 + cg * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < C) {
    for (int pix = pg; pix < HW; pix += 32) {
      float v[8];
      load8(x + ((long long)n * HW + pix) * C + c0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
  __shared__ float red[32][64 + 1];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[pg][cg * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int g = 0; g < 32; ++g) s += red[g][threadIdx.x];  // fixed order: deterministic
    const int c = slab * 64 + threadIdx.x;
    if (c < C) out[(long long)n * C + c] = (T)(s * inv);
  }
}

// What the three btx_maxpool2d_cl* entry points share: the argument checks in their order of precedence, the output extent and
// the grid.  `a`, `b`: the two activation tensors; `idx`: the window positions (with_idx: the training pair; the window
// position must fit a byte); per_input: one thread per 8 channels of an INPUT pixel (the backward), else of an output pixel.
struct PoolGrid {
  int Ho, Wo, blocks;
  long long total;
};
static int maxpool_grid(const void* a, const void* b, const uint8_t* idx, bool with_idx, bool per_input, int NB, int H, int W, int C,
                        int k, int stride, int pad, PoolGrid* pg) {
  if (!a || !b || (with_idx && !idx)) return BTX_E_NULL;
  if (NB <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0 || pad < 0 || 2 * pad > k) return BTX_E_SHAPE;
  if (C % 8 || (with_idx && k > 15)) return BTX_E_UNSUPPORTED;
  if ((((uintptr_t)a | (uintptr_t)b) & 15) || (with_idx && (((uintptr_t)idx) & 7))) return BTX_E_ALIGN;
  pg->Ho = (H + 2 * pad - k) / stride + 1;
  pg->Wo = (W + 2 * pad - k) / stride + 1;
  if (pg->Ho <= 0 || pg->Wo <= 0) return BTX_E_SHAPE;
  pg->total = per_input ? (long long)NB * H * W * (C / 8) : (long long)NB * pg->Ho * pg->Wo * (C / 8);
  const long long blocks = (pg->total + 255) / 256;
  pg->blocks = (int)(blocks > 262144 ? 262144 : blocks);
  return 0;
}

extern "C" {
int btx_maxpool2d_cl(const void* x, void* out, int dtype, int NB, int H, int W, int C, int k, int stride, int pad,
                     void* stream) {
  PoolGrid pg;
  const int rc = maxpool_grid(x, out, nullptr, false, false, NB, H, W, C, k, stride, pad, &pg);
  if (rc) return rc;
  return launch_by_act(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(maxpool2d_cl_kernel<T>, dim3(pg.blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)out, NB, H, W, C,
                       pg.Ho, pg.Wo, k, stride, pad, pg.total);
  });
}

int btx_maxpool2d_cl_train(const void* x, void* out, uint8_t* idx, int dtype, int NB, int H, int W, int C, int k, int stride, int pad,
                           void* stream) {
  PoolGrid pg;
  const int rc = maxpool_grid(x, out, idx, true, false, NB, H, W, C, k, stride, pad, &pg);
  if (rc) return rc;
  return launch_by_act(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(maxpool2d_cl_idx_kernel<T>, dim3(pg.blocks), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)out, idx, NB, H,
                       W, C, pg.Ho, pg.Wo, k, stride, pad, pg.total);
  });
}

int btx_maxpool2d_cl_bwd(const void* dy, const uint8_t* idx, void* dx, int dtype, int NB, int H, int W, int C, int k, int stride,
                         int pad, void* stream) {
  PoolGrid pg;
  const int rc = maxpool_grid(dy, dx, idx, true, true, NB, H, W, C, k, stride, pad, &pg);
  if (rc) return rc;
  return launch_by_act(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(maxpool2d_cl_bwd_kernel<T>, dim3(pg.blocks), dim3(256), 0, (hipStream_t)stream, (const T*)dy, idx, (T*)dx, NB, H,
                       W, C, pg.Ho, pg.Wo, k, stride, pad, pg.total);
  });
}

int btx_avgpool_global_cl(const void* x, void* out, int dtype, int NB, int HW, int C, void* stream) {
  if (!x || !out) return BTX_E_NULL;
  if (NB <= 0 || HW <= 0 || C <= 0) return BTX_E_SHAPE;
  if (C % 8) return BTX_E_UNSUPPORTED;
  if (((uintptr_t)x) & 15) return BTX_E_ALIGN;
  return launch_by_act(dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(avgpool_global_cl_kernel<T>, dim3((C + 63) / 64, NB), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)out,
                       HW, C, 1.0f / (float)HW);
  });
}
}  // extern "C"

// ========================================================================================================
// K6: MC predictive accumulation.  Reference (host side, numpy/torch): torch.stack(output_mc) -> softmax(dim=2)
// -> mean(dim=0)  examples/main_bayesian_imagenet_dnn2bnn.py:483-499 ; predictive_entropy / mutual_information
// utils/util.py:41-60.  One workgroup per batch row; the row is owned by that workgroup so no atomics.
// ========================================================================================================
// lanes > 1 (btx_mc_accumulate_lanes): the logits of `lanes` MC samples back to back ([lanes][bs][C]).  A workgroup owns a
// batch row; its sixteen waves take the lanes round-robin — one wave computes one lane's softmax row (probabilities into LDS, the
// lane's entropy beside them) with no workgroup barrier — then every thread adds its columns' probabilities lane by lane IN
// ORDER: the same additions, in the same order, as `lanes` single-sample launches (which run this very code with one lane),
// at a sixteenth of the serial depth (20 lanes: 78 -> ~20 us per replay of the bench).  The per-row reductions keep a fixed
// shape — 256 "virtual threads" (4 per thread: column v + 256 k), a shuffle tree per virtual wave, ((r0 + r1) + r2) + r3 — so a
// row's figures do not depend on which wave computed it.  LDS: min(lanes, LC) x C floats; more lanes run in chunks of LC.
template <typename ACT>
__global__ __launch_bounds__(1024) void mc_accumulate_kernel(const ACT* __restrict__ logits, int bs, int C, float kl,
                                                            float* __restrict__ packed, int lanes, int LC) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_smem[];
  float* const pr_lds = (float*)mc_smem;            // [LC][C]
  float* const ent_lds = pr_lds + (size_t)LC * C;   // [LC]
  const int row = blockIdx.x;
  const int wave = threadIdx.x >> 6, li = threadIdx.x & 63;
  float* const sp = packed + (size_t)row * C;
  float* const sp2 = packed + (size_t)bs * C + (size_t)row * C;
  for (int l0 = 0; l0 < lanes; l0 += LC) {
    const int nl = min(LC, lanes - l0);
    for (int k = wave; k < nl; k += 16) {  // wave-uniform
      const ACT* lr = logits + ((size_t)(l0 + k) * bs + row) * C;
      float* const pk = pr_lds + (size_t)k * C;
      float mx = -INFINITY;
      for (int c = li; c < C; c += 64) mx = fmaxf(mx, (float)lr[c]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      float se[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        for (int c = j * 64 + li; c < C; c += 256) se[j] += expf((float)lr[c] - mx);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) se[j] += __shfl_down(se[j], off, 64);
      const float tot = __shfl(((se[0] + se[1]) + se[2]) + se[3], 0, 64);
      const float inv = 1.0f / tot;
      float en[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        for (int c = j * 64 + li; c < C; c += 256) {
          const float pv = expf((float)lr[c] - mx) * inv;
          pk[c] = pv;
          const float t = pv * logf(pv + 1e-15f);  // utils/util.py:44 epsilon
          en[j] -= t;
        }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) en[j] += __shfl_down(en[j], off, 64);
      if (li == 0) ent_lds[k] = ((en[0] + en[1]) + en[2]) + en[3];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 1024) {
      float a = sp[c], a2 = sp2[c];
      for (int k = 0; k < nl; ++k) {
        const float pv = pr_lds[(size_t)k * C + c];
        a += pv;
        const float q = pv * pv;
        a2 += q;
      }
      sp[c] = a;
      sp2[c] = a2;
    }
    if (threadIdx.x == 0) {
      float e = packed[(size_t)2 * bs * C + row];
      for (int k = 0; k < nl; ++k) e += ent_lds[k];
      packed[(size_t)2 * bs * C + row] = e;
      if (row == 0) {
        float a = packed[(size_t)2 * bs * C + bs], n = packed[(size_t)2 * bs * C + bs + 1];
        for (int k = 0; k < nl; ++k) { a += kl; n += 1.0f; }
        packed[(size_t)2 * bs * C + bs] = a;
        packed[(size_t)2 * bs * C + bs + 1] = n;
      }
    }
    __syncthreads();  // the next chunk overwrites the LDS rows
  }
}

extern "C" {
size_t btx_mc_packed_floats(int bs, int C) {
  if (bs <= 0 || C <= 0) return 0;
  return (size_t)2 * bs * C + (size_t)bs + 2;
}

int btx_mc_accumulate(const void* logits, int bs, int C, int act_dtype, float kl, float* packed, void* stream) {
  return btx_mc_accumulate_lanes(logits, 1, bs, C, act_dtype, kl, packed, stream);
}

int btx_mc_accumulate_lanes(const void* logits, int lanes, int bs, int C, int act_dtype, float kl, float* packed,
                            void* stream) {
  if (!logits || !packed) return BTX_E_NULL;
  if (bs <= 0 || C <= 0 || lanes <= 0) return BTX_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  // lanes per LDS chunk: up to 96 KiB of probabilities.  Above the 64 KiB every kernel may use, the limit is an opt-in per
  // function AND per device: asked for once per device, and a device that refuses keeps 64 KiB chunks.
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const bool f32 = act_dtype == BTX_ACT_F32;
  if (!f32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  static unsigned char big_lds[2][64];  // 0 not asked yet, 1 granted, 2 refused
  unsigned char& st_big = big_lds[f32 ? 0 : 1][dev];
  if (!st_big) {
    const void* fn = f32 ? (const void*)mc_accumulate_kernel<float> : (const void*)mc_accumulate_kernel<__bf16>;
    st_big = (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 98304 + 64) == hipSuccess) ? 1 : 2;
    if (st_big == 2) (void)hipGetLastError();
  }
  const size_t chunk = (st_big == 1) ? (size_t)98304 : (size_t)65536;
  const size_t per_lane = (size_t)C * 4 + 4;
  int LC = (int)(chunk / per_lane);
  if (LC < 1) return BTX_E_UNSUPPORTED;  // a row of > 24 575 classes does not fit a chunk (include/btx.h K6)
  if (LC > lanes) LC = lanes;
  const size_t lds = (size_t)LC * per_lane;
  if (f32)
    hipLaunchKernelGGL(mc_accumulate_kernel<float>, dim3(bs), dim3(1024), lds, st, (const float*)logits, bs, C, kl, packed,
                       lanes, LC);
  else
    hipLaunchKernelGGL(mc_accumulate_kernel<__bf16>, dim3(bs), dim3(1024), lds, st, (const __bf16*)logits, bs, C, kl,
                       packed, lanes, LC);
  return (int)hipGetLastError();
}

}  // extern "C"
