// btx_klmc.hip — BTX-KLMC v1: the sampled KL of a variational Gaussian against a non-Gaussian weight prior
// (two-component scale mixture, Laplace, Student-t) for every parameter tensor of a model, forward and backward.  gfx950 only.
//
//   kl = sum over tensors of (1 / n) sum_i [ -log sigma_i - (1 + log 2 pi) / 2 - (1 / S) sum_j log p(mu_i + sigma_i eps_j[i]) ]
//
// The entropy is closed-form, the cross term is sampled with the estimator's own BTX-RNG v1 streams (BTX_STREAM_KL_W / _KL_B |
// j << 8): eps is regenerated in both directions and never stored.  The shape follows btx_kl_gauss_model in btx_small.hip: up to
// 48 items per launch, each with its own block range, an f64 partial per block scaled by 1 / n, one fixed-order final reduce.
// A thread owns one Philox group (four consecutive elements) at a time and loops over the draws in registers.
// VALU-bound: per element and draw one quarter of a Philox4x32-10, half a Box-Muller (log, sqrt, sin or cos) and the prior's
// transcendentals (mixture: exp + log; Student-t: log; Laplace: none), plus one softplus and one log per element; 8 B/element read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/btx.h"
#include "btx_rng.h"

namespace {

constexpr int KLMC_BLOCK = 256;
constexpr int KLMC_MAX_ITEMS = 48;
constexpr uint32_t KLMC_GROUP_ELEMS = KLMC_BLOCK * 4;  // elements one block covers per pass: one Philox group per thread
constexpr uint32_t KLMC_ITEM_BLOCKS = 64;              // block cap per item; larger tensors stride
constexpr float KLMC_ENTROPY_C = 1.4189385332046727f;  // (1 + log 2 pi) / 2

typedef float klmc_f32x4 __attribute__((ext_vector_type(4)));

// One batch is ONE kernel argument and has to stay under the 4-KiB kernel-argument segment: pointers and scalars in separate arrays
// (no padding), the block ranges recomputed from n in the kernel instead of stored.
struct KlMcPtrs {
  const float* mu; const float* rho; const float* loc_t;
  float* dmu; float* drho;  // backward only
  const uint32_t* sample_dev;
};
struct KlMcScalars {
  float loc, c0, c1, c2, c3;  // the prior's constants, derived on the host in double (klmc_constants)
  uint32_t n, layer, sample, type_stream;  // type | rng_stream << 8
};
struct KlMcBatchDev {
  KlMcPtrs p[KLMC_MAX_ITEMS];
  KlMcScalars s[KLMC_MAX_ITEMS];
  int n;
  int draws;
  float inv_draws;
  uint32_t k0, k1;
};
static_assert(sizeof(KlMcBatchDev) + 16 <= 4096, "the batch and the kernel's other arguments must fit the kernel-argument segment");

__host__ __device__ __forceinline__ uint32_t klmc_item_blocks(uint32_t n) {
  const uint32_t nb = (n >> 10) + ((n & (KLMC_GROUP_ELEMS - 1)) ? 1u : 0u);
  return nb > KLMC_ITEM_BLOCKS ? KLMC_ITEM_BLOCKS : nb;
}

// log p(w) (SCORE = false) or s(w) = d log p / dw (SCORE = true) at d = w - loc
template <int TYPE, bool SCORE>
__device__ __forceinline__ float klmc_prior(float d, const KlMcScalars& c) {
  if (TYPE == BTX_PRIOR_GAUSS_MIX2) {
    // c0 = log pi - log sigma1 - log(2 pi) / 2, c1 = log(1 - pi) - log sigma2 - log(2 pi) / 2, c2 = 1 / (2 sigma1^2), c3 = 1 / (2 sigma2^2)
    const float q = d * d;
    const float a = c.c0 - q * c.c2, b = c.c1 - q * c.c3;
    const float e = expf(-fabsf(a - b));  // the smaller component over the larger one: in (0, 1]
    if (!SCORE) return fmaxf(a, b) + logf(1.0f + e);  // 1 + e in [1, 2]: the absolute error stays at the rounding of the argument
    const float r_small = e / (1.0f + e), r_large = 1.0f / (1.0f + e);  // the two responsibilities
    const float ra = a >= b ? r_large : r_small, rb = a >= b ? r_small : r_large;
    return -d * (ra * (2.0f * c.c2) + rb * (2.0f * c.c3));
  } else if (TYPE == BTX_PRIOR_LAPLACE) {
    // c0 = -log(2 b), c1 = 1 / b
    if (!SCORE) return c.c0 - fabsf(d) * c.c1;
    return d > 0.0f ? -c.c1 : (d < 0.0f ? c.c1 : 0.0f);
  } else {
    // c0 = lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2 - log t, c1 = (nu + 1) / 2, c2 = 1 / (nu t^2), c3 = nu t^2
    if (!SCORE) return c.c0 - c.c1 * logf(1.0f + d * d * c.c2);  // absolute error u32 near d = 0, against a term of size |c0|
    return -(2.0f * c.c1) * d / (c.c3 + d * d);
  }
}

// The elements [4 q, 4 q + 4) of one item: forward -> the sum of their KL terms (f64); backward -> their dmu / drho stored.
template <int TYPE, bool BWD>
__device__ __forceinline__ double klmc_group(const KlMcPtrs& p, const KlMcScalars& c, const KlMcBatchDev& b, uint32_t q, uint32_t sample,
                                             bool vec_in, bool vec_out, float gn) {
  const uint32_t n = c.n;
  const size_t i0 = (size_t)q << 2;
  const bool full = i0 + 4 <= (size_t)n;
  float mu[4], rho[4], loc[4];
  if (full && vec_in) {
    const klmc_f32x4 m = *(const klmc_f32x4*)(p.mu + i0);
    const klmc_f32x4 r = *(const klmc_f32x4*)(p.rho + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) { mu[e] = m[e]; rho[e] = r[e]; loc[e] = c.loc; }
    if (p.loc_t) {
      const klmc_f32x4 l = *(const klmc_f32x4*)(p.loc_t + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) loc[e] = l[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = i0 + e < (size_t)n;
      mu[e] = in ? p.mu[i0 + e] : 0.0f;
      rho[e] = in ? p.rho[i0 + e] : 0.0f;
      loc[e] = (in && p.loc_t) ? p.loc_t[i0 + e] : c.loc;
    }
  }
  float sig[4], acc0[4], acc1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { sig[e] = log1pf(expf(rho[e])); acc0[e] = 0.0f; acc1[e] = 0.0f; }
  const uint32_t stream = c.type_stream >> 8;
  for (int j = 0; j < b.draws; ++j) {
    float z[4];
    btx_normal4(q, sample, c.layer, stream | ((uint32_t)j << 8), b.k0, b.k1, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = (mu[e] + sig[e] * z[e]) - loc[e];
      const float v = klmc_prior<TYPE, BWD>(d, c);
      acc0[e] += v;                     // forward: sum_j log p ; backward: sum_j s
      if (BWD) acc1[e] += v * z[e];     // backward: sum_j s eps_j
    }
  }
  if (!BWD) {
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float term = (-logf(sig[e]) - KLMC_ENTROPY_C) - acc0[e] * b.inv_draws;
      if (i0 + e < (size_t)n) t += (double)term;
    }
    return t;
  }
  float dmu[4], drho[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dsig = 1.0f / (1.0f + expf(-rho[e]));  // d softplus / d rho
    dmu[e] = -gn * (acc0[e] * b.inv_draws);
    drho[e] = gn * (-1.0f / sig[e] - acc1[e] * b.inv_draws) * dsig;
  }
  if (full && vec_out) {
    klmc_f32x4 m, r;
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = dmu[e]; r[e] = drho[e]; }
    *(klmc_f32x4*)(p.dmu + i0) = m;
    *(klmc_f32x4*)(p.drho + i0) = r;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < (size_t)n) { p.dmu[i0 + e] = dmu[e]; p.drho[i0 + e] = drho[e]; }
  }
  return 0.0;
}

// The groups of item `it` that fall to this block (block `blk` of the item's `nblk`), thread by thread.
template <int TYPE, bool BWD>
__device__ __forceinline__ double klmc_item(const KlMcBatchDev& b, int it, uint32_t blk, uint32_t nblk, float gn) {
  const KlMcPtrs& p = b.p[it];
  const KlMcScalars& c = b.s[it];
  uint32_t sample = c.sample;
  if (p.sample_dev) sample = __builtin_amdgcn_readfirstlane(*p.sample_dev);  // captured steps: the index lives on the device
  const bool vec_in = ((((uintptr_t)p.mu | (uintptr_t)p.rho | (uintptr_t)p.loc_t) & 15) == 0);
  const bool vec_out = BWD && ((((uintptr_t)p.dmu | (uintptr_t)p.drho) & 15) == 0);
  const uint32_t ngroups = (c.n >> 2) + ((c.n & 3u) ? 1u : 0u);
  double acc = 0.0;
  for (uint64_t q = (uint64_t)blk * KLMC_BLOCK + threadIdx.x; q < ngroups; q += (uint64_t)nblk * KLMC_BLOCK)
    acc += klmc_group<TYPE, BWD>(p, c, b, (uint32_t)q, sample, vec_in, vec_out, gn);
  return acc;
}

// Which item this block belongs to: the block ranges follow from the sizes (uniform, scalar work).
__device__ __forceinline__ int klmc_locate(const KlMcBatchDev& b, uint32_t& first, uint32_t& nblk) {
  int it = 0;
  first = 0;
  nblk = klmc_item_blocks(b.s[0].n);
  for (int j = 1; j < b.n; ++j) {
    const uint32_t start = first + nblk;
    if (blockIdx.x < start) break;
    it = j; first = start; nblk = klmc_item_blocks(b.s[j].n);
  }
  return it;
}

template <bool BWD>
__device__ __forceinline__ double klmc_dispatch(const KlMcBatchDev& b, int it, uint32_t blk, uint32_t nblk, float gn) {
  switch (b.s[it].type_stream & 0xffu) {
    case BTX_PRIOR_GAUSS_MIX2: return klmc_item<BTX_PRIOR_GAUSS_MIX2, BWD>(b, it, blk, nblk, gn);
    case BTX_PRIOR_LAPLACE: return klmc_item<BTX_PRIOR_LAPLACE, BWD>(b, it, blk, nblk, gn);
    default: return klmc_item<BTX_PRIOR_STUDENT_T, BWD>(b, it, blk, nblk, gn);
  }
}

__global__ __launch_bounds__(KLMC_BLOCK) void klmc_partial_kernel(const KlMcBatchDev b, double* __restrict__ partials) {
  uint32_t first, nblk;
  const int it = klmc_locate(b, first, nblk);
  double acc = klmc_dispatch<false>(b, it, blockIdx.x - first, nblk, 0.0f);
  // wave64 shuffle reduce -> LDS -> one value per block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double wsum[KLMC_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < KLMC_BLOCK / 64; ++w) s += wsum[w];
    // the MEAN of each tensor, the means summed (the Gaussian KL's convention): the scaling is per tensor
    partials[blockIdx.x] = s / (double)b.s[it].n;
  }
}

__global__ __launch_bounds__(KLMC_BLOCK) void klmc_bwd_kernel(const KlMcBatchDev b, const float* __restrict__ gout) {
  uint32_t first, nblk;
  const int it = klmc_locate(b, first, nblk);
  (void)klmc_dispatch<true>(b, it, blockIdx.x - first, nblk, gout[0] / (float)b.s[it].n);
}

__global__ __launch_bounds__(64) void klmc_final_kernel(const double* __restrict__ partials, int nblocks, float* __restrict__ out,
                                                        int accumulate) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) acc += partials[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) {
    const float kl = (float)acc;
    out[0] = accumulate ? out[0] + kl : kl;
  }
}

// The device constants of a prior, in double; false when a parameter is out of range (NaN included).
bool klmc_constants(const BtxPrior& pr, KlMcScalars* s) {
  const double half_log_2pi = 0.91893853320467274178;
  s->loc = pr.loc;
  s->c0 = s->c1 = s->c2 = s->c3 = 0.0f;
  if (!(pr.loc == pr.loc) || isinf(pr.loc)) return false;
  if (pr.type == BTX_PRIOR_GAUSS_MIX2) {
    const double pi = pr.p0, s1 = pr.p1, s2 = pr.p2;
    if (!(pi > 0.0 && pi < 1.0) || !(s1 > 0.0) || !(s2 > 0.0) || isinf(s1) || isinf(s2)) return false;
    s->c0 = (float)(log(pi) - log(s1) - half_log_2pi);
    s->c1 = (float)(log1p(-pi) - log(s2) - half_log_2pi);
    s->c2 = (float)(1.0 / (2.0 * s1 * s1));
    s->c3 = (float)(1.0 / (2.0 * s2 * s2));
  } else if (pr.type == BTX_PRIOR_LAPLACE) {
    const double bb = pr.p0;
    if (!(bb > 0.0) || isinf(bb)) return false;
    s->c0 = (float)(-log(2.0 * bb));
    s->c1 = (float)(1.0 / bb);
  } else {
    const double nu = pr.p0, t = pr.p1;
    if (!(nu > 0.0) || !(t > 0.0) || isinf(nu) || isinf(t)) return false;
    s->c0 = (float)(lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846) - log(t));
    s->c1 = (float)(0.5 * (nu + 1.0));
    s->c2 = (float)(1.0 / (nu * t * t));
    s->c3 = (float)(nu * t * t);
  }
  return true;
}

// Every item of the call, before anything is launched.
int klmc_validate(const BtxKlMcItem* items, int n_items, int draws, bool bwd) {
  if (!items) return BTX_E_NULL;
  if (n_items <= 0 || draws < 1 || draws >= (1 << 24)) return BTX_E_SHAPE;
  for (int i = 0; i < n_items; ++i)
    if (!items[i].mu || !items[i].rho || (bwd && (!items[i].dmu || !items[i].drho))) return BTX_E_NULL;
  KlMcScalars tmp;
  for (int i = 0; i < n_items; ++i) {
    const BtxKlMcItem& s = items[i];
    const bool known = s.prior.type == BTX_PRIOR_GAUSS_MIX2 || s.prior.type == BTX_PRIOR_LAPLACE || s.prior.type == BTX_PRIOR_STUDENT_T;
    if (s.n == 0 || s.rng_stream >= 256u || (known && !klmc_constants(s.prior, &tmp))) return BTX_E_SHAPE;
  }
  for (int i = 0; i < n_items; ++i) {
    const BtxKlMcItem& s = items[i];
    const bool known = s.prior.type == BTX_PRIOR_GAUSS_MIX2 || s.prior.type == BTX_PRIOR_LAPLACE || s.prior.type == BTX_PRIOR_STUDENT_T;
    if (!known || s.n > 0xfffffffcull) return BTX_E_UNSUPPORTED;  // BTX-RNG v1 block index is 32 bits
  }
  return 0;
}

// items [base, base + 48) -> the batch; returns its block count
uint32_t klmc_fill_batch(const BtxKlMcItem* items, int base, int n_items, uint64_t seed, int draws, KlMcBatchDev* b) {
  memset(b, 0, sizeof(*b));
  b->n = n_items - base < KLMC_MAX_ITEMS ? n_items - base : KLMC_MAX_ITEMS;
  b->draws = draws;
  b->inv_draws = (float)(1.0 / (double)draws);
  b->k0 = (uint32_t)seed;
  b->k1 = (uint32_t)(seed >> 32);
  uint32_t blocks = 0;
  for (int i = 0; i < b->n; ++i) {
    const BtxKlMcItem& s = items[base + i];
    KlMcPtrs& p = b->p[i];
    p.mu = s.mu; p.rho = s.rho; p.loc_t = s.loc_t; p.dmu = s.dmu; p.drho = s.drho; p.sample_dev = s.sample_idx_dev;
    KlMcScalars& c = b->s[i];
    klmc_constants(s.prior, &c);
    c.n = (uint32_t)s.n; c.layer = s.layer_id; c.sample = s.sample_idx;
    c.type_stream = (uint32_t)s.prior.type | (s.rng_stream << 8);
    blocks += klmc_item_blocks(c.n);
  }
  return blocks;
}

}  // namespace

extern "C" {
size_t btx_kl_mc_workspace_bytes(int n_items) {
  if (n_items <= 0) return 0;
  return (size_t)((n_items + KLMC_MAX_ITEMS - 1) / KLMC_MAX_ITEMS) * KLMC_MAX_ITEMS * KLMC_ITEM_BLOCKS * sizeof(double);
}

int btx_kl_mc_model(const BtxKlMcItem* items, int n_items, uint64_t seed, int draws, float* kl_out, uint32_t flags, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!items || !kl_out || !ws) return BTX_E_NULL;
  int rc = klmc_validate(items, n_items, draws, false);
  if (rc) return rc;
  if (ws_bytes < btx_kl_mc_workspace_bytes(n_items)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  int total = 0;
  for (int base = 0; base < n_items; base += KLMC_MAX_ITEMS) {
    KlMcBatchDev b;
    const uint32_t blocks = klmc_fill_batch(items, base, n_items, seed, draws, &b);
    hipLaunchKernelGGL(klmc_partial_kernel, dim3(blocks), dim3(KLMC_BLOCK), 0, st, b, part + total);
    total += (int)blocks;
  }
  hipLaunchKernelGGL(klmc_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, total, kl_out,
                     (flags & BTX_FLAG_KL_ACCUM) ? 1 : 0);
  return (int)hipGetLastError();
}

int btx_kl_mc_model_bwd(const BtxKlMcItem* items, int n_items, uint64_t seed, int draws, const float* grad_out, void* stream) {
  if (!items || !grad_out) return BTX_E_NULL;
  int rc = klmc_validate(items, n_items, draws, true);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < n_items; base += KLMC_MAX_ITEMS) {
    KlMcBatchDev b;
    const uint32_t blocks = klmc_fill_batch(items, base, n_items, seed, draws, &b);
    hipLaunchKernelGGL(klmc_bwd_kernel, dim3(blocks), dim3(KLMC_BLOCK), 0, st, b, grad_out);
  }
  return (int)hipGetLastError();
}
}  // extern "C"
