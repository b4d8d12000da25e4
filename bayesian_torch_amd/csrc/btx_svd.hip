// btx_svd.hip — BTX-SVD v1: sparse variational dropout (Molchanov, Ashukha & Vetrov 2017) on the additive
// (mu, sigma) parametrisation.  gfx950 only.
//
//   la    = clamp(2 log sigma - log(mu^2 + EPS), -LA_MAX, LA_MAX)          log alpha, sigma = log1p(exp(rho))
//   kl_i  = k1 - k1 sigmoid(k2 + k3 la) + 0.5 log1p(exp(-la))             KL(q || log-uniform), eq. 14 of the paper
//   kl    = sum over tensors of c sum_i kl_i,  c = 1 / n ("mean") or 1 ("sum")
//
// Four entry points over up to 48 tensors per launch: the KL (an f64 partial per block, a fixed-order fold), its backward (one
// element-wise launch, every element of dmu / drho written), the log-alpha statistics (integer counters: exact in any order) and
// pruning in place.  Nothing is sampled, nothing saved.  Traffic is 8 B/element read (16 B with the backward's writes), but the pass is
// bound by its per-element VALU work, not by HBM: three logf, three expf, a log1pf and a division forward (the backward: two logf, four
// expf, a log1pf, five divisions) — measured 0.98 TB/s forward on ResNet18's 11.7 M elements (profiles/svd_bench.txt).  Built with
// -ffp-contract=off: every f32 step is its own rounded operation, so the vector and the scalar access paths give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/btx.h"
#include "btx_heads.h"  // wave_sum, block_sum_pairwise4

namespace {

constexpr int SVD_BLOCK = 256;
constexpr int SVD_MAX_ITEMS = 48;
constexpr uint32_t SVD_GROUP_ELEMS = SVD_BLOCK * 4;  // elements one block covers per pass: four consecutive ones per thread
constexpr uint32_t SVD_ITEM_BLOCKS = 256;            // block cap per item (one per CU); larger tensors stride
constexpr int SVD_MAX_BINS = 4096;
constexpr float SVD_EPS = 1e-8f;
constexpr float SVD_LA_MAX = 20.0f;
constexpr float SVD_K1 = 0.63576f, SVD_K2 = 1.87320f, SVD_K3 = 1.48695f;
constexpr float SVD_RHO_PRUNED = -40.0f;

typedef float svd_f32x4 __attribute__((ext_vector_type(4)));

// One batch is ONE kernel argument (under the 4-KiB kernel-argument segment); the block ranges are recomputed from n in the kernel.
struct SvdBatchDev {
  float* mu[SVD_MAX_ITEMS];
  float* rho[SVD_MAX_ITEMS];
  float* dmu[SVD_MAX_ITEMS];   // backward only
  float* drho[SVD_MAX_ITEMS];  // backward only
  uint32_t n[SVD_MAX_ITEMS];
  uint32_t sum[SVD_MAX_ITEMS];  // 1: reduction "sum", 0: "mean"
  int count;
};
struct SvdThresholds { float t[BTX_LOGALPHA_MAX_THRESHOLDS]; };
static_assert(sizeof(SvdBatchDev) + sizeof(SvdThresholds) + 64 <= 4096,
              "the batch and the kernel's other arguments must fit the kernel-argument segment");

__host__ __device__ __forceinline__ uint32_t svd_item_blocks(uint32_t n) {
  const uint32_t nb = (n >> 10) + ((n & (SVD_GROUP_ELEMS - 1)) ? 1u : 0u);
  return nb > SVD_ITEM_BLOCKS ? SVD_ITEM_BLOCKS : nb;
}

__device__ __forceinline__ float svd_la_raw(float mu, float rho) {
  const float sig = log1pf(expf(rho));  // 0 once exp(rho) underflows: log gives -inf and the clamp -LA_MAX
  return 2.0f * logf(sig) - logf(mu * mu + SVD_EPS);
}
__device__ __forceinline__ float svd_clamp(float la_raw) { return fminf(fmaxf(la_raw, -SVD_LA_MAX), SVD_LA_MAX); }

__device__ __forceinline__ float svd_kl_term(float la) {
  const float s = 1.0f / (1.0f + expf(-(SVD_K2 + SVD_K3 * la)));
  // logf(1 + z), not log1pf(z): the term is judged on its ABSOLUTE error (k1 - k1 s next to it rounds at 2^-24 k1 whatever la is), which
  // the rounding of 1 + z already sets; logf is the function whose device error tests/envelope.py measured
  return (SVD_K1 - SVD_K1 * s) + 0.5f * logf(1.0f + expf(-la));
}

// d kl_i / d(mu, rho) times gc; both 0 where la_raw lies strictly outside [-LA_MAX, LA_MAX] (a select, not a product: sigma == 0
// makes the rho factor 0 / 0)
__device__ __forceinline__ void svd_kl_grad(float mu, float rho, float gc, float& dmu, float& drho) {
  const float sig = log1pf(expf(rho));
  const float m2 = mu * mu + SVD_EPS;
  const float la_raw = 2.0f * logf(sig) - logf(m2);
  const float la = svd_clamp(la_raw);
  const float s = 1.0f / (1.0f + expf(-(SVD_K2 + SVD_K3 * la)));
  const float sn = 1.0f / (1.0f + expf(la));  // sigmoid(-la)
  const float d = -((SVD_K1 * SVD_K3) * s * (1.0f - s) + 0.5f * sn);
  const float dsig = 1.0f / (1.0f + expf(-rho));  // d softplus / d rho
  const bool pass = la_raw >= -SVD_LA_MAX && la_raw <= SVD_LA_MAX;
  dmu = pass ? gc * (d * (-2.0f * mu / m2)) : 0.0f;
  drho = pass ? gc * (d * (2.0f * dsig / sig)) : 0.0f;
}

// Which item this block belongs to: the block ranges follow from the sizes (uniform, scalar work).
__device__ __forceinline__ int svd_locate(const SvdBatchDev& b, uint32_t& first, uint32_t& nblk) {
  int it = 0;
  first = 0;
  nblk = svd_item_blocks(b.n[0]);
  for (int j = 1; j < b.count; ++j) {
    const uint32_t start = first + nblk;
    if (blockIdx.x < start) break;
    it = j; first = start; nblk = svd_item_blocks(b.n[j]);
  }
  return it;
}

// The elements [4 q, 4 q + 4) of an item: one 16-byte load per tensor on the grid, element by element off it or at the ragged tail
// (elements past n read as mu = 1, rho = 0 and are never counted or stored).
__device__ __forceinline__ void svd_load4(const float* mu, const float* rho, uint32_t n, size_t i0, bool vec, float* m, float* r) {
  if (vec && i0 + 4 <= (size_t)n) {
    const svd_f32x4 a = *(const svd_f32x4*)(mu + i0);
    const svd_f32x4 c = *(const svd_f32x4*)(rho + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) { m[e] = a[e]; r[e] = c[e]; }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = i0 + e < (size_t)n;
      m[e] = in ? mu[i0 + e] : 1.0f;
      r[e] = in ? rho[i0 + e] : 0.0f;
    }
  }
}
__device__ __forceinline__ void svd_store4(float* a, float* c, uint32_t n, size_t i0, bool vec, const float* va, const float* vc) {
  if (vec && i0 + 4 <= (size_t)n) {
    svd_f32x4 x, y;
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = va[e]; y[e] = vc[e]; }
    *(svd_f32x4*)(a + i0) = x;
    *(svd_f32x4*)(c + i0) = y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < (size_t)n) { a[i0 + e] = va[e]; c[i0 + e] = vc[e]; }
  }
}
__device__ __forceinline__ bool svd_on_grid(const void* a, const void* c) { return ((((uintptr_t)a | (uintptr_t)c) & 15) == 0); }

__global__ __launch_bounds__(SVD_BLOCK) void svd_kl_partial_kernel(const SvdBatchDev b, double* __restrict__ partials) {
  uint32_t first, nblk;
  const int it = svd_locate(b, first, nblk);
  const float* mu = b.mu[it];
  const float* rho = b.rho[it];
  const uint32_t n = b.n[it];
  const bool vec = svd_on_grid(mu, rho);
  const uint32_t ngroups = (n >> 2) + ((n & 3u) ? 1u : 0u);
  double acc = 0.0;
  for (uint64_t q = (uint64_t)(blockIdx.x - first) * SVD_BLOCK + threadIdx.x; q < ngroups; q += (uint64_t)nblk * SVD_BLOCK) {
    const size_t i0 = (size_t)q << 2;
    float m[4], r[4];
    svd_load4(mu, rho, n, i0, vec, m, r);
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float term = svd_kl_term(svd_clamp(svd_la_raw(m[e], r[e])));
      if (i0 + e < (size_t)n) t += (double)term;
    }
    acc += t;
  }
  __shared__ double part[4];
  const double s = block_sum_pairwise4(acc, part);
  // "mean": the mean of each tensor, the means summed (the Gaussian KL's convention); "sum": the ELBO's KL
  if (threadIdx.x == 0) partials[blockIdx.x] = b.sum[it] ? s : s / (double)n;
}

// One wave folds the batch: per item its blocks' partials (lane-strided, then the butterfly: a function of n alone), the items in
// index order on top of the running total of the earlier batches (`carry`).  The last batch writes kl_out.
__global__ __launch_bounds__(64) void svd_kl_fold_kernel(const SvdBatchDev b, const double* __restrict__ partials, double* __restrict__ carry,
                                                         double* __restrict__ terms, int is_first, int is_last,
                                                         float* __restrict__ out, int accumulate) {
  double total = is_first ? 0.0 : carry[0];
  uint32_t first = 0;
  for (int it = 0; it < b.count; ++it) {
    const uint32_t nblk = svd_item_blocks(b.n[it]);
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < nblk; i += 64) acc += partials[first + i];
    acc = wave_sum(acc);
    if (terms && threadIdx.x == 0) terms[it] = acc;
    total += acc;
    first += nblk;
  }
  if (threadIdx.x == 0) {
    if (is_last) {
      const float kl = (float)total;
      out[0] = accumulate ? out[0] + kl : kl;
    } else {
      carry[0] = total;
    }
  }
}

__global__ __launch_bounds__(SVD_BLOCK) void svd_kl_bwd_kernel(const SvdBatchDev b, const float* __restrict__ gout) {
  uint32_t first, nblk;
  const int it = svd_locate(b, first, nblk);
  const float* mu = b.mu[it];
  const float* rho = b.rho[it];
  float* dmu = b.dmu[it];
  float* drho = b.drho[it];
  const uint32_t n = b.n[it];
  const float gc = b.sum[it] ? gout[0] : gout[0] / (float)n;
  const bool vec_in = svd_on_grid(mu, rho), vec_out = svd_on_grid(dmu, drho);
  const uint32_t ngroups = (n >> 2) + ((n & 3u) ? 1u : 0u);
  for (uint64_t q = (uint64_t)(blockIdx.x - first) * SVD_BLOCK + threadIdx.x; q < ngroups; q += (uint64_t)nblk * SVD_BLOCK) {
    const size_t i0 = (size_t)q << 2;
    float m[4], r[4], gm[4], gr[4];
    svd_load4(mu, rho, n, i0, vec_in, m, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) svd_kl_grad(m[e], r[e], gc, gm[e], gr[e]);
    svd_store4(dmu, drho, n, i0, vec_out, gm, gr);
  }
}

// Per item: out[0 .. 8) = count(la > t_k) (unused thresholds are +inf), out[8] = count(mu == 0); hist[b] when bins > 0.  Per-thread
// counters, folded per block (below), then one 64-bit integer atomic per block and counter; the histogram in LDS first.
__global__ __launch_bounds__(SVD_BLOCK) void svd_stats_kernel(const SvdBatchDev b, const SvdThresholds th, int bins,
                                                              unsigned long long* __restrict__ out,
                                                              unsigned long long* __restrict__ hist) {
  __shared__ uint32_t lhist[SVD_MAX_BINS];
  uint32_t first, nblk;
  const int it = svd_locate(b, first, nblk);
  const float* mu = b.mu[it];
  const float* rho = b.rho[it];
  const uint32_t n = b.n[it];
  const bool vec = svd_on_grid(mu, rho);
  const uint32_t ngroups = (n >> 2) + ((n & 3u) ? 1u : 0u);
  if (bins > 0) {
    for (int i = threadIdx.x; i < bins; i += SVD_BLOCK) lhist[i] = 0u;
    __syncthreads();
  }
  const float bscale = (float)bins;
  int cnt[BTX_LOGALPHA_MAX_THRESHOLDS + 1];
#pragma unroll
  for (int k = 0; k <= BTX_LOGALPHA_MAX_THRESHOLDS; ++k) cnt[k] = 0;
  for (uint64_t q = (uint64_t)(blockIdx.x - first) * SVD_BLOCK + threadIdx.x; q < ngroups; q += (uint64_t)nblk * SVD_BLOCK) {
    const size_t i0 = (size_t)q << 2;
    float m[4], r[4];
    svd_load4(mu, rho, n, i0, vec, m, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e >= (size_t)n) continue;
      const float la = svd_clamp(svd_la_raw(m[e], r[e]));
#pragma unroll
      for (int k = 0; k < BTX_LOGALPHA_MAX_THRESHOLDS; ++k) cnt[k] += la > th.t[k] ? 1 : 0;
      cnt[BTX_LOGALPHA_MAX_THRESHOLDS] += m[e] == 0.0f ? 1 : 0;
      if (bins > 0) {
        int bin = (int)floorf((la + SVD_LA_MAX) * bscale / (2.0f * SVD_LA_MAX));
        bin = bin > bins - 1 ? bins - 1 : (bin < 0 ? 0 : bin);
        atomicAdd(&lhist[bin], 1u);
      }
    }
  }
  // the block's counters: the butterfly per wave, the four waves in LDS, then ONE 64-bit atomic per block and counter
  __shared__ int bcnt[SVD_BLOCK / 64][BTX_LOGALPHA_MAX_THRESHOLDS + 1];
#pragma unroll
  for (int k = 0; k <= BTX_LOGALPHA_MAX_THRESHOLDS; ++k) {
    const int c = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0) bcnt[threadIdx.x >> 6][k] = c;
  }
  __syncthreads();
  if (threadIdx.x <= BTX_LOGALPHA_MAX_THRESHOLDS) {
    const int c = (bcnt[0][threadIdx.x] + bcnt[1][threadIdx.x]) + (bcnt[2][threadIdx.x] + bcnt[3][threadIdx.x]);
    if (c) atomicAdd(out + (size_t)it * BTX_LOGALPHA_STATS_WORDS + threadIdx.x, (unsigned long long)c);
  }
  if (bins > 0) {
    for (int i = threadIdx.x; i < bins; i += SVD_BLOCK) {
      const uint32_t c = lhist[i];
      if (c) atomicAdd(hist + (size_t)it * bins + i, (unsigned long long)c);
    }
  }
}

// mu = 0, rho = RHO_PRUNED wherever la > t; out[0] of the item = how many.  A group is stored only when one of its elements changed.
__global__ __launch_bounds__(SVD_BLOCK) void svd_prune_kernel(const SvdBatchDev b, float t, unsigned long long* __restrict__ out) {
  uint32_t first, nblk;
  const int it = svd_locate(b, first, nblk);
  float* mu = b.mu[it];
  float* rho = b.rho[it];
  const uint32_t n = b.n[it];
  const bool vec = svd_on_grid(mu, rho);
  const uint32_t ngroups = (n >> 2) + ((n & 3u) ? 1u : 0u);
  int cnt = 0;
  for (uint64_t q = (uint64_t)(blockIdx.x - first) * SVD_BLOCK + threadIdx.x; q < ngroups; q += (uint64_t)nblk * SVD_BLOCK) {
    const size_t i0 = (size_t)q << 2;
    float m[4], r[4];
    svd_load4(mu, rho, n, i0, vec, m, r);
    int hit = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool p = i0 + e < (size_t)n && svd_clamp(svd_la_raw(m[e], r[e])) > t;
      if (p) { m[e] = 0.0f; r[e] = SVD_RHO_PRUNED; ++hit; }
    }
    if (hit) svd_store4(mu, rho, n, i0, vec, m, r);
    cnt += hit;
  }
  const int c = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out + (size_t)it * BTX_LOGALPHA_STATS_WORDS, (unsigned long long)c);
}

// Every item of a KL call, before anything is launched.
int svd_validate_kl(const BtxKlLogUItem* items, int n_items, bool bwd) {
  if (!items) return BTX_E_NULL;
  if (n_items < 1) return BTX_E_SHAPE;
  for (int i = 0; i < n_items; ++i)
    if (!items[i].mu || !items[i].rho || (bwd && (!items[i].dmu || !items[i].drho))) return BTX_E_NULL;
  for (int i = 0; i < n_items; ++i)
    if (items[i].n == 0 || (items[i].reduction != BTX_REDUCE_MEAN && items[i].reduction != BTX_REDUCE_SUM)) return BTX_E_SHAPE;
  for (int i = 0; i < n_items; ++i)
    if (items[i].n > 0xfffffffcull) return BTX_E_UNSUPPORTED;  // element counts are 32 bits on the device
  return 0;
}

int svd_validate_la(const BtxLogAlphaItem* items, int n_items) {
  if (!items) return BTX_E_NULL;
  if (n_items < 1) return BTX_E_SHAPE;
  for (int i = 0; i < n_items; ++i)
    if (!items[i].mu || !items[i].rho) return BTX_E_NULL;
  for (int i = 0; i < n_items; ++i)
    if (items[i].n == 0) return BTX_E_SHAPE;
  for (int i = 0; i < n_items; ++i)
    if (items[i].n > 0xfffffffcull) return BTX_E_UNSUPPORTED;
  return 0;
}

// items [base, base + 48) -> the batch; returns its block count
uint32_t svd_fill_kl(const BtxKlLogUItem* items, int base, int n_items, SvdBatchDev* b) {
  memset(b, 0, sizeof(*b));
  b->count = n_items - base < SVD_MAX_ITEMS ? n_items - base : SVD_MAX_ITEMS;
  uint32_t blocks = 0;
  for (int i = 0; i < b->count; ++i) {
    const BtxKlLogUItem& s = items[base + i];
    b->mu[i] = const_cast<float*>(s.mu); b->rho[i] = const_cast<float*>(s.rho); b->dmu[i] = s.dmu; b->drho[i] = s.drho;
    b->n[i] = (uint32_t)s.n; b->sum[i] = s.reduction == BTX_REDUCE_SUM ? 1u : 0u;
    blocks += svd_item_blocks(b->n[i]);
  }
  return blocks;
}
uint32_t svd_fill_la(const BtxLogAlphaItem* items, int base, int n_items, SvdBatchDev* b) {
  memset(b, 0, sizeof(*b));
  b->count = n_items - base < SVD_MAX_ITEMS ? n_items - base : SVD_MAX_ITEMS;
  uint32_t blocks = 0;
  for (int i = 0; i < b->count; ++i) {
    b->mu[i] = items[base + i].mu; b->rho[i] = items[base + i].rho; b->n[i] = (uint32_t)items[base + i].n;
    blocks += svd_item_blocks(b->n[i]);
  }
  return blocks;
}

}  // namespace

extern "C" {
size_t btx_kl_logu_workspace_bytes(int n_items) {
  if (n_items <= 0) return 0;
  // the running total of the earlier batches, then a partial per block
  return (size_t)(1 + (size_t)((n_items + SVD_MAX_ITEMS - 1) / SVD_MAX_ITEMS) * SVD_MAX_ITEMS * SVD_ITEM_BLOCKS) * sizeof(double);
}

int btx_kl_logu_model(const BtxKlLogUItem* items, int n_items, float* kl_out, double* terms_out, uint32_t flags, void* ws,
                      size_t ws_bytes, void* stream) {
  if (!items || !kl_out || !ws) return BTX_E_NULL;
  int rc = svd_validate_kl(items, n_items, false);
  if (rc) return rc;
  if (ws_bytes < btx_kl_logu_workspace_bytes(n_items)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws & 7) != 0 || ((uintptr_t)terms_out & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  double* carry = (double*)ws;
  double* part = carry + 1;
  for (int base = 0; base < n_items; base += SVD_MAX_ITEMS) {
    SvdBatchDev b;
    const uint32_t blocks = svd_fill_kl(items, base, n_items, &b);
    hipLaunchKernelGGL(svd_kl_partial_kernel, dim3(blocks), dim3(SVD_BLOCK), 0, st, b, part);
    hipLaunchKernelGGL(svd_kl_fold_kernel, dim3(1), dim3(64), 0, st, b, (const double*)part, carry,
                       terms_out ? terms_out + base : (double*)nullptr, base == 0 ? 1 : 0, base + SVD_MAX_ITEMS >= n_items ? 1 : 0,
                       kl_out, (flags & BTX_FLAG_KL_ACCUM) ? 1 : 0);
    part += blocks;
  }
  return (int)hipGetLastError();
}

int btx_kl_logu_model_bwd(const BtxKlLogUItem* items, int n_items, const float* grad_out, void* stream) {
  if (!items || !grad_out) return BTX_E_NULL;
  int rc = svd_validate_kl(items, n_items, true);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < n_items; base += SVD_MAX_ITEMS) {
    SvdBatchDev b;
    const uint32_t blocks = svd_fill_kl(items, base, n_items, &b);
    hipLaunchKernelGGL(svd_kl_bwd_kernel, dim3(blocks), dim3(SVD_BLOCK), 0, st, b, grad_out);
  }
  return (int)hipGetLastError();
}

int btx_logalpha_stats(const BtxLogAlphaItem* items, int n_items, const float* thresholds, int n_thresholds, int bins,
                       uint64_t* stats_out, uint64_t* hist_out, void* stream) {
  if (!items || !stats_out || (n_thresholds > 0 && !thresholds) || (bins > 0 && !hist_out)) return BTX_E_NULL;
  int rc = svd_validate_la(items, n_items);
  if (rc) return rc;
  if (n_thresholds < 0 || n_thresholds > BTX_LOGALPHA_MAX_THRESHOLDS || bins < 0 || bins > SVD_MAX_BINS) return BTX_E_SHAPE;
  for (int k = 0; k < n_thresholds; ++k)
    if (thresholds[k] != thresholds[k]) return BTX_E_SHAPE;  // NaN
  if (((uintptr_t)stats_out & 7) != 0 || ((uintptr_t)hist_out & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  SvdThresholds th;
  for (int k = 0; k < BTX_LOGALPHA_MAX_THRESHOLDS; ++k) th.t[k] = k < n_thresholds ? thresholds[k] : INFINITY;
  rc = (int)hipMemsetAsync(stats_out, 0, (size_t)n_items * BTX_LOGALPHA_STATS_WORDS * sizeof(uint64_t), st);
  if (rc) return rc;
  if (bins > 0) {
    rc = (int)hipMemsetAsync(hist_out, 0, (size_t)n_items * (size_t)bins * sizeof(uint64_t), st);
    if (rc) return rc;
  }
  for (int base = 0; base < n_items; base += SVD_MAX_ITEMS) {
    SvdBatchDev b;
    const uint32_t blocks = svd_fill_la(items, base, n_items, &b);
    hipLaunchKernelGGL(svd_stats_kernel, dim3(blocks), dim3(SVD_BLOCK), 0, st, b, th, bins,
                       (unsigned long long*)stats_out + (size_t)base * BTX_LOGALPHA_STATS_WORDS,
                       bins > 0 ? (unsigned long long*)hist_out + (size_t)base * bins : (unsigned long long*)nullptr);
  }
  return (int)hipGetLastError();
}

int btx_logalpha_prune(const BtxLogAlphaItem* items, int n_items, float threshold, uint64_t* stats_out, void* stream) {
  if (!items || !stats_out) return BTX_E_NULL;
  int rc = svd_validate_la(items, n_items);
  if (rc) return rc;
  if (threshold != threshold) return BTX_E_SHAPE;
  if (((uintptr_t)stats_out & 7) != 0) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  rc = (int)hipMemsetAsync(stats_out, 0, (size_t)n_items * BTX_LOGALPHA_STATS_WORDS * sizeof(uint64_t), st);
  if (rc) return rc;
  for (int base = 0; base < n_items; base += SVD_MAX_ITEMS) {
    SvdBatchDev b;
    const uint32_t blocks = svd_fill_la(items, base, n_items, &b);
    hipLaunchKernelGGL(svd_prune_kernel, dim3(blocks), dim3(SVD_BLOCK), 0, st, b, threshold,
                       (unsigned long long*)stats_out + (size_t)base * BTX_LOGALPHA_STATS_WORDS);
  }
  return (int)hipGetLastError();
}
}  // extern "C"
