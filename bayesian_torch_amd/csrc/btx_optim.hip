// btx_optim.hip — K11: the parameter update of SGD / Adam / AdamW and the global gradient norm (include/btx.h, DESIGN.md §14
// "BTX-OPT v1").  HBM-bound, one pass: read p, g and the state, write p and the state (28 B/element for Adam, 16 - 20 for SGD).
// Built with -ffp-contract=off: every f32 operation below is rounded once, exactly as tests/optim_model.py spells it.  gfx950 only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/btx.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int OPT_BLOCK = 256;
constexpr int OPT_CHUNK = BTX_OPTIM_CHUNK;  // elements a workgroup owns: 4 x float4 per thread
constexpr int OPT_MAX_ITEMS = 48;           // per launch: the table travels by value in the kernel arguments (KlBatchDev pattern)
static_assert(OPT_CHUNK % (OPT_BLOCK * 4) == 0, "a chunk is a whole number of float4 sweeps");

struct OptItemDev {
  float* p; const float* g; float* s0; float* s1;
  uint64_t n;
  uint32_t first_block, pad;
};
struct OptBatchDev {
  OptItemDev it[OPT_MAX_ITEMS];
  int n;
  uint32_t total_blocks;
};

// the item that owns this workgroup, and the workgroup's element range [lo, hi) inside it
__device__ __forceinline__ const OptItemDev& opt_find(const OptBatchDev& b, size_t* lo, size_t* hi) {
  int i = 0;
  for (int j = 1; j < b.n; ++j)
    if (blockIdx.x >= b.it[j].first_block) i = j;
  const OptItemDev& it = b.it[i];
  *lo = (size_t)(blockIdx.x - it.first_block) * OPT_CHUNK;
  const size_t end = *lo + OPT_CHUNK;
  *hi = end < it.n ? end : (size_t)it.n;
  return it;
}

struct Hyper {
  float neg_lr, wd, decay_mul, one_m_b1, b2, one_m_b2, eps, neg_step_size, bc2s, momentum, one_m_damp, s;
  bool maximize, nesterov, decoupled, first, coupled, clip;
};
__device__ __forceinline__ Hyper load_hyper(const BtxOptimHyper* __restrict__ hp, const float* __restrict__ coef) {
  Hyper h;
  h.neg_lr = hp->neg_lr; h.wd = hp->wd; h.decay_mul = hp->decay_mul; h.one_m_b1 = hp->one_m_b1; h.b2 = hp->b2;
  h.one_m_b2 = hp->one_m_b2; h.eps = hp->eps; h.neg_step_size = hp->neg_step_size; h.bc2s = hp->bc2s; h.momentum = hp->momentum;
  h.one_m_damp = hp->one_m_damp;
  const uint32_t f = hp->flags;
  h.maximize = f & BTX_OPT_MAXIMIZE; h.nesterov = f & BTX_OPT_NESTEROV; h.decoupled = f & BTX_OPT_DECOUPLED;
  h.first = f & BTX_OPT_FIRST_STEP; h.coupled = f & BTX_OPT_COUPLED_WD;
  h.clip = coef != nullptr;
  h.s = coef ? coef[0] : 1.0f;
  return h;
}

// BTX-OPT v1, gradient preamble: maximize, clip coefficient, coupled weight decay
__device__ __forceinline__ float opt_grad(const Hyper& h, float g, float p) {
  if (h.maximize) g = -g;
  if (h.clip) g = g * h.s;
  if (h.coupled) g = g + h.wd * p;
  return g;
}

__device__ __forceinline__ void adam_elem(const Hyper& h, float& p, float g, float& m, float& v) {
  g = opt_grad(h, g, p);
  if (h.decoupled) p = p * h.decay_mul;
  m = m + h.one_m_b1 * (g - m);
  v = h.b2 * v + (h.one_m_b2 * g) * g;
  const float den = sqrtf(v) / h.bc2s + h.eps;
  p = p + (h.neg_step_size * m) / den;
}

template <bool MOM>
__device__ __forceinline__ void sgd_elem(const Hyper& h, float& p, float g, float& buf) {
  g = opt_grad(h, g, p);
  if (MOM) {
    buf = h.first ? g : h.momentum * buf + h.one_m_damp * g;
    g = h.nesterov ? g + h.momentum * buf : buf;
  }
  p = p + h.neg_lr * g;
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_adam_kernel(const OptBatchDev b, const BtxOptimHyper* __restrict__ hp,
                                                               const float* __restrict__ coef) {
  size_t lo, hi;
  const OptItemDev& it = opt_find(b, &lo, &hi);
  const Hyper h = load_hyper(hp, coef);
  float* __restrict__ P = it.p; const float* __restrict__ G = it.g; float* __restrict__ M = it.s0; float* __restrict__ V = it.s1;
  size_t k = lo;
  if (((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15) == 0)) {  // lo is a multiple of 4: alignment carries over
    const size_t nv = (hi - lo) >> 2;
    for (size_t q = threadIdx.x; q < nv; q += OPT_BLOCK) {
      const size_t e = lo + (q << 2);
      f32x4 p = *(const f32x4*)(P + e), m = *(const f32x4*)(M + e), v = *(const f32x4*)(V + e);
      const f32x4 g = *(const f32x4*)(G + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_elem(h, pj, g[j], mj, vj);
        p[j] = pj; m[j] = mj; v[j] = vj;
      }
      *(f32x4*)(P + e) = p; *(f32x4*)(M + e) = m; *(f32x4*)(V + e) = v;
    }
    k = lo + (nv << 2);
  }
  for (size_t e = k + threadIdx.x; e < hi; e += OPT_BLOCK) {  // unaligned items, and the tail of aligned ones
    float p = P[e], m = M[e], v = V[e];
    adam_elem(h, p, G[e], m, v);
    P[e] = p; M[e] = m; V[e] = v;
  }
}

template <bool MOM>
__global__ __launch_bounds__(OPT_BLOCK) void optim_sgd_kernel(const OptBatchDev b, const BtxOptimHyper* __restrict__ hp,
                                                              const float* __restrict__ coef) {
  size_t lo, hi;
  const OptItemDev& it = opt_find(b, &lo, &hi);
  const Hyper h = load_hyper(hp, coef);
  float* __restrict__ P = it.p; const float* __restrict__ G = it.g; float* __restrict__ B = it.s0;
  size_t k = lo;
  if (((((uintptr_t)P | (uintptr_t)G | (MOM ? (uintptr_t)B : 0)) & 15) == 0)) {
    const size_t nv = (hi - lo) >> 2;
    for (size_t q = threadIdx.x; q < nv; q += OPT_BLOCK) {
      const size_t e = lo + (q << 2);
      f32x4 p = *(const f32x4*)(P + e);
      const f32x4 g = *(const f32x4*)(G + e);
      f32x4 bf = {0.f, 0.f, 0.f, 0.f};
      if (MOM && !h.first) bf = *(const f32x4*)(B + e);  // the first step never reads the (uninitialised) buffer
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], bj = bf[j];
        sgd_elem<MOM>(h, pj, g[j], bj);
        p[j] = pj; bf[j] = bj;
      }
      *(f32x4*)(P + e) = p;
      if (MOM) *(f32x4*)(B + e) = bf;
    }
    k = lo + (nv << 2);
  }
  for (size_t e = k + threadIdx.x; e < hi; e += OPT_BLOCK) {
    float p = P[e], bj = (MOM && !h.first) ? B[e] : 0.f;
    sgd_elem<MOM>(h, p, G[e], bj);
    P[e] = p;
    if (MOM) B[e] = bj;
  }
}

// sum of squares of one chunk: each lane sums its own squares in f32 (in element order), the lanes are folded in f64 in a fixed
// order (wave shuffle tree, then the 4 waves in order)
__global__ __launch_bounds__(OPT_BLOCK) void optim_sumsq_kernel(const OptBatchDev b, double* __restrict__ partials) {
  size_t lo, hi;
  const OptItemDev& it = opt_find(b, &lo, &hi);
  const float* __restrict__ G = it.g;
  float s = 0.f;
  size_t k = lo;
  if (((uintptr_t)G & 15) == 0) {
    const size_t nv = (hi - lo) >> 2;
    for (size_t q = threadIdx.x; q < nv; q += OPT_BLOCK) {
      const f32x4 g = *(const f32x4*)(G + lo + (q << 2));
#pragma unroll
      for (int j = 0; j < 4; ++j) s = s + g[j] * g[j];
    }
    k = lo + (nv << 2);
  }
  for (size_t e = k + threadIdx.x; e < hi; e += OPT_BLOCK) s = s + G[e] * G[e];
  double acc = (double)s;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double wsum[OPT_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < OPT_BLOCK / 64; ++w) t += wsum[w];
    partials[blockIdx.x] = t;
  }
}

// one block folds the partials in a fixed order and writes total_norm and the clip coefficient
__global__ __launch_bounds__(OPT_BLOCK) void optim_norm_final_kernel(const double* __restrict__ partials, uint32_t n, float max_norm,
                                                                     float* __restrict__ out) {
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += OPT_BLOCK) acc += partials[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double wsum[OPT_BLOCK / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < OPT_BLOCK / 64; ++w) t += wsum[w];
    const float total = (float)sqrt(t);
    const float c = max_norm / (total + 1e-6f);
    out[0] = total;
    out[1] = c < 1.0f ? c : 1.0f;
  }
}

// what each entry point needs of an item: bit 0 state0, bit 1 state1
int opt_validate(const BtxOptimItem* items, int n_items, int need) {
  if (n_items < 0) return BTX_E_SHAPE;
  if (n_items > BTX_OPTIM_MAX_ITEMS) return BTX_E_UNSUPPORTED;
  if (n_items > 0 && !items) return BTX_E_NULL;
  for (int i = 0; i < n_items; ++i) {
    const BtxOptimItem& s = items[i];
    if (s.n < 0) return BTX_E_SHAPE;
    if (s.n == 0) continue;
    if (!s.g || ((need & 4) && !s.p) || ((need & 1) && !s.state0) || ((need & 2) && !s.state1)) return BTX_E_NULL;
    uintptr_t a = (uintptr_t)s.g;
    if (need & 4) a |= (uintptr_t)s.p;
    if (need & 1) a |= (uintptr_t)s.state0;
    if (need & 2) a |= (uintptr_t)s.state1;
    if (a & 3) return BTX_E_ALIGN;
  }
  return 0;
}

// the next table of at most OPT_MAX_ITEMS non-empty items starting at *pos; false when none is left
bool opt_next_batch(const BtxOptimItem* items, int n_items, int* pos, OptBatchDev* b) {
  memset(b, 0, sizeof(*b));
  uint32_t blocks = 0;
  int i = *pos;
  for (; i < n_items && b->n < OPT_MAX_ITEMS; ++i) {
    const BtxOptimItem& s = items[i];
    if (s.n == 0) continue;
    const uint64_t nb = ((uint64_t)s.n + OPT_CHUNK - 1) / OPT_CHUNK;
    if (blocks + nb > 0x7fffffffull) break;  // the grid of one launch: the rest goes to the next table
    OptItemDev& it = b->it[b->n++];
    it.p = s.p; it.g = s.g; it.s0 = s.state0; it.s1 = s.state1; it.n = (uint64_t)s.n; it.first_block = blocks;
    blocks += (uint32_t)nb;
  }
  *pos = i;
  b->total_blocks = blocks;
  return b->n > 0;
}

}  // namespace

extern "C" {

int btx_optim_adam(const BtxOptimItem* items, int n_items, const BtxOptimHyper* hyper_dev, const float* coef_dev, void* stream) {
  if (!hyper_dev) return BTX_E_NULL;
  if (((uintptr_t)hyper_dev & 15) || ((uintptr_t)coef_dev & 3)) return BTX_E_ALIGN;
  const int rc = opt_validate(items, n_items, 4 | 3);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  OptBatchDev b;
  bool any = false;
  for (int pos = 0; opt_next_batch(items, n_items, &pos, &b); any = true)
    hipLaunchKernelGGL(optim_adam_kernel, dim3(b.total_blocks), dim3(OPT_BLOCK), 0, st, b, hyper_dev, coef_dev);
  return any ? (int)hipGetLastError() : 0;
}

int btx_optim_sgd(const BtxOptimItem* items, int n_items, const BtxOptimHyper* hyper_dev, int has_momentum, const float* coef_dev,
                  void* stream) {
  if (!hyper_dev) return BTX_E_NULL;
  if (((uintptr_t)hyper_dev & 15) || ((uintptr_t)coef_dev & 3)) return BTX_E_ALIGN;
  const int rc = opt_validate(items, n_items, 4 | (has_momentum ? 1 : 0));
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  OptBatchDev b;
  bool any = false;
  for (int pos = 0; opt_next_batch(items, n_items, &pos, &b); any = true) {
    if (has_momentum)
      hipLaunchKernelGGL(optim_sgd_kernel<true>, dim3(b.total_blocks), dim3(OPT_BLOCK), 0, st, b, hyper_dev, coef_dev);
    else
      hipLaunchKernelGGL(optim_sgd_kernel<false>, dim3(b.total_blocks), dim3(OPT_BLOCK), 0, st, b, hyper_dev, coef_dev);
  }
  return any ? (int)hipGetLastError() : 0;
}

size_t btx_optim_grad_norm_workspace_bytes(int n_items, int64_t total_elements) {
  if (n_items <= 0 || total_elements <= 0) return sizeof(double);
  return ((size_t)(total_elements / OPT_CHUNK) + (size_t)n_items) * sizeof(double);  // >= sum of ceil(n_i / chunk)
}

int btx_optim_grad_norm(const BtxOptimItem* items, int n_items, float max_norm, float* out_dev, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!out_dev || !ws) return BTX_E_NULL;
  if (!(max_norm > 0.0f)) return BTX_E_SHAPE;
  if (((uintptr_t)out_dev & 3) || ((uintptr_t)ws & 7)) return BTX_E_ALIGN;
  const int rc = opt_validate(items, n_items, 0);
  if (rc) return rc;
  uint64_t chunks = 0;
  for (int i = 0; i < n_items; ++i) chunks += ((uint64_t)items[i].n + OPT_CHUNK - 1) / OPT_CHUNK;
  if (chunks > 0xffffffffull) return BTX_E_UNSUPPORTED;
  if (ws_bytes < (chunks ? chunks : 1) * sizeof(double)) return BTX_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  uint32_t total = 0;
  OptBatchDev b;
  for (int pos = 0; opt_next_batch(items, n_items, &pos, &b);) {
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(b.total_blocks), dim3(OPT_BLOCK), 0, st, b, part + total);
    total += b.total_blocks;
  }
  hipLaunchKernelGGL(optim_norm_final_kernel, dim3(1), dim3(OPT_BLOCK), 0, st, (const double*)part, total, max_norm, out_dev);
  return (int)hipGetLastError();
}

}  // extern "C"
