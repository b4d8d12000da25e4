// K16: regression heads (BTX-REG v1): what a model that predicts real values needs at its two ends.
//
//   btx_mc_moments_lanes     MC moment statistics of `lanes` samples: float64 sums of m, m^2 and exp(s) per element
//   btx_mc_gnll_fwd / _bwd   the Gaussian negative log-likelihood of a stack of MC outputs [S][B][W] against real targets [B][D]
//   btx_reg_eval_update      a batch of packed moments and its targets folded into a float64 evaluation state
//
// Output layout: W = 2 D with has_var (columns [0, D) the mean m, [D, 2 D) the log-variance s, Kendall & Gal), W = D without.
// Per-element arithmetic is f32 in the loss head and f64 in the evaluator, every operation rounded once: the unit is built with
// -ffp-contract=off.  Sums: element terms widen to double; one workgroup of 256 threads owns a chunk of REG_CHUNK elements, thread
// t adds e = t, t + 256, ... in order from zero, a xor butterfly inside the wave, (w0 + w1) + (w2 + w3) (block_sum_pairwise4 of
// btx_heads.h); a one-workgroup fold adds the chunks' partials (lane l: l, l + 64, ...) with the same butterfly.  Shapes fixed by
// the element count alone: no atomics, no "last block" counters, no host read.  Plain vector stores only.
#include "btx_heads.h"

#define REG_THREADS 256
#define REG_CHUNK 4096
#define REG_FOLD_THREADS 1024
#define REG_FOLD_WAVES 16
#define REG_EVAL_SUMS 9                                /* valid, ignored and the seven sums of the state */
#define REG_EVAL_Q (REG_EVAL_SUMS + BTX_REG_EVAL_MAX_LEVELS)
#define REG_TWO_PI 6.283185307179586

namespace {

// ---- MC moment statistics ---------------------------------------------------------------------------------------------
// A thread owns the elements e0 .. e0 + V - 1 (V = 16 bytes of outputs) and folds the lanes in order, so `lanes` samples in one
// call equal `lanes` single calls bit for bit; the vector path (vec: out and packed on the 16-byte grid, D % V == 0, so the V
// elements share a row) and the element-wise path compute every element alike.  packed: [N sum m | N sum m^2 | N sum v | kl | n].
template <typename ACT>
__global__ __launch_bounds__(REG_THREADS) void moments_kernel(const ACT* __restrict__ out, int lanes, int bs, int D, int W,
                                                             int has_var, double kl, bool vec, double* __restrict__ packed) {
#pragma clang fp contract(off)
  constexpr int V = Vw<ACT>::V;
  const long long N = (long long)bs * D;
  const long long e0 = ((long long)blockIdx.x * REG_THREADS + threadIdx.x) * V;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double a = packed[3 * N], n = packed[3 * N + 1];
    for (int k = 0; k < lanes; ++k) { a += kl; n += 1.0; }
    packed[3 * N] = a;
    packed[3 * N + 1] = n;
  }
  if (e0 >= N) return;
  double sm[V], sq[V], sv[V];
  if (vec) {
    const int b = (int)(e0 / D), d = (int)(e0 - (long long)b * D);
#pragma unroll
    for (int j = 0; j < V; j += 2) {
      const double2 q0 = *reinterpret_cast<const double2*>(packed + e0 + j);
      const double2 q1 = *reinterpret_cast<const double2*>(packed + N + e0 + j);
      const double2 q2 = *reinterpret_cast<const double2*>(packed + 2 * N + e0 + j);
      sm[j] = q0.x; sm[j + 1] = q0.y; sq[j] = q1.x; sq[j + 1] = q1.y; sv[j] = q2.x; sv[j + 1] = q2.y;
    }
    for (int k = 0; k < lanes; ++k) {
      const ACT* row = out + ((size_t)k * bs + b) * (size_t)W + d;
      float m[V];
      load_v<ACT>(row, 0, V, true, m);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double md = (double)m[j];
        sm[j] += md;
        sq[j] += md * md;
      }
      if (has_var) {
        float s[V];
        load_v<ACT>(row + D, 0, V, true, s);
#pragma unroll
        for (int j = 0; j < V; ++j) sv[j] += (double)expf(s[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < V; j += 2) {
      *reinterpret_cast<double2*>(packed + e0 + j) = make_double2(sm[j], sm[j + 1]);
      *reinterpret_cast<double2*>(packed + N + e0 + j) = make_double2(sq[j], sq[j + 1]);
      if (has_var) *reinterpret_cast<double2*>(packed + 2 * N + e0 + j) = make_double2(sv[j], sv[j + 1]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const long long e = e0 + j;
      if (e >= N) break;
      const int b = (int)(e / D), d = (int)(e - (long long)b * D);
      double am = packed[e], aq = packed[N + e], av = packed[2 * N + e];
      for (int k = 0; k < lanes; ++k) {
        const ACT* row = out + ((size_t)k * bs + b) * (size_t)W + d;
        const double md = (double)(float)row[0];
        am += md;
        aq += md * md;
        if (has_var) av += (double)expf((float)row[D]);
      }
      packed[e] = am;
      packed[N + e] = aq;
      if (has_var) packed[2 * N + e] = av;
    }
  }
}

// ---- Gaussian NLL head ------------------------------------------------------------------------------------------------
// the f32 terms of element (b, d): reduce 1 ("loss") sum_s l_s in double, l_s = 0.5 (s + (y - m)^2 exp(-s)); reduce 0 ("moments")
// l = 0.5 (log vbar + (y - mbar)^2 / vbar) of the moment-matched predictive.  Without has_var every sample has s = s0.
template <typename ACT>
__device__ __forceinline__ void moments_of(const ACT* __restrict__ col, size_t ss, int S, int D, int has_var, float s0, float* mbar,
                                           float* vbar) {
#pragma clang fp contract(off)
  float sm = 0.f, sv = 0.f;
  for (int s = 0; s < S; ++s) {
    sm += (float)col[(size_t)s * ss];
    sv += expf(has_var ? (float)col[(size_t)s * ss + D] : s0);
  }
  const float mb = sm / (float)S;
  float se = 0.f;
  for (int s = 0; s < S; ++s) {
    const float c = (float)col[(size_t)s * ss] - mb;
    se += c * c;
  }
  *mbar = mb;
  *vbar = sv / (float)S + se / (float)S;
}

template <typename ACT>
__global__ __launch_bounds__(REG_THREADS) void gnll_chunk_kernel(const ACT* __restrict__ stack, const float* __restrict__ target,
                                                                int S, int B, int D, int W, int has_var, float s0, int reduce,
                                                                double* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ double part[4];
  const long long N = (long long)B * D;
  const size_t ss = (size_t)B * W;
  double acc = 0.0;
  for (long long e = (long long)blockIdx.x * REG_CHUNK + threadIdx.x; e < N && e < ((long long)blockIdx.x + 1) * REG_CHUNK;
       e += REG_THREADS) {
    const int b = (int)(e / D), d = (int)(e - (long long)b * D);
    const ACT* col = stack + (size_t)b * W + d;
    const float y = target[e];
    double term;
    if (reduce) {
      term = 0.0;
      for (int s = 0; s < S; ++s) {
        const float m = (float)col[(size_t)s * ss];
        const float lv = has_var ? (float)col[(size_t)s * ss + D] : s0;
        const float r = y - m;
        term += (double)(0.5f * (lv + (r * r) * expf(-lv)));
      }
    } else {
      float mb, vb;
      moments_of<ACT>(col, ss, S, D, has_var, s0, &mb, &vb);
      const float r = y - mb;
      term = (double)(0.5f * (logf(vb) + (r * r) / vb));
    }
    acc += term;
  }
  const double t = block_sum_pairwise4(acc, part);
  if (threadIdx.x == 0) ws[blockIdx.x] = t;
}

// out[0] = (float)(sum / div + add + kl / B): the division, the constant of `full` and the KL term in double, rounded to f32 once
__global__ __launch_bounds__(64) void gnll_fold_kernel(const double* __restrict__ ws, int nchunks, double div, double add, double B,
                                                      const float* __restrict__ kl, float* __restrict__ out) {
#pragma clang fp contract(off)
  double a = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += 64) a += ws[i];
  a = wave_sum(a);
  if (threadIdx.x == 0) {
    double t = a / div + add;
    if (kl) t += (double)kl[0] / B;
    out[0] = (float)t;
  }
}

// reduce 1: d m_s = g ((-(r exp(-s))) k), d s_s = g ((0.5 (1 - r^2 exp(-s))) k), k = 1 / (S B)
// reduce 0: a = 1 / vbar - r^2 / vbar^2;  d m_s = g ((-(r / vbar) + (m_s - mbar) a) k),  d s_s = g ((0.5 exp(s_s) a) k)
// The upstream gradient g multiplies LAST: a loss scaled by a factor gives exactly that factor times these gradients, rounded once.
template <typename ACT>
__global__ __launch_bounds__(REG_THREADS) void gnll_bwd_kernel(const ACT* __restrict__ stack, const float* __restrict__ target, int S,
                                                              int B, int D, int W, int has_var, float s0, int reduce,
                                                              const float* __restrict__ g_loss, ACT* __restrict__ dstack) {
#pragma clang fp contract(off)
  const long long N = (long long)B * D;
  const long long e = (long long)blockIdx.x * REG_THREADS + threadIdx.x;
  if (e >= N) return;
  const size_t ss = (size_t)B * W;
  const int b = (int)(e / D), d = (int)(e - (long long)b * D);
  const ACT* col = stack + (size_t)b * W + d;
  ACT* dcol = dstack + (size_t)b * W + d;
  const float y = target[e], g = g_loss[0];
  const float k = 1.0f / ((float)S * (float)B);
  if (reduce) {
    for (int s = 0; s < S; ++s) {
      const float m = (float)col[(size_t)s * ss];
      const float lv = has_var ? (float)col[(size_t)s * ss + D] : s0;
      const float r = y - m, iv = expf(-lv);
      dcol[(size_t)s * ss] = (ACT)(g * ((-(r * iv)) * k));
      if (has_var) dcol[(size_t)s * ss + D] = (ACT)(g * ((0.5f * (1.0f - (r * r) * iv)) * k));
    }
  } else {
    float mb, vb;
    moments_of<ACT>(col, ss, S, D, has_var, s0, &mb, &vb);
    const float r = y - mb;
    const float a = 1.0f / vb - (r * r) / (vb * vb);
    const float c0 = -(r / vb);
    for (int s = 0; s < S; ++s) {
      const float m = (float)col[(size_t)s * ss];
      dcol[(size_t)s * ss] = (ACT)(g * ((c0 + (m - mb) * a) * k));
      if (has_var) dcol[(size_t)s * ss + D] = (ACT)(g * (((0.5f * expf((float)col[(size_t)s * ss + D])) * a) * k));
    }
  }
}

// ---- evaluation ---------------------------------------------------------------------------------------------------------
// ws: per chunk REG_EVAL_Q doubles: valid, ignored, sum err^2, |err|, nll, ep, al, y, y^2, then the coverage counts
__global__ __launch_bounds__(REG_THREADS) void reg_eval_chunk_kernel(const double* __restrict__ packed, const float* __restrict__ target,
                                                                    long long N, double noise_var, double min_var,
                                                                    const double* __restrict__ z2, int K,
                                                                    const double* __restrict__ state, float* __restrict__ records,
                                                                    long long capacity, double* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ double part[4];
  const double n = packed[3 * N + 1];
  double zk[BTX_REG_EVAL_MAX_LEVELS];
#pragma unroll
  for (int k = 0; k < BTX_REG_EVAL_MAX_LEVELS; ++k) zk[k] = (k < K) ? z2[k] : 0.0;
  double a[REG_EVAL_Q];
#pragma unroll
  for (int j = 0; j < REG_EVAL_Q; ++j) a[j] = 0.0;
  const long long cursor = records ? (long long)state[BTX_REG_EVAL_CURSOR] : 0;
  for (long long e = (long long)blockIdx.x * REG_CHUNK + threadIdx.x; e < N && e < ((long long)blockIdx.x + 1) * REG_CHUNK;
       e += REG_THREADS) {
    const float yf = target[e];
    const bool ok = !(yf != yf);  // a NaN target marks an ignored element
    const double y = (double)yf;
    const double mean = packed[e] / n;
    const double ep = fmax(packed[N + e] / n - mean * mean, 0.0);
    const double al = packed[2 * N + e] / n + noise_var;
    const double var = fmax(ep + al, min_var);
    const double err = y - mean;
    const double e2 = err * err;
    const double nll = 0.5 * ((double)logf((float)(REG_TWO_PI * var)) + e2 / var);
    a[0] += ok ? 1.0 : 0.0;
    a[1] += ok ? 0.0 : 1.0;
    a[2] += ok ? e2 : 0.0;
    a[3] += ok ? fabs(err) : 0.0;
    a[4] += ok ? nll : 0.0;
    a[5] += ok ? ep : 0.0;
    a[6] += ok ? al : 0.0;
    a[7] += ok ? y : 0.0;
    a[8] += ok ? y * y : 0.0;
#pragma unroll
    for (int k = 0; k < BTX_REG_EVAL_MAX_LEVELS; ++k) a[REG_EVAL_SUMS + k] += (ok && k < K && e2 <= zk[k] * var) ? 1.0 : 0.0;
    if (records) {
      const long long at = cursor + e;
      if (at >= 0 && at < capacity) {
        float* q = records + (size_t)at * 4;
        q[0] = (float)mean;
        q[1] = (float)ep;
        q[2] = (float)al;
        q[3] = (float)err;  // NaN on an ignored element
      }
    }
  }
#pragma unroll
  for (int j = 0; j < REG_EVAL_Q; ++j) {
    const double t = block_sum_pairwise4(a[j], part);
    if (threadIdx.x == 0) ws[(size_t)blockIdx.x * REG_EVAL_Q + j] = t;
  }
}

// a wave takes the quantities wave, wave + 16, ...: no two waves touch the same state word
__global__ __launch_bounds__(REG_FOLD_THREADS) void reg_eval_fold_kernel(const double* __restrict__ ws, int nchunks, long long N, int K,
                                                                        double* __restrict__ state, long long capacity) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, li = threadIdx.x & 63;
  for (int q = wave; q < REG_EVAL_SUMS + K; q += REG_FOLD_WAVES) {  // wave-uniform
    double a = 0.0;
    for (int i = li; i < nchunks; i += 64) a += ws[(size_t)i * REG_EVAL_Q + q];
    a = wave_sum(a);
    if (li == 0) state[q < REG_EVAL_SUMS ? q : BTX_REG_EVAL_HEADER + (q - REG_EVAL_SUMS)] += a;
  }
  if (threadIdx.x == REG_FOLD_THREADS - 1) {  // the cursor words are touched by this thread alone
    const double cur = state[BTX_REG_EVAL_CURSOR];
    const double over = cur + (double)N - (double)capacity;
    state[BTX_REG_EVAL_DROPPED] += fmin(fmax(over, 0.0), (double)N);
    state[BTX_REG_EVAL_CURSOR] = cur + (double)N;
  }
}

inline int check_reg_shape(long long rows, int D, int has_var) {
  if (rows < 1 || D < 1 || (has_var != 0 && has_var != 1)) return BTX_E_SHAPE;
  if (rows * (long long)D > 2147483647LL - 2) return BTX_E_UNSUPPORTED;
  return 0;
}

inline size_t chunks_of(long long N) { return (size_t)((N + REG_CHUNK - 1) / REG_CHUNK); }

}  // namespace

extern "C" {

int btx_mc_moments_lanes(const void* out, int lanes, int bs, int D, int has_var, int act_dtype, double kl, double* packed,
                         void* stream) {
  if (!out || !packed) return BTX_E_NULL;
  if (lanes < 1 || bs < 1) return BTX_E_SHAPE;
  if (const int rc = check_reg_shape(bs, D, has_var)) return rc;
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if ((((uintptr_t)out) & (uintptr_t)(esize - 1)) || (((uintptr_t)packed) & 7)) return BTX_E_ALIGN;  // below the element types' own
  const int W = has_var ? 2 * D : D, V = 16 / esize;
  const long long N = (long long)bs * D;
  const bool vec = on_grid(out, D, esize) && aligned16(packed);  // then N % V == 0 and every block of packed is on the grid
  const unsigned grid = (unsigned)((N + (long long)REG_THREADS * V - 1) / ((long long)REG_THREADS * V));
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(moments_kernel<T>, dim3(grid), dim3(REG_THREADS), 0, (hipStream_t)stream, (const T*)out, lanes, bs, D, W,
                       has_var, kl, vec, packed);
  });
}

size_t btx_mc_gnll_workspace_bytes(int B, int D) {
  if (B < 1 || D < 1) return 0;
  return chunks_of((long long)B * D) * sizeof(double);
}

static int gnll_check(const void* stack, const float* target, int S, int B, int D, int has_var, int act_dtype, int reduce,
                      float noise_var) {
  if (!stack || !target) return BTX_E_NULL;
  if (S < 1 || S > BTX_MCLOSS_MAX_S || (reduce != 0 && reduce != 1)) return BTX_E_SHAPE;
  if (const int rc = check_reg_shape(B, D, has_var)) return rc;
  if (!has_var && !(noise_var > 0.f)) return BTX_E_SHAPE;
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if ((((uintptr_t)stack) & (uintptr_t)(esize - 1)) || (((uintptr_t)target) & 3)) return BTX_E_ALIGN;
  return 0;
}

int btx_mc_gnll_fwd(const void* stack, const float* target, int S, int B, int D, int has_var, int act_dtype, int reduce, float noise_var,
                    int full, const float* kl, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!out || !ws) return BTX_E_NULL;
  if (const int rc = gnll_check(stack, target, S, B, D, has_var, act_dtype, reduce, noise_var)) return rc;
  if (full != 0 && full != 1) return BTX_E_SHAPE;
  if (ws_bytes < btx_mc_gnll_workspace_bytes(B, D)) return BTX_E_WORKSPACE;
  if ((((uintptr_t)ws) & 7) || (((uintptr_t)out) & 3) || (((uintptr_t)kl) & 3)) return BTX_E_ALIGN;
  const long long N = (long long)B * D;
  const int nchunks = (int)chunks_of(N), W = has_var ? 2 * D : D;
  const float s0 = has_var ? 0.f : logf(noise_var);
  const double div = reduce ? (double)S * (double)B : (double)B;
  const double add = full ? 0.5 * 1.8378770664093453 * (double)D : 0.0;  // 0.5 log(2 pi) D
  hipStream_t st = (hipStream_t)stream;
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(gnll_chunk_kernel<T>, dim3(nchunks), dim3(REG_THREADS), 0, st, (const T*)stack, target, S, B, D, W, has_var, s0,
                       reduce, (double*)ws);
    hipLaunchKernelGGL(gnll_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, nchunks, div, add, (double)B, kl, out);
  });
}

int btx_mc_gnll_bwd(const void* stack, const float* target, int S, int B, int D, int has_var, int act_dtype, int reduce, float noise_var,
                    const float* g_loss, void* dstack, void* stream) {
  if (!g_loss || !dstack) return BTX_E_NULL;
  if (const int rc = gnll_check(stack, target, S, B, D, has_var, act_dtype, reduce, noise_var)) return rc;
  if ((((uintptr_t)dstack) & (uintptr_t)(act_esize(act_dtype) - 1)) || (((uintptr_t)g_loss) & 3)) return BTX_E_ALIGN;
  const long long N = (long long)B * D;
  const int W = has_var ? 2 * D : D;
  const float s0 = has_var ? 0.f : logf(noise_var);
  const unsigned grid = (unsigned)((N + REG_THREADS - 1) / REG_THREADS);
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(gnll_bwd_kernel<T>, dim3(grid), dim3(REG_THREADS), 0, (hipStream_t)stream, (const T*)stack, target, S, B, D, W,
                       has_var, s0, reduce, g_loss, (T*)dstack);
  });
}

size_t btx_reg_eval_workspace_bytes(int bs, int D) {
  if (bs < 1 || D < 1) return 0;
  return chunks_of((long long)bs * D) * REG_EVAL_Q * sizeof(double);
}

int btx_reg_eval_update(const double* packed, const float* target, int bs, int D, double noise_var, double min_var, const double* z2,
                        int K, double* state, size_t state_doubles, float* records, int64_t capacity, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!packed || !target || !state || !ws || (K > 0 && !z2) || (capacity > 0 && !records)) return BTX_E_NULL;
  if (K < 0 || K > BTX_REG_EVAL_MAX_LEVELS || capacity < 0 || !(noise_var >= 0.0) || !(min_var > 0.0)) return BTX_E_SHAPE;
  if (const int rc = check_reg_shape(bs, D, 0)) return rc;
  if (ws_bytes < btx_reg_eval_workspace_bytes(bs, D) || state_doubles < (size_t)BTX_REG_EVAL_HEADER + (size_t)K) return BTX_E_WORKSPACE;
  if ((((uintptr_t)packed) & 7) || (((uintptr_t)state) & 7) || (((uintptr_t)ws) & 7) || (((uintptr_t)z2) & 7) ||
      (((uintptr_t)target) & 3) || (((uintptr_t)records) & 3))
    return BTX_E_ALIGN;  // the natural alignment of the element types: no valid tensor ends here
  const long long N = (long long)bs * D;
  const int nchunks = (int)chunks_of(N);
  if (capacity == 0) records = nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(reg_eval_chunk_kernel, dim3(nchunks), dim3(REG_THREADS), 0, st, packed, target, N, noise_var, min_var, z2, K,
                     (const double*)state, records, (long long)capacity, (double*)ws);
  hipLaunchKernelGGL(reg_eval_fold_kernel, dim3(1), dim3(REG_FOLD_THREADS), 0, st, (const double*)ws, nchunks, N, K, state,
                     (long long)capacity);
  return (int)hipGetLastError();
}

}  // extern "C"
