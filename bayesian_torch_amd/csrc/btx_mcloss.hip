// K12: loss heads on a stack of Monte-Carlo logits [S][B][C] (the reference's num_mc training loop,
// examples/main_bayesian_cifar.py:363-372, and the AvUC losses on mutual information, utils/avuc_loss.py type = 1).
//
//   MC cross-entropy   reduce 0 ("logits"): CE(mean_s z_s, y);  reduce 1 ("loss"): mean_s CE(z_s, y);  loss = ce + kl / B
//   AvUC on the stack  p_s = softmax(z_s), pbar = mean_s p_s, conf / pred from pbar, u = H(pbar) - mean_s H(p_s) (epsilon 1e-10
//                      inside every log), then the quadrant arithmetic of btx_calib.hip (single threshold or 21-threshold area)
//
// One workgroup of 256 threads owns a batch row for ALL S samples: one row launch each way, plus a one-workgroup fold in the
// forward (the sum over B).  Rows are streamed from L2 (an [S][C] slab of one batch row is a few KB); LDS holds the per-sample
// (max, 1 / sum) pairs, the reduction partials and, in the AvUC backward, the row of d H(pbar) / d pbar.
// Determinism: a thread owns the classes c0 .. c0 + V - 1 (V = 16 bytes of logits) for c0 = V * (tid + 256 i) on the vector path
// AND on the scalar path (rows off the 16-byte grid), so both paths add the same numbers in the same order; partials meet in a xor
// butterfly inside the wave and the four wave partials are added in index order (block_sum_inorder4 of btx_heads.h, which also holds
// Vw / load_v / store_v and the calibration workspace layout).  No atomics.  The sums over B are double.
#include "btx_heads.h"

#define MCL_THREADS 256
#define MCL_WAVES 4
#define MCL_EPS 1e-10f

namespace {

// V values of the row the cross-entropy sees: the mean over `sin` samples (stride `ss` elements) in sample order; sin = 1 with
// inv = 1 is the sample itself, bit for bit.  (Stays here: the units differ in how they pin contraction, see btx_heads.h.)
template <typename ACT>
__device__ __forceinline__ void mean_v(const ACT* __restrict__ row, size_t ss, int sin, float inv, int c0, int C, bool vec, float* v) {
  constexpr int V = Vw<ACT>::V;
  load_v<ACT>(row, c0, C, vec, v);
  for (int s = 1; s < sin; ++s) {
    float t[V];
    load_v<ACT>(row + (size_t)s * ss, c0, C, vec, t);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] += t[j];
  }
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] *= inv;
}

// ---- MC cross-entropy -----------------------------------------------------------------------------------------------
// ws (floats): [0, B) the rows' losses, then per (o, b), o < sout, the pair (max, sum of exp) the backward rebuilds the softmax from
template <typename ACT>
__global__ __launch_bounds__(MCL_THREADS) void mc_ce_row_kernel(const ACT* __restrict__ logits, const long long* __restrict__ labels,
                                                               int S, int B, int C, int reduce, float ls, bool vec,
                                                               float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int V = Vw<ACT>::V;
  __shared__ float red[MCL_WAVES];
  const int b = blockIdx.x;
  const size_t ss = (size_t)B * C;
  const int sout = reduce ? S : 1, sin = reduce ? 1 : S;
  const float inv = reduce ? 1.0f : 1.0f / (float)S;
  const long long y = labels[b];
  const bool y_ok = y >= 0 && y < (long long)C;  // (torch raises on such a label; here it contributes no target term and reads nothing)
  float acc = 0.f;
  for (int o = 0; o < sout; ++o) {
    const ACT* row = logits + (size_t)o * ss + (size_t)b * C;
    float mx = -INFINITY;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V];
      mean_v<ACT>(row, ss, sin, inv, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) mx = fmaxf(mx, v[j]);
    }
    mx = block_max_inorder4(mx, red);
    float se = 0.f, sz = 0.f;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V];
      mean_v<ACT>(row, ss, sin, inv, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) { se += expf(v[j] - mx); sz += v[j]; }
    }
    se = block_sum_inorder4(se, red);
    sz = block_sum_inorder4(sz, red);
    if (threadIdx.x == 0) {
      float zy = 0.f;
      if (y_ok) {
        for (int s = 0; s < sin; ++s) zy += (float)row[(size_t)s * ss + (size_t)y];
        zy *= inv;
      }
      const float lse = mx + logf(se);
      acc += (lse - (y_ok ? (1.0f - ls) * zy : 0.f)) - (ls / (float)C) * sz;
      float* st = ws + B + 2 * ((size_t)o * B + b);
      st[0] = mx;
      st[1] = se;
    }
  }
  if (threadIdx.x == 0) ws[b] = reduce ? acc / (float)S : acc;
}

__global__ __launch_bounds__(MCL_THREADS) void mc_ce_fold_kernel(const float* __restrict__ ws, int B, float inv_b,
                                                                const float* __restrict__ kl, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double part[MCL_WAVES];
  double a = 0.0;
  for (int i = threadIdx.x; i < B; i += MCL_THREADS) a += (double)ws[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = part[0];
    for (int w = 1; w < MCL_WAVES; ++w) t += part[w];
    t *= (double)inv_b;
    if (kl) t += (double)kl[0] * (double)inv_b;
    out[0] = (float)t;
  }
}

// d z_s[b][c] = g * (inv_b / S * (softmax(row)[c] - target[c])),  target = (1 - ls) onehot(y) + ls / C;  reduce 0: the same for every s.
// The upstream gradient g multiplies LAST: a loss scaled by a factor gives exactly that factor times these gradients, rounded once.
template <typename ACT>
__global__ __launch_bounds__(MCL_THREADS) void mc_ce_bwd_kernel(const ACT* __restrict__ logits, const long long* __restrict__ labels,
                                                               int S, int B, int C, int reduce, float ls, float inv_b, bool vec,
                                                               const float* __restrict__ g_loss, const float* __restrict__ ws,
                                                               ACT* __restrict__ dlogits) {
#pragma clang fp contract(off)
  constexpr int V = Vw<ACT>::V;
  const int b = blockIdx.x;
  const size_t ss = (size_t)B * C;
  const int sout = reduce ? S : 1, sin = reduce ? 1 : S;
  const float inv = reduce ? 1.0f : 1.0f / (float)S;
  const long long y = labels[b];
  const float g = g_loss[0], ks = inv_b / (float)S;
  const float tl = ls / (float)C;
  for (int o = 0; o < sout; ++o) {
    const ACT* row = logits + (size_t)o * ss + (size_t)b * C;
    ACT* drow = dlogits + (size_t)o * ss + (size_t)b * C;
    const float* st = ws + B + 2 * ((size_t)o * B + b);
    const float mx = st[0], rse = 1.0f / st[1];
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V], d[V];
      mean_v<ACT>(row, ss, sin, inv, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float p = expf(v[j] - mx) * rse;
        d[j] = g * (ks * ((p - tl) - ((long long)(c0 + j) == y ? 1.0f - ls : 0.f)));
      }
      for (int s = 0; s < sin; ++s) store_v<ACT>(drow + (size_t)s * ss, c0, C, vec, d);
    }
  }
}

// ---- AvUC on the stack ----------------------------------------------------------------------------------------------
// ws (floats): the header and the per-row records of btx_calib.hip, then per (s, b) the pair (max, 1 / sum of exp)
template <typename ACT>
__global__ __launch_bounds__(MCL_THREADS) void avu_mc_row_kernel(const ACT* __restrict__ logits, const long long* __restrict__ labels,
                                                                int S, int B, int C, bool vec, float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int V = Vw<ACT>::V;
  __shared__ float red[MCL_WAVES];
  __shared__ int redi[MCL_WAVES];
  __shared__ float m_s[BTX_MCLOSS_MAX_S], i_s[BTX_MCLOSS_MAX_S];
  const int b = blockIdx.x;
  const size_t ss = (size_t)B * C;
  const ACT* row0 = logits + (size_t)b * C;
  float* pairs = ws + CALIB_HDR_FLOATS + (size_t)B * CALIB_ROW_FLOATS;
  for (int s = 0; s < S; ++s) {
    const ACT* row = row0 + (size_t)s * ss;
    float mx = -INFINITY;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V];
      load_v<ACT>(row, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) mx = fmaxf(mx, v[j]);
    }
    mx = block_max_inorder4(mx, red);
    float se = 0.f;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V];
      load_v<ACT>(row, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) se += expf(v[j] - mx);
    }
    se = block_sum_inorder4(se, red);
    if (threadIdx.x == 0) {
      m_s[s] = mx;
      i_s[s] = 1.0f / se;
      pairs[2 * ((size_t)s * B + b)] = mx;
      pairs[2 * ((size_t)s * B + b) + 1] = 1.0f / se;
    }
  }
  __syncthreads();
  const float invS = 1.0f / (float)S;
  float eh = 0.f, hb = 0.f, best = -INFINITY;  // sum_s H(p_s), H(pbar), max of pbar with its lowest index
  int am = 0x7fffffff;
  for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
    float pb[V];
#pragma unroll
    for (int j = 0; j < V; ++j) pb[j] = 0.f;
    for (int s = 0; s < S; ++s) {
      float v[V];
      load_v<ACT>(row0 + (size_t)s * ss, c0, C, vec, v);
      const float mx = m_s[s], is = i_s[s];
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) {
          const float p = expf(v[j] - mx) * is;
          pb[j] += p;
          eh -= p * logf(p + MCL_EPS);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (c0 + j < C) {
        const float p = pb[j] * invS;
        hb -= p * logf(p + MCL_EPS);
        if (p > best) { best = p; am = c0 + j; }  // ascending classes: a tie keeps the lowest index
      }
  }
  eh = block_sum_inorder4(eh, red);
  hb = block_sum_inorder4(hb, red);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(am, off, 64);
    if (ob > best || (ob == best && oa < am)) { best = ob; am = oa; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = best; redi[threadIdx.x >> 6] = am; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < MCL_WAVES; ++w)
      if (red[w] > best || (red[w] == best && redi[w] < am)) { best = red[w]; am = redi[w]; }
    if (am >= C) am = 0;  // a row of NaN compares false everywhere: keep the index inside the row
    const float u = hb - eh * invS;
    float* r = ws + CALIB_HDR_FLOATS + (size_t)b * CALIB_ROW_FLOATS;
    r[0] = best;
    r[1] = u;
    r[2] = tanhf(u);
    r[3] = __int_as_float((am << 1) | (labels[b] == (long long)am ? 1 : 0));
  }
}

// d / d z_s[j] = gs / S * ( dc * p_s[m] * (delta_jm - p_s[j]) + du * p_s[j] * (q_s[j] - sum_c p_s[c] q_s[c]) ),
// q_s = gb - g_s,  gb = dH/dp at pbar,  g_s = dH/dp at p_s,  dH/dp = -(log(p + eps) + p / (p + eps)),  m = arg-max of pbar.
// gs = g_loss * dloss/dr + g_r.  The upstream gradients multiply LAST (d = g_loss * (dloss/dr * unit) + g_r * unit): a loss scaled by a
// factor gives exactly that factor times these gradients, rounded once.
template <typename ACT>
__global__ __launch_bounds__(MCL_THREADS) void avu_mc_bwd_kernel(const ACT* __restrict__ logits, int S, int B, int C, bool vec,
                                                                const float* __restrict__ g_loss, const float* __restrict__ g_r,
                                                                const float* __restrict__ ws, ACT* __restrict__ dlogits) {
#pragma clang fp contract(off)
  constexpr int V = Vw<ACT>::V;
  extern __shared__ __attribute__((aligned(16))) float gb[];  // [C rounded up to V]
  __shared__ float red[MCL_WAVES];
  __shared__ float m_s[BTX_MCLOSS_MAX_S], i_s[BTX_MCLOSS_MAX_S];
  const int b = blockIdx.x;
  const size_t ss = (size_t)B * C;
  const float* r = ws + CALIB_HDR_FLOATS + (size_t)b * CALIB_ROW_FLOATS;
  const float* pairs = ws + CALIB_HDR_FLOATS + (size_t)B * CALIB_ROW_FLOATS;
  const float cf = r[0], t = r[2];
  const double u = (double)r[1];
  const int code = __float_as_int(r[3]);
  const bool good = code & 1;
  const int am = min(max(code >> 1, 0), C - 1);
  const int K = min(max(__float_as_int(ws[HDR_K]), 0), CALIB_K_AREA);
  const double* th = (const double*)(ws + HDR_TH);
  const float* G = ws + HDR_G;
  float sa = 0.f, su = 0.f;
  for (int k = 0; k < K; ++k) {
    if (u <= th[k]) sa += G[4 * k + (good ? 0 : 2)];
    else su += G[4 * k + (good ? 1 : 3)];
  }
  const float gl = g_loss ? g_loss[0] : 0.f, gr = g_r ? g_r[0] : 0.f, dldr = ws[HDR_DLDR];
  const float invS = 1.0f / (float)S;
  const float w = good ? cf : 1.0f - cf;
  const float dc = (good ? 1.0f : -1.0f) * (sa * (1.0f - t) + su * t) * invS;  // d r / d conf and d r / d u of this row, over S
  const float du = w * (su - sa) * (1.0f - t * t) * invS;
  if (threadIdx.x < S) {
    m_s[threadIdx.x] = pairs[2 * ((size_t)threadIdx.x * B + b)];
    i_s[threadIdx.x] = pairs[2 * ((size_t)threadIdx.x * B + b) + 1];
  }
  __syncthreads();
  const ACT* row0 = logits + (size_t)b * C;
  ACT* drow0 = dlogits + (size_t)b * C;
  for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
    float pb[V];
#pragma unroll
    for (int j = 0; j < V; ++j) pb[j] = 0.f;
    for (int s = 0; s < S; ++s) {
      float v[V];
      load_v<ACT>(row0 + (size_t)s * ss, c0, C, vec, v);
      const float mx = m_s[s], is = i_s[s];
#pragma unroll
      for (int j = 0; j < V; ++j) pb[j] += expf(v[j] - mx) * is;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float p = pb[j] * invS;
      gb[c0 + j] = -(logf(p + MCL_EPS) + p / (p + MCL_EPS));  // (a thread reads back only what it wrote)
    }
  }
  for (int s = 0; s < S; ++s) {
    const ACT* row = row0 + (size_t)s * ss;
    const float mx = m_s[s], is = i_s[s];
    float a = 0.f;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V];
      load_v<ACT>(row, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (c0 + j < C) {
          const float p = expf(v[j] - mx) * is;
          a += p * (gb[c0 + j] + (logf(p + MCL_EPS) + p / (p + MCL_EPS)));
        }
    }
    a = block_sum_inorder4(a, red);
    const float pm = expf((float)row[am] - mx) * is;
    for (int c0 = threadIdx.x * V; c0 < C; c0 += MCL_THREADS * V) {
      float v[V], d[V];
      load_v<ACT>(row, c0, C, vec, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float p = expf(v[j] - mx) * is;
        const float q = gb[c0 + j] + (logf(p + MCL_EPS) + p / (p + MCL_EPS));
        const float unit = dc * pm * ((c0 + j == am ? 1.0f : 0.0f) - p) + du * p * (q - a);  // d r / d z_s[j]
        float v = g_loss ? gl * (dldr * unit) : 0.f;
        if (g_r) v += gr * unit;
        d[j] = v;
      }
      store_v<ACT>(drow0 + (size_t)s * ss, c0, C, vec, d);
    }
  }
}

inline size_t ce_floats(int S, int B) { return (size_t)B + 2 * (size_t)S * B; }
inline size_t avu_floats(int S, int B) { return (size_t)CALIB_HDR_FLOATS + (size_t)B * CALIB_ROW_FLOATS + 2 * (size_t)S * B; }

inline int check_shape(int S, int B, int C) {
  if (S < 1 || S > BTX_MCLOSS_MAX_S || B < 1 || C < 1) return BTX_E_SHAPE;
  if (C > BTX_MCLOSS_MAX_CLASSES) return BTX_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

size_t btx_mcloss_workspace_bytes(int S, int B) {
  if (S < 0) S = 0;
  if (B < 0) B = 0;
  const size_t a = ce_floats(S, B), c = avu_floats(S, B);
  return 4 * (a > c ? a : c);
}

int btx_mc_ce_fwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int reduce, float label_smoothing,
                  const float* kl, float inv_b, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !labels || !out || !ws) return BTX_E_NULL;
  if (const int rc = check_shape(S, B, C)) return rc;
  if ((reduce != 0 && reduce != 1) || !(label_smoothing >= 0.f && label_smoothing < 1.f)) return BTX_E_SHAPE;
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if (ws_bytes < 4 * ce_floats(S, B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 3) return BTX_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(mc_ce_row_kernel<T>, dim3(B), dim3(MCL_THREADS), 0, st, (const T*)logits, (const long long*)labels, S, B, C,
                       reduce, label_smoothing, on_grid(logits, C, esize), (float*)ws);
    hipLaunchKernelGGL(mc_ce_fold_kernel, dim3(1), dim3(MCL_THREADS), 0, st, (const float*)ws, B, inv_b, kl, out);
  });
}

int btx_mc_ce_bwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int reduce, float label_smoothing,
                  float inv_b, const float* g_loss, const void* ws, size_t ws_bytes, void* dlogits, void* stream) {
  if (!logits || !labels || !g_loss || !ws || !dlogits) return BTX_E_NULL;
  if (const int rc = check_shape(S, B, C)) return rc;
  if ((reduce != 0 && reduce != 1) || !(label_smoothing >= 0.f && label_smoothing < 1.f)) return BTX_E_SHAPE;
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if (ws_bytes < 4 * ce_floats(S, B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 3) return BTX_E_ALIGN;
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(mc_ce_bwd_kernel<T>, dim3(B), dim3(MCL_THREADS), 0, (hipStream_t)stream, (const T*)logits,
                       (const long long*)labels, S, B, C, reduce, label_smoothing, inv_b,
                       on_grid(logits, C, esize) && on_grid(dlogits, C, esize), g_loss, (const float*)ws, (T*)dlogits);
  });
}

int btx_avu_mc_fwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int area, float th,
                   const float* th_dev, float beta, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !labels || !out || !ws) return BTX_E_NULL;
  if (const int rc = check_shape(S, B, C)) return rc;
  if (C > BTX_AVU_MC_MAX_CLASSES) return BTX_E_UNSUPPORTED;
  if (area != 0 && area != 1) return BTX_E_SHAPE;
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if (ws_bytes < 4 * avu_floats(S, B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;  // the header holds the thresholds as doubles
  hipStream_t st = (hipStream_t)stream;
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(avu_mc_row_kernel<T>, dim3(B), dim3(MCL_THREADS), 0, st, (const T*)logits, (const long long*)labels, S, B, C,
                       on_grid(logits, C, esize), (float*)ws);
    // the fold of btx_calib.hip on the records above.  Next to what the backward reads (HDR_DLDR, HDR_K, HDR_G, HDR_TH) it stores
    // HDR_LOSS, HDR_R and HDR_THA: inside the header avu_floats() reserves, read by no kernel of this unit.
    btx::launch_avu_fold(B, area, th, th_dev, beta, out, (float*)ws, st);
  });
}

int btx_avu_mc_bwd(const void* logits, int S, int B, int C, int act_dtype, const float* g_loss, const float* g_r, const void* ws,
                   size_t ws_bytes, void* dlogits, void* stream) {
  if (!logits || !ws || !dlogits || (!g_loss && !g_r)) return BTX_E_NULL;
  if (const int rc = check_shape(S, B, C)) return rc;
  if (C > BTX_AVU_MC_MAX_CLASSES) return BTX_E_UNSUPPORTED;  // the backward's LDS row stays below 64 KiB: no per-function opt-in
  const int esize = act_esize(act_dtype);
  if (!esize) return BTX_E_DTYPE;
  if (ws_bytes < 4 * avu_floats(S, B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;
  const size_t lds = (((size_t)C + 7) & ~(size_t)7) * 4;  // the row of dH/dp at pbar: inside the 64 KiB every kernel may use
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(avu_mc_bwd_kernel<T>, dim3(B), dim3(MCL_THREADS), lds, (hipStream_t)stream, (const T*)logits, S, B, C,
                       on_grid(logits, C, esize) && on_grid(dlogits, C, esize), g_loss, g_r, (const float*)ws, (T*)dlogits);
  });
}

}  // extern "C"

