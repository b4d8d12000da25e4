// K9: uncertainty-calibration losses (AvU / AUAvU / EaU / EaC), forward and backward, three launches per loss and none of
// them synchronises.  Reference (host loops with .item() per example): utils/avuc_loss.py:127-176, 310-366 and
// utils/uncertainty_calibration_loss.py:61-108, 142-189, 210-261.
//
//   loss = -beta * log(r + 1e-10),  r = (n_1 + n_4) / (n_1 + n_2 + n_3 + n_4 + 1e-10)      (area form: r = trapezoid of r_k)
//   n_q  = sum over the examples of quadrant q (good / bad x certain / uncertain) of a product of two soft weights
//
// Launches: (1) avu_row_kernel, one wave per batch row: softmax statistics of the row; (2) calib_fold_kernel, ONE workgroup:
// thresholds, quadrant sums, the loss and the table d r / d n_q; (3) a backward kernel that walks that table per row.
// Determinism: every sum has a shape fixed by (B, C) alone — a lane's strided partial, a xor butterfly inside the wave (both
// partners add the same two numbers, so all lanes hold the same bits), and partials of the fold added in index order by one
// thread.  No atomics.  The quadrant sums and everything after them are double.
// The workspace layout (CALIB_*, HDR_*) and wave_sum live in btx_heads.h; the fold's AvU mode also serves btx_mcloss.hip, through
// btx::launch_avu_fold.
#include "btx_heads.h"

#define CALIB_EPS 1e-10f

namespace {

// ---- (1) per-row softmax statistics ---------------------------------------------------------------------------------
template <typename ACT>
__global__ __launch_bounds__(256) void avu_row_kernel(const ACT* __restrict__ logits, const long long* __restrict__ labels,
                                                      int B, int C, float* __restrict__ rows) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), li = threadIdx.x & 63;
  if (row >= B) return;  // wave-uniform
  const ACT* lr = logits + (size_t)row * C;
  float mx = -INFINITY;
  int am = 0x7fffffff;
  for (int c = li; c < C; c += 64) {
    const float v = (float)lr[c];
    if (v > mx || am == 0x7fffffff) { mx = v; am = c; }  // ascending c: a tie keeps the lowest index
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mx, off, 64);
    const int oa = __shfl_xor(am, off, 64);
    if (oa != 0x7fffffff && (am == 0x7fffffff || om > mx || (om == mx && oa < am))) { mx = om; am = oa; }
  }
  float se = 0.f;
  for (int c = li; c < C; c += 64) se += expf((float)lr[c] - mx);
  se = wave_sum(se);
  const float inv = 1.0f / se;  // = the largest probability: exp(mx - mx) * inv
  float en = 0.f;
  for (int c = li; c < C; c += 64) {
    const float pv = expf((float)lr[c] - mx) * inv;
    en -= pv * logf(pv + CALIB_EPS);  // avuc_loss.py:68 epsilon (not the 1e-15 of utils/util.py)
  }
  en = wave_sum(en);
  if (li == 0) {
    float* r = rows + (size_t)row * CALIB_ROW_FLOATS;
    r[0] = inv;
    r[1] = en;
    r[2] = tanhf(en);
    r[3] = __int_as_float((am << 1) | (labels[row] == (long long)am ? 1 : 0));
    r[4] = mx;
  }
}

// ---- (2) the fold: one workgroup ------------------------------------------------------------------------------------
// MODE 0: AvU rows (K = 1 or 21);  1: EaU (a = error, b = unc);  2: EaC (a = error, b = conf)
template <int MODE>
__device__ __forceinline__ void calib_example(const float* __restrict__ rows, const float* __restrict__ a,
                                              const float* __restrict__ b, int i, float th_a, bool* good, float* s,
                                              float* wc, float* wu) {
  if (MODE == 0) {
    const float* r = rows + (size_t)i * CALIB_ROW_FLOATS;
    const float cf = r[0], t = r[2];
    *good = (__float_as_int(r[3]) & 1) != 0;
    *s = r[1];
    const float w = *good ? cf : 1.0f - cf;
    *wc = w * (1.0f - t);
    *wu = w * t;
  } else {
    const float e = a[i], o = b[i];
    const float te = tanhf(e);
    *good = e <= th_a;
    *s = o;
    const float w = *good ? 1.0f - te : te;
    if (MODE == 1) {
      const float tu = tanhf(o);
      *wc = w * (1.0f - tu);
      *wu = w * tu;
    } else {
      *wc = w * o;
      *wu = w * (1.0f - o);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(CALIB_FOLD_THREADS) void calib_fold_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                        int B, int K, float th_a, const float* __restrict__ th_a_dev,
                                                                        float th_b, const float* __restrict__ th_b_dev, float beta,
                                                                        float* __restrict__ out, float* __restrict__ ws) {
#pragma clang fp contract(off)
  __shared__ double part[CALIB_K_AREA][CALIB_FOLD_WAVES][4];
  __shared__ double th_s[CALIB_K_AREA];
  __shared__ double r_s[CALIB_K_AREA];
  __shared__ float mm_s[2][CALIB_FOLD_WAVES];
  const float* rows = ws + CALIB_HDR_FLOATS;
  const int wave = threadIdx.x >> 6, li = threadIdx.x & 63;
  if (th_a_dev) th_a = *th_a_dev;
  if (th_b_dev) th_b = *th_b_dev;
  if (K > 1) {  // area form: thresholds between the least and the most uncertain example (min / max are exact in any order)
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < B; i += CALIB_FOLD_THREADS) {
      const float h = rows[(size_t)i * CALIB_ROW_FLOATS + 1];
      lo = fminf(lo, h);
      hi = fmaxf(hi, h);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, off, 64));
      hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (li == 0) { mm_s[0][wave] = lo; mm_s[1][wave] = hi; }
    __syncthreads();
    if (threadIdx.x < K) {
      for (int w = 0; w < CALIB_FOLD_WAVES; ++w) { lo = fminf(lo, mm_s[0][w]); hi = fmaxf(hi, mm_s[1][w]); }
      const int k = threadIdx.x;
      // double from the f32 ends; the top threshold IS umax (no rounding coin flip for the most uncertain example)
      th_s[k] = (k == K - 1) ? (double)hi : (double)lo + ((double)k * 0.05) * ((double)hi - (double)lo);
    }
  } else if (threadIdx.x == 0) {
    th_s[0] = (double)th_b;
  }
  __syncthreads();
  // quadrant sums.  S slices of rows (slice s: rows s*64 + lane, + 64*S, ...), one wave per (threshold, slice) item.
  const int S = min(CALIB_FOLD_WAVES, (B + 63) / 64);
  for (int item = wave; item < K * S; item += CALIB_FOLD_WAVES) {  // wave-uniform
    const int k = item / S, s = item - k * S;
    const double th = th_s[k];
    double n[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = s * 64 + li; i < B; i += 64 * S) {
      bool good;
      float sv, wc, wu;
      calib_example<MODE>(rows, a, b, i, th_a, &good, &sv, &wc, &wu);
      const bool cert = (MODE == 2) ? ((double)sv > th) : ((double)sv <= th);
      const int q = (good ? 0 : 2) + (cert ? 0 : 1);
      const double w = (double)(cert ? wc : wu);
#pragma unroll
      for (int j = 0; j < 4; ++j) n[j] += (q == j) ? w : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) n[j] = wave_sum(n[j]);
    if (li == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) part[k][s][j] = n[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    double n[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) n[j] += part[k][s][j];
    const double num = n[0] + n[3];
    const double den = ((n[0] + n[1]) + (n[2] + n[3])) + 1e-10;
    r_s[k] = num / den;
    const double wk = (K == 1) ? 1.0 : ((k == 0 || k == K - 1) ? 0.025 : 0.05);  // trapezoid over linspace(0, 1, 21)
    float* G = ws + HDR_G + 4 * k;
    G[0] = (float)(wk * (den - num) / (den * den));
    G[1] = (float)(wk * (-num) / (den * den));
    G[2] = G[1];
    G[3] = G[0];
    ((double*)(ws + HDR_TH))[k] = th_s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = r_s[0];
    if (K > 1) {
      r = 0.0;
      for (int k = 0; k + 1 < K; ++k) r += 0.05 * (r_s[k] + r_s[k + 1]) * 0.5;
    }
    const float loss = (float)(-(double)beta * log(r + 1e-10));
    out[0] = loss;
    out[1] = (float)r;
    ws[HDR_LOSS] = loss;
    ws[HDR_R] = (float)r;
    ws[HDR_DLDR] = (float)(-(double)beta / (r + 1e-10));
    ws[HDR_K] = __int_as_float(K);
    ws[HDR_THA] = th_a;
  }
}

// ---- (3) backward ---------------------------------------------------------------------------------------------------
// d loss / d z_j = gs * (dc * conf * (delta_jm - p_j) + dH * p_j * (g_j - sum_l p_l g_l)),  g = dH / dp = -(log(p + eps) + p / (p + eps))
template <typename ACT>
__global__ __launch_bounds__(256) void avu_bwd_kernel(const ACT* __restrict__ logits, int B, int C, const float* __restrict__ g_loss,
                                                      const float* __restrict__ g_r, const float* __restrict__ ws,
                                                      ACT* __restrict__ dlogits) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), li = threadIdx.x & 63;
  if (row >= B) return;
  const float* r = ws + CALIB_HDR_FLOATS + (size_t)row * CALIB_ROW_FLOATS;
  const float cf = r[0], t = r[2], mx = r[4];
  const double H = (double)r[1];
  const int code = __float_as_int(r[3]);
  const bool good = code & 1;
  const int am = code >> 1;
  const int K = __float_as_int(ws[HDR_K]);
  const double* th = (const double*)(ws + HDR_TH);
  const float* G = ws + HDR_G;
  float sa = 0.f, su = 0.f;  // coefficients of the row's certain / uncertain weight, over the thresholds in order
  for (int k = 0; k < K; ++k) {
    if (H <= th[k]) sa += G[4 * k + (good ? 0 : 2)];
    else su += G[4 * k + (good ? 1 : 3)];
  }
  float gs = g_loss ? g_loss[0] * ws[HDR_DLDR] : 0.f;
  if (g_r) gs += g_r[0];
  // weight = w(conf) * (1 - t) certain, w(conf) * t uncertain;  w = conf (good) or 1 - conf
  const float w = good ? cf : 1.0f - cf;
  const float dc = (good ? 1.0f : -1.0f) * (sa * (1.0f - t) + su * t) * gs;
  const float dH = w * (su - sa) * (1.0f - t * t) * gs;
  const ACT* lr = logits + (size_t)row * C;
  ACT* dr = dlogits + (size_t)row * C;
  float sg = 0.f;
  for (int c = li; c < C; c += 64) {
    const float pv = expf((float)lr[c] - mx) * cf;
    sg -= pv * (logf(pv + CALIB_EPS) + pv / (pv + CALIB_EPS));
  }
  sg = wave_sum(sg);
  for (int c = li; c < C; c += 64) {
    const float pv = expf((float)lr[c] - mx) * cf;
    const float g = -(logf(pv + CALIB_EPS) + pv / (pv + CALIB_EPS));
    const float v = dc * cf * ((c == am ? 1.0f : 0.0f) - pv) + dH * pv * (g - sg);
    dr[c] = (ACT)v;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void eau_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int B,
                                                      const float* __restrict__ g_loss, const float* __restrict__ ws,
                                                      float* __restrict__ da, float* __restrict__ db) {
#pragma clang fp contract(off)
  const float th_a = ws[HDR_THA];
  const double th = ((const double*)(ws + HDR_TH))[0];
  const float gs = g_loss[0] * ws[HDR_DLDR];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
    const float e = a[i], o = b[i];
    const float te = tanhf(e);
    const bool good = e <= th_a;
    const bool cert = (MODE == 2) ? ((double)o > th) : ((double)o <= th);
    const float G = ws[HDR_G + (good ? 0 : 2) + (cert ? 0 : 1)] * gs;
    const float we = good ? 1.0f - te : te;
    const float dwe = (good ? -1.0f : 1.0f) * (1.0f - te * te);
    float wo, dwo;
    if (MODE == 1) {
      const float tu = tanhf(o);
      wo = cert ? 1.0f - tu : tu;
      dwo = (cert ? -1.0f : 1.0f) * (1.0f - tu * tu);
    } else {
      wo = cert ? o : 1.0f - o;
      dwo = cert ? 1.0f : -1.0f;
    }
    if (da) da[i] = G * dwe * wo;
    if (db) db[i] = G * we * dwo;
  }
}

}  // namespace

void btx::launch_avu_fold(int B, int area, float th, const float* th_dev, float beta, float* out, float* ws, hipStream_t st) {
  hipLaunchKernelGGL(calib_fold_kernel<0>, dim3(1), dim3(CALIB_FOLD_THREADS), 0, st, (const float*)nullptr, (const float*)nullptr,
                     B, area ? CALIB_K_AREA : 1, 0.f, (const float*)nullptr, th, th_dev, beta, out, ws);
}

extern "C" {

size_t btx_calib_workspace_bytes(int B) {
  if (B < 0) B = 0;
  return (size_t)CALIB_HDR_FLOATS * 4 + (size_t)B * CALIB_ROW_FLOATS * 4;
}

int btx_avu_fwd(const void* logits, const int64_t* labels, int B, int C, int act_dtype, int area, float th, const float* th_dev,
                float beta, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!logits || !labels || !out || !ws) return BTX_E_NULL;
  if (B <= 0 || C <= 0 || (area != 0 && area != 1)) return BTX_E_SHAPE;
  if (!act_esize(act_dtype)) return BTX_E_DTYPE;
  if (ws_bytes < btx_calib_workspace_bytes(B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;  // the header holds the thresholds as doubles
  hipStream_t st = (hipStream_t)stream;
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(avu_row_kernel<T>, dim3((B + 3) / 4), dim3(256), 0, st, (const T*)logits, (const long long*)labels, B, C,
                       (float*)ws + CALIB_HDR_FLOATS);
    btx::launch_avu_fold(B, area, th, th_dev, beta, out, (float*)ws, st);
  });
}

int btx_avu_bwd(const void* logits, int B, int C, int act_dtype, const float* g_loss, const float* g_r, const void* ws,
                size_t ws_bytes, void* dlogits, void* stream) {
  if (!logits || !ws || !dlogits || (!g_loss && !g_r)) return BTX_E_NULL;
  if (B <= 0 || C <= 0) return BTX_E_SHAPE;
  if (!act_esize(act_dtype)) return BTX_E_DTYPE;
  if (ws_bytes < btx_calib_workspace_bytes(B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;  // the header holds the thresholds as doubles
  return launch_by_act(act_dtype, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(avu_bwd_kernel<T>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const T*)logits, B, C, g_loss, g_r,
                       (const float*)ws, (T*)dlogits);
  });
}

int btx_eau_fwd(const float* error, const float* other, int B, int conf_form, float error_th, const float* error_th_dev,
                float other_th, const float* other_th_dev, float beta, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!error || !other || !out || !ws) return BTX_E_NULL;
  if (B <= 0 || (conf_form != 0 && conf_form != 1)) return BTX_E_SHAPE;
  if (ws_bytes < btx_calib_workspace_bytes(B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;  // the header holds the thresholds as doubles
  hipStream_t st = (hipStream_t)stream;
  if (conf_form)
    hipLaunchKernelGGL(calib_fold_kernel<2>, dim3(1), dim3(CALIB_FOLD_THREADS), 0, st, error, other, B, 1, error_th, error_th_dev,
                       other_th, other_th_dev, beta, out, (float*)ws);
  else
    hipLaunchKernelGGL(calib_fold_kernel<1>, dim3(1), dim3(CALIB_FOLD_THREADS), 0, st, error, other, B, 1, error_th, error_th_dev,
                       other_th, other_th_dev, beta, out, (float*)ws);
  return (int)hipGetLastError();
}

int btx_eau_bwd(const float* error, const float* other, int B, int conf_form, const float* g_loss, const void* ws, size_t ws_bytes, float* derror, float* dother, void* stream) {
  if (!error || !other || !g_loss || !ws || (!derror && !dother)) return BTX_E_NULL;
  if (B <= 0 || (conf_form != 0 && conf_form != 1)) return BTX_E_SHAPE;
  if (ws_bytes < btx_calib_workspace_bytes(B)) return BTX_E_WORKSPACE;
  if (((uintptr_t)ws) & 7) return BTX_E_ALIGN;  // the header holds the thresholds as doubles
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(min((B + 255) / 256, 1024));
  if (conf_form)
    hipLaunchKernelGGL(eau_bwd_kernel<2>, grid, dim3(256), 0, st, error, other, B, g_loss, (const float*)ws, derror,
                       dother);
  else
    hipLaunchKernelGGL(eau_bwd_kernel<1>, grid, dim3(256), 0, st, error, other, B, g_loss, (const float*)ws, derror,
                       dother);
  return (int)hipGetLastError();
}

}  // extern "C"
