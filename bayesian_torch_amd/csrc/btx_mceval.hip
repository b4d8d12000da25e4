// K15: Monte-Carlo evaluation head (BTX-EVAL v1): from the packed MC statistics and the labels of a batch to
// top-1 / top-k hits, NLL, Brier, predictive entropy, mutual information, ECE bins and the AvU quadrant counts, folded into a
// float64 state on the device.  Two launches on the caller's stream and no host read.  Reference (host code with numpy and a
// Python loop per example): examples/main_bayesian_imagenet.py:549-642 (validate / evaluate), utils/util.py:41-60,
// utils/avuc_loss.py:392-443 (eval_avu / accuracy_vs_uncertainty).
//
// Launches: (1) mceval_row_kernel, one workgroup per batch row: ONE pass over the row of sum_p (p_y is read directly, so the
// rank, the Brier score and the entropy need no second pass and nothing is staged in LDS); it writes the row's record of 8
// floats into the workspace and, below `capacity`, into the record buffer at the state's cursor.  (2) mceval_fold_kernel, ONE
// workgroup: widens the records to double and adds them to the state.
// Determinism: a row sum is a thread's strided partial (c = t, t + 256, ...), a xor butterfly inside the wave (both partners add
// the same two numbers, so every lane holds the same bits) and (w0 + w1) + (w2 + w3) over the four waves; a state sum is a
// lane's strided partial over the rows (i = lane, lane + 64, ...) and the same butterfly.  Shapes fixed by C and bs alone, no
// atomics, no "last block" counters.  Every load and store is element-wise: any 4-byte aligned packed / workspace / records.
// The butterfly is wave_sum of btx_heads.h; the pairwise sum over the four waves is spelled out in the row kernel, which folds five
// quantities behind ONE barrier (block_sum_pairwise4 would take one per quantity).
#include "btx_heads.h"

#define EVAL_EPS 1e-15f
#define EVAL_ROW_THREADS 256
#define EVAL_FOLD_THREADS 1024
#define EVAL_FOLD_WAVES 16

namespace {

// the ECE bin of a confidence: right-closed bins ((b / nbins, (b + 1) / nbins])
__device__ __forceinline__ int eval_bin(float conf, int nbins) {
  const float e = ceilf(conf * (float)nbins);
  int b = (e >= 1.0f) ? (int)fminf(e, 65.0f) - 1 : 0;  // NaN and anything below one land in bin 0
  return min(b, nbins - 1);
}

// ---- (1) one workgroup per row --------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_ROW_THREADS) void mceval_row_kernel(const float* __restrict__ packed,
                                                                      const long long* __restrict__ labels, int bs, int C,
                                                                      const double* __restrict__ state, float* __restrict__ rows,
                                                                      float* __restrict__ records, long long capacity) {
#pragma clang fp contract(off)
  __shared__ float sm_mx[4];
  __shared__ int sm_am[4];
  __shared__ int sm_rk[4];
  __shared__ float sm_h[4];
  __shared__ float sm_b[4];
  const int row = blockIdx.x, t = threadIdx.x, wave = t >> 6, li = t & 63;
  const size_t bc = (size_t)bs * C;
  const float* sp = packed + (size_t)row * C;
  const float n = packed[2 * bc + bs + 1];
  const long long y = labels[row];
  const bool valid = y >= 0 && y < (long long)C;
  const int yi = valid ? (int)y : -1;
  const float py = valid ? sp[yi] / n : 0.f;
  float mx = -INFINITY, hs = 0.f, br = 0.f;
  int am = 0x7fffffff, rk = 0;
  for (int c = t; c < C; c += EVAL_ROW_THREADS) {
    const float p = sp[c] / n;
    if (p > mx || am == 0x7fffffff) { mx = p; am = c; }  // ascending c: a tie keeps the lowest index
    rk += (p > py || (p == py && c < yi)) ? 1 : 0;
    hs += p * logf(p + EVAL_EPS);
    const float d = p - (c == yi ? 1.0f : 0.0f);
    br += d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(mx, off, 64);
    const int oa = __shfl_xor(am, off, 64);
    if (oa != 0x7fffffff && (am == 0x7fffffff || om > mx || (om == mx && oa < am))) { mx = om; am = oa; }
  }
  rk = wave_sum(rk);
  hs = wave_sum(hs);
  br = wave_sum(br);
  if (li == 0) { sm_mx[wave] = mx; sm_am[wave] = am; sm_rk[wave] = rk; sm_h[wave] = hs; sm_b[wave] = br; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      const float om = sm_mx[w];
      const int oa = sm_am[w];
      if (oa != 0x7fffffff && (am == 0x7fffffff || om > mx || (om == mx && oa < am))) { mx = om; am = oa; }
    }
    const int rank = (sm_rk[0] + sm_rk[1]) + (sm_rk[2] + sm_rk[3]);
    const float H = -((sm_h[0] + sm_h[1]) + (sm_h[2] + sm_h[3]));
    const float brier = (sm_b[0] + sm_b[1]) + (sm_b[2] + sm_b[3]);
    const float MI = H - packed[2 * bc + row] / n;
    float rec[8];
    rec[0] = (float)am;
    rec[1] = valid ? (float)rank : -1.0f;
    rec[2] = mx;
    rec[3] = py;
    rec[4] = valid ? -logf(py + EVAL_EPS) : 0.f;
    rec[5] = valid ? brier : 0.f;
    rec[6] = H;
    rec[7] = MI;
    float* r = rows + (size_t)row * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = rec[j];
    if (records) {
      const long long at = (long long)state[BTX_MC_EVAL_CURSOR] + row;
      if (at >= 0 && at < capacity) {
        float* q = records + (size_t)at * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = rec[j];
      }
    }
  }
}

// ---- (2) the fold: one workgroup ------------------------------------------------------------------------------------
// item 0: the eleven scalars; items 1 .. nbins: one ECE bin each; items nbins + 1 .. nbins + T: one threshold each.  A wave takes
// the items wave, wave + 16, ...; no two waves touch the same state word.
__global__ __launch_bounds__(EVAL_FOLD_THREADS) void mceval_fold_kernel(const float* __restrict__ rows, int bs, int topk, int nbins,
                                                                        const float* __restrict__ th, int T, int use_mi,
                                                                        double* __restrict__ state, long long capacity) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, li = threadIdx.x & 63;
  for (int item = wave; item < 1 + nbins + T; item += EVAL_FOLD_WAVES) {  // wave-uniform
    if (item == 0) {
      double a[11];
#pragma unroll
      for (int j = 0; j < 11; ++j) a[j] = 0.0;
      for (int i = li; i < bs; i += 64) {
        const float* r = rows + (size_t)i * 8;
        const float rank = r[1];
        const bool valid = rank >= 0.f, hit = rank == 0.f;
        const double u = (double)(use_mi ? r[7] : r[6]);
        a[0] += valid ? 1.0 : 0.0;
        a[1] += valid ? 0.0 : 1.0;
        a[2] += hit ? 1.0 : 0.0;
        a[3] += (valid && rank < (float)topk) ? 1.0 : 0.0;
        a[4] += valid ? (double)r[4] : 0.0;
        a[5] += valid ? (double)r[5] : 0.0;
        a[6] += valid ? (double)r[6] : 0.0;
        a[7] += valid ? (double)r[7] : 0.0;
        a[8] += valid ? (double)r[2] : 0.0;
        a[9] += hit ? u : 0.0;
        a[10] += (valid && !hit) ? u : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 11; ++j) a[j] = wave_sum(a[j]);
      if (li == 0) {
#pragma unroll
        for (int j = 0; j < 11; ++j) state[j] += a[j];
      }
    } else if (item <= nbins) {
      const int b = item - 1;
      double a[3] = {0.0, 0.0, 0.0};
      for (int i = li; i < bs; i += 64) {
        const float* r = rows + (size_t)i * 8;
        const bool in = r[1] >= 0.f && eval_bin(r[2], nbins) == b;
        a[0] += in ? 1.0 : 0.0;
        a[1] += in ? (double)r[2] : 0.0;
        a[2] += (in && r[1] == 0.f) ? 1.0 : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) a[j] = wave_sum(a[j]);
      if (li == 0) {
        double* s = state + BTX_MC_EVAL_HEADER + 3 * b;
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += a[j];
      }
    } else {
      const int k = item - 1 - nbins;
      const float thk = th[k];
      double a[4] = {0.0, 0.0, 0.0, 0.0};
      for (int i = li; i < bs; i += 64) {
        const float* r = rows + (size_t)i * 8;
        const bool valid = r[1] >= 0.f, hit = r[1] == 0.f;
        const bool cert = (use_mi ? r[7] : r[6]) <= thk;
        const int q = (hit ? 0 : 2) + (cert ? 0 : 1);  // n_ac, n_au, n_ic, n_iu
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (valid && q == j) ? 1.0 : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = wave_sum(a[j]);
      if (li == 0) {
        double* s = state + BTX_MC_EVAL_HEADER + 3 * nbins + 4 * k;
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += a[j];
      }
    }
  }
  if (threadIdx.x == EVAL_FOLD_THREADS - 1) {  // the cursor is touched by this thread alone (the scalars stop at word 10)
    const double cur = state[BTX_MC_EVAL_CURSOR];
    const double over = cur + (double)bs - (double)capacity;
    state[BTX_MC_EVAL_DROPPED] += fmin(fmax(over, 0.0), (double)bs);
    state[BTX_MC_EVAL_CURSOR] = cur + (double)bs;
  }
}

}  // namespace

extern "C" {

size_t btx_mc_eval_state_doubles(int nbins, int T) {
  if (nbins < 1 || nbins > BTX_MC_EVAL_MAX_BINS || T < 0 || T > BTX_MC_EVAL_MAX_THRESHOLDS) return 0;
  return (size_t)BTX_MC_EVAL_HEADER + 3 * (size_t)nbins + 4 * (size_t)T;
}

size_t btx_mc_eval_workspace_bytes(int bs) {
  if (bs < 0) bs = 0;
  return (size_t)bs * 8 * sizeof(float);
}

int btx_mc_eval(const float* packed, const int64_t* labels, int bs, int C, int topk, int nbins, const float* th, int T, int use_mi,
                double* state, size_t state_doubles, float* records, int64_t capacity, void* ws, size_t ws_bytes, void* stream) {
  if (!packed || !labels || !state || !ws || (T > 0 && !th) || (capacity > 0 && !records)) return BTX_E_NULL;
  if (bs <= 0 || C <= 0 || topk < 1 || nbins < 1 || nbins > BTX_MC_EVAL_MAX_BINS || T < 0 || T > BTX_MC_EVAL_MAX_THRESHOLDS ||
      capacity < 0 || (use_mi != 0 && use_mi != 1))
    return BTX_E_SHAPE;
  if (C > BTX_MC_EVAL_MAX_CLASSES) return BTX_E_UNSUPPORTED;
  if (ws_bytes < btx_mc_eval_workspace_bytes(bs) || state_doubles < btx_mc_eval_state_doubles(nbins, T)) return BTX_E_WORKSPACE;
  if ((((uintptr_t)packed) & 3) || (((uintptr_t)ws) & 3) || (((uintptr_t)records) & 3) || (((uintptr_t)th) & 3) ||
      (((uintptr_t)labels) & 7) || (((uintptr_t)state) & 7))
    return BTX_E_ALIGN;  // the natural alignment of the element types: no valid tensor ends here
  hipStream_t st = (hipStream_t)stream;
  if (capacity == 0) records = nullptr;
  hipLaunchKernelGGL(mceval_row_kernel, dim3(bs), dim3(EVAL_ROW_THREADS), 0, st, packed, (const long long*)labels, bs, C,
                     (const double*)state, (float*)ws, records, (long long)capacity);
  hipLaunchKernelGGL(mceval_fold_kernel, dim3(1), dim3(EVAL_FOLD_THREADS), 0, st, (const float*)ws, bs, topk, nbins, th, T, use_mi,
                     state, (long long)capacity);
  return (int)hipGetLastError();
}

}  // extern "C"
