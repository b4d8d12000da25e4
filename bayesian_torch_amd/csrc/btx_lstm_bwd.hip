// btx_lstm_bwd.hip — backward through time of the fused Bayesian LSTM (btx_lstm_bwd) for gfx950.
//
// The backward of one btx_lstm_fwd_train call (one lane), enqueued from C++ on the caller's stream, so it can be captured:
//
//   * T step launches, t = T-1 .. 0 (lstm_bwd_kernel, MODE 0):
//       dh_t = d hidden_seq[:, t] + dgates_{t+1} . W_hh(s+t+1)           (no recurrent term for t = T-1)
//       dc_t = d c_seq[:, t] + dc_{t+1} * f_{t+1} + dh_t * o_t * (1 - tanh^2 c_t)
//       dgates_t = (dc_t g_t, dc_t c_{t-1}, dc_t i_t, dh_t tanh c_t) * the gate derivatives   -> f32 workspace [T][B][4H]
//     A workgroup owns BJ hidden units j (columns of W_hh) and BB batch rows.  Per chunk of BNC gate rows n it samples
//     W_hh[n][j0 .. j0+BJ) from (mu, rho) in registers into LDS (the sampled weight never exists in HBM): four threads per row
//     read 64 contiguous bytes of the [4H][H] parameters.  Wave w owns columns j0 + 4w .. + 3 for its 64 batch lanes and
//     walks n in order: one fixed f32 FMA chain per output.  Flipout adds s_in(b,k) . sum_n (dg o s_out)(b,n) Delta(n,k).
//   * dh0 / dc0 (MODE 2): the same contraction with dgates_0 and W_hh(s); dc0 = dc_0 * f_0 (the carry after step 0).
//   * the input gradient of every step in one launch (MODE 1): dx_t = dgates_t . W_ih(s+t), written in the activation dtype.
//   * one weight-gradient launch per layer (lstm_wgrad_kernel): a workgroup owns a 16 x 64 tile of the [4H][K] weight and walks
//     t = 0 .. T-1 and the batch in a fixed order (no atomics).  Per step it forms dW_t = dg_t^T in_t (in = x_t, or h_{t-1}: h0 or
//     zeros for t = 0), regenerates eps_t of its tile with the forward's indices, and accumulates dmu += dW_t and
//     sum_t dW_t o eps_t (Flipout: dDelta_t = (dg_t o s_out)^T (in_t o s_in)); drho = that sum * sigmoid(rho).  The workgroups of
//     the first k tile also form the bias gradients.
//
// Noise indices are the forward's (btx_lstm.hip): eps_w element n*Kr + k, eps_b element n, s_in element b*Kr + k, s_out element
// b*4H + n, all keyed on sample index s + t of the layer.  Precision: f32 = f32 FMA chains; bf16 = the operands the forward
// rounds (x, h, the sampled W / mu / Delta) rounded to bf16, gradients and accumulation in f32.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/btx.h"
#include "btx_rng.h"

namespace {

constexpr int BJ = 16;          // columns k per workgroup of the contraction kernel (4 per wave)
constexpr int BB = 64;          // batch rows per workgroup: lane b of every wave
constexpr int BNC = 64;         // gate rows n per LDS chunk
constexpr int BXS = BNC + 4;    // padded dgates row (floats): conflict-free ds_read_b128 across b
constexpr int WN = 16;          // weight-gradient tile: gate rows
constexpr int WK = 64;          //   and columns (one normal4 group per thread)

struct LstmBArgs {
  const float* mu_w;            // the contracted layer: hh (MODE 0 / 2) or ih (MODE 1), [4H][K]
  const float* rho_w;
  const uint32_t* sample_dev;   // one word, or null: sample
  uint32_t sample, layer, k0, k1;
  int B, K, Kr, H, T, t, kblocks;
  float* dG;                    // [T][B][4H] f32 dgates
  const float* sg;              // saved gate pre-activations [T][B][4H]
  const float* sc;              // saved f32 cell states [T][B][H]
  const void* c0;               // [B][H] or null
  const void* dhs;              // d hidden_seq [B][T][H] or null
  const void* dcs;              // d c_seq or null
  float* dcc;                   // [B][H] f32 carry dc_t * f_t
  void* out;                    // MODE 1: dx [B][T][K]; MODE 2: dh0 [B][H] (or null)
  void* out2;                   // MODE 2: dc0 [B][H] (or null)
};

struct LstmWArgs {
  const float* rho_w;           // [4H][K]
  const float* rho_b;           // [4H] or null
  const uint32_t* sample_dev;
  uint32_t sample, layer, k0, k1;
  int B, K, Kr, H, T, hh;       // hh: the input of step t is h_{t-1} (hidden_seq[:, t-1], h0 or zeros); else x_t
  const void* in;               // x [B][T][I] or hidden_seq [B][T][H]
  const void* h0;               // [B][H] or null
  const float* dG;
  float* dmu_w;
  float* drho_w;
  float* dmu_b;                 // or null
  float* drho_b;
};

template <typename T> __device__ __forceinline__ float ld_f(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st_f(T* p, float v) { *p = (T)v; }
__device__ __forceinline__ float rbf(float v) { return (float)(__bf16)v; }

__device__ __forceinline__ bool sign_neg(uint32_t idx, uint32_t ka, uint32_t kb) {
  return (btx_sign_word(idx >> 5, ka, kb) >> btx_sign_bitpos(idx & 31u)) & 1u;
}

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

// MODE 0: recurrent step t (grid.x = kblocks over H); 1: input gradient of all steps (grid.x = kblocks over I * T);
// 2: dh0 / dc0.  grid.y = batch blocks.
template <int FLIP, int BFP, typename XT, int MODE>
__global__ __launch_bounds__(256) void lstm_bwd_kernel(LstmBArgs a) {
  __shared__ __attribute__((aligned(16))) float gs[BB * BXS];
  __shared__ __attribute__((aligned(16))) float gd[FLIP ? BB * BXS : 4];
  __shared__ __attribute__((aligned(16))) float ws[BNC * BJ];
  __shared__ __attribute__((aligned(16))) float wd[FLIP ? BNC * BJ : 4];

  const int tid = threadIdx.x, lane_b = tid & 63, wave = tid >> 6;
  int kb, t;
  if (MODE == 1) {
    t = blockIdx.x / a.kblocks;
    kb = blockIdx.x - t * a.kblocks;
  } else {
    kb = blockIdx.x; t = a.t;
  }
  const int k0 = kb * BJ, b0 = blockIdx.y * BB, gb = b0 + lane_b;
  const int B = a.B, K = a.K, Kr = a.Kr, H = a.H, N4 = 4 * H, T = a.T;
  // the step whose dgates and weight sample are contracted: t + 1 (recurrent term of step t), t (dx_t), 0 (dh0)
  const int tc = MODE == 0 ? t + 1 : (MODE == 1 ? t : 0);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, accd[4] = {0.f, 0.f, 0.f, 0.f};
  if (tc < T) {
    uint32_t s = a.sample_dev ? __builtin_amdgcn_readfirstlane(a.sample_dev[0]) : a.sample;
    s += (uint32_t)tc;
    uint32_t koa = 0, kob = 0;
    if (FLIP) {
      const BtxPhilox4 k = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_OUT, a.k0, a.k1);
      koa = k.x[0]; kob = k.x[1];
    }
    const float* dg = a.dG + (long long)tc * B * N4;
    const int sr = tid >> 2, sk = k0 + (tid & 3) * 4;  // sampler role: chunk row sr, columns sk .. sk + 3
    for (int nc = 0; nc < N4; nc += BNC) {
      // ---- stage dgates[b][nc .. nc + BNC) (zero outside [B) x [4H)); Flipout also dg o s_out
#pragma unroll
      for (int e = 0; e < BB * BNC / 256; ++e) {
        const int idx = tid + e * 256, b = idx / BNC, nn = idx - b * BNC, g_b = b0 + b, n = nc + nn;
        const bool ok = g_b < B && n < N4;
        const float v = ok ? dg[(long long)g_b * N4 + n] : 0.f;
        gs[b * BXS + nn] = v;
        if (FLIP) gd[b * BXS + nn] = (ok && sign_neg((uint32_t)g_b * (uint32_t)N4 + (uint32_t)n, koa, kob)) ? -v : v;
      }
      // ---- sample W[nc + sr][sk .. sk + 3] in registers, to LDS only (the forward's values, bit for bit)
      {
        float wv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
        const int n = nc + sr;
        if (n < N4 && sk < K) {
          float z[4];
          btx_normal4_hw(((uint32_t)n * (uint32_t)Kr + (uint32_t)sk) >> 2, s, a.layer, BTX_STREAM_EPS_W, a.k0, a.k1, z);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (sk + i < K) {
              const long long o = (long long)n * K + sk + i;
              const float mu = a.mu_w[o], d = btx_softplus_hw(a.rho_w[o]) * z[i];
              if (FLIP) { wv[i] = mu; dv[i] = d; }
              else wv[i] = mu + d;
            }
          }
        }
        const int sq = (tid & 3) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ws[sr * BJ + sq + i] = BFP ? rbf(wv[i]) : wv[i];
          if (FLIP) wd[sr * BJ + sq + i] = BFP ? rbf(dv[i]) : dv[i];
        }
      }
      __syncthreads();
      // ---- contract: lane b, wave w -> columns k0 + 4w .. + 3, n in order
#pragma unroll 4
      for (int nn = 0; nn < BNC; nn += 4) {
        const float4 gv = *(const float4*)&gs[lane_b * BXS + nn];
        float4 gdv = gv;
        if (FLIP) gdv = *(const float4*)&gd[lane_b * BXS + nn];
        const float gu[4] = {gv.x, gv.y, gv.z, gv.w}, gdu[4] = {gdv.x, gdv.y, gdv.z, gdv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 w = *(const float4*)&ws[(nn + u) * BJ + wave * 4];
          acc[0] = fmaf(gu[u], w.x, acc[0]); acc[1] = fmaf(gu[u], w.y, acc[1]);
          acc[2] = fmaf(gu[u], w.z, acc[2]); acc[3] = fmaf(gu[u], w.w, acc[3]);
          if (FLIP) {
            const float4 d = *(const float4*)&wd[(nn + u) * BJ + wave * 4];
            accd[0] = fmaf(gdu[u], d.x, accd[0]); accd[1] = fmaf(gdu[u], d.y, accd[1]);
            accd[2] = fmaf(gdu[u], d.z, accd[2]); accd[3] = fmaf(gdu[u], d.w, accd[3]);
          }
        }
      }
      __syncthreads();
    }
    if (FLIP) {
      const BtxPhilox4 k = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_IN, a.k0, a.k1);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = k0 + wave * 4 + i;
        const bool neg = gb < B && kk < K && sign_neg((uint32_t)gb * (uint32_t)Kr + (uint32_t)kk, k.x[0], k.x[1]);
        acc[i] = neg ? acc[i] - accd[i] : acc[i] + accd[i];
      }
    }
  }
  if (gb >= B) return;

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + wave * 4 + i;
    if (k >= K) break;
    if (MODE == 1) {
      st_f((XT*)a.out + ((long long)gb * T + t) * K + k, acc[i]);
    } else if (MODE == 2) {
      if (a.out) st_f((XT*)a.out + (long long)gb * H + k, acc[i]);
      if (a.out2) st_f((XT*)a.out2 + (long long)gb * H + k, a.dcc[(long long)gb * H + k]);
    } else {
      // ---- gate / cell backward of hidden unit j = k, batch row gb
      const int j = k;
      float dh = acc[i];
      if (a.dhs) dh += ld_f((const XT*)a.dhs + ((long long)gb * T + t) * H + j);
      const float* g = a.sg + ((long long)t * B + gb) * N4 + j;
      const float ig = sigm(g[0]), fg = sigm(g[H]), gg = tanhf(g[2 * H]), og = sigm(g[3 * H]);
      const float c = a.sc[((long long)t * B + gb) * H + j];
      float cp = 0.f;
      if (t > 0) cp = a.sc[((long long)(t - 1) * B + gb) * H + j];
      else if (a.c0) cp = ld_f((const XT*)a.c0 + (long long)gb * H + j);
      const float th = tanhf(c);
      float dc = dh * og * (1.f - th * th);
      if (a.dcs) dc += ld_f((const XT*)a.dcs + ((long long)gb * T + t) * H + j);
      if (t + 1 < T) dc += a.dcc[(long long)gb * H + j];
      float* d = a.dG + ((long long)t * B + gb) * N4 + j;
      d[0] = dc * gg * (ig * (1.f - ig));
      d[H] = dc * cp * (fg * (1.f - fg));
      d[2 * H] = dc * ig * (1.f - gg * gg);
      d[3 * H] = dh * th * (og * (1.f - og));
      a.dcc[(long long)gb * H + j] = dc * fg;
    }
  }
}

// grid.x = 4H / WN row tiles, grid.y = K / WK column tiles.  Thread: gate row n0 + (tid >> 4), columns kt + (tid & 15) * 4 .. + 3.
template <int FLIP, int BFP, typename XT>
__global__ __launch_bounds__(256) void lstm_wgrad_kernel(LstmWArgs a) {
  __shared__ __attribute__((aligned(16))) float gl[BB * WN];
  __shared__ __attribute__((aligned(16))) float gld[FLIP ? BB * WN : 4];
  __shared__ __attribute__((aligned(16))) float il[BB * WK];
  __shared__ __attribute__((aligned(16))) float ild[FLIP ? BB * WK : 4];

  const int tid = threadIdx.x;
  const int B = a.B, K = a.K, Kr = a.Kr, H = a.H, N4 = 4 * H, T = a.T;
  const int n0 = blockIdx.x * WN, kt = blockIdx.y * WK;
  const int nl = tid >> 4, kq = (tid & 15) * 4, n = n0 + nl, kk = kt + kq;
  const bool bias_thr = a.dmu_b && blockIdx.y == 0 && (tid & 15) == 0;
  const uint32_t s0 = a.sample_dev ? __builtin_amdgcn_readfirstlane(a.sample_dev[0]) : a.sample;
  float dmu[4] = {0.f, 0.f, 0.f, 0.f}, se[4] = {0.f, 0.f, 0.f, 0.f};
  float bm = 0.f, bs = 0.f;
  for (int t = 0; t < T; ++t) {
    const uint32_t s = s0 + (uint32_t)t;
    uint32_t ka = 0, kb = 0, koa = 0, kob = 0;
    if (FLIP) {
      const BtxPhilox4 ki = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_IN, a.k0, a.k1);
      const BtxPhilox4 ko = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_OUT, a.k0, a.k1);
      ka = ki.x[0]; kb = ki.x[1]; koa = ko.x[0]; kob = ko.x[1];
    }
    const XT* src = nullptr;
    long long srow = 0;
    if (!a.hh) { src = (const XT*)a.in + (long long)t * K; srow = (long long)T * K; }
    else if (t > 0) { src = (const XT*)a.in + (long long)(t - 1) * K; srow = (long long)T * K; }
    else if (a.h0) { src = (const XT*)a.h0; srow = K; }
    const float* dg = a.dG + (long long)t * B * N4;
    float aw[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
    float ab = 0.f, abd = 0.f;
    for (int bc = 0; bc < B; bc += BB) {
      // ---- stage dg[b][n0 .. n0 + WN) and in[b][kt .. kt + WK) (zero outside the tensors); Flipout also their signed copies
#pragma unroll
      for (int e = 0; e < BB * WN / 256; ++e) {
        const int idx = tid + e * 256, b = idx / WN, nn = idx - b * WN, g_b = bc + b, gn = n0 + nn;
        const bool ok = g_b < B && gn < N4;
        const float v = ok ? dg[(long long)g_b * N4 + gn] : 0.f;
        gl[idx] = v;
        if (FLIP) gld[idx] = (ok && sign_neg((uint32_t)g_b * (uint32_t)N4 + (uint32_t)gn, koa, kob)) ? -v : v;
      }
#pragma unroll
      for (int e = 0; e < BB * WK / 256; ++e) {
        const int idx = tid + e * 256, b = idx / WK, k2 = idx - b * WK, g_b = bc + b, k = kt + k2;
        const bool ok = src && g_b < B && k < K;
        float v = ok ? ld_f(src + g_b * srow + k) : 0.f;
        if (BFP) v = rbf(v);
        il[idx] = v;
        if (FLIP) ild[idx] = (ok && sign_neg((uint32_t)g_b * (uint32_t)Kr + (uint32_t)k, ka, kb)) ? -v : v;
      }
      __syncthreads();
#pragma unroll 4
      for (int b = 0; b < BB; ++b) {
        const float g = gl[b * WN + nl];
        const float4 xv = *(const float4*)&il[b * WK + kq];
        aw[0] = fmaf(g, xv.x, aw[0]); aw[1] = fmaf(g, xv.y, aw[1]);
        aw[2] = fmaf(g, xv.z, aw[2]); aw[3] = fmaf(g, xv.w, aw[3]);
        float gdd = g;
        if (FLIP) {
          gdd = gld[b * WN + nl];
          const float4 xd = *(const float4*)&ild[b * WK + kq];
          ad[0] = fmaf(gdd, xd.x, ad[0]); ad[1] = fmaf(gdd, xd.y, ad[1]);
          ad[2] = fmaf(gdd, xd.z, ad[2]); ad[3] = fmaf(gdd, xd.w, ad[3]);
        }
        if (bias_thr) { ab += g; abd += gdd; }
      }
      __syncthreads();
    }
    // ---- fold step t: dmu += dW_t, sum += dW_t (Flipout dDelta_t) o eps_t
    if (n < N4 && kk < K) {
      float z[4];
      btx_normal4_hw(((uint32_t)n * (uint32_t)Kr + (uint32_t)kk) >> 2, s, a.layer, BTX_STREAM_EPS_W, a.k0, a.k1, z);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dmu[i] += aw[i];
        se[i] = fmaf(FLIP ? ad[i] : aw[i], z[i], se[i]);
      }
    }
    if (bias_thr && n < N4) {
      const float eb = btx_normal1((unsigned long long)n, s, a.layer, BTX_STREAM_EPS_B, a.k0, a.k1);
      bm += ab;
      bs = fmaf(FLIP ? abd : ab, eb, bs);
    }
  }
  if (n >= N4) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (kk + i < K) {
      const long long o = (long long)n * K + kk + i;
      a.dmu_w[o] = dmu[i];
      a.drho_w[o] = se[i] * sigm(a.rho_w[o]);
    }
  }
  if (bias_thr) {
    a.dmu_b[n] = bm;
    a.drho_b[n] = bs * sigm(a.rho_b[n]);
  }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

template <int FLIP, int BFP, typename XT>
hipError_t launch_bwd(LstmBArgs sa, LstmBArgs xa, LstmWArgs wi, LstmWArgs wh, bool want_h0, bool want_x, bool want_wi,
                      bool want_wh, int bblocks, hipStream_t st) {
  hipError_t e;
  for (int t = sa.T - 1; t >= 0; --t) {
    sa.t = t;
    hipLaunchKernelGGL((lstm_bwd_kernel<FLIP, BFP, XT, 0>), dim3(sa.kblocks, bblocks), dim3(256), 0, st, sa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (want_h0) {
    hipLaunchKernelGGL((lstm_bwd_kernel<FLIP, BFP, XT, 2>), dim3(sa.kblocks, bblocks), dim3(256), 0, st, sa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (want_x) {
    hipLaunchKernelGGL((lstm_bwd_kernel<FLIP, BFP, XT, 1>), dim3(xa.kblocks * xa.T, bblocks), dim3(256), 0, st, xa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int nt = (4 * sa.H + WN - 1) / WN;
  if (want_wi) {
    hipLaunchKernelGGL((lstm_wgrad_kernel<FLIP, BFP, XT>), dim3(nt, (wi.K + WK - 1) / WK), dim3(256), 0, st, wi);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (want_wh) {
    hipLaunchKernelGGL((lstm_wgrad_kernel<FLIP, BFP, XT>), dim3(nt, (wh.K + WK - 1) / WK), dim3(256), 0, st, wh);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

int check_grads(const BtxLstmGrads* g, const BtxLstmLayer* l) {
  if (!g) return 0;
  if (!g->dmu_w || !g->drho_w) return BTX_E_NULL;
  if ((g->dmu_b == nullptr) != (g->drho_b == nullptr)) return BTX_E_NULL;
  if (g->dmu_b && !l->mu_b) return BTX_E_NULL;  // bias gradients of a layer without bias
  return 0;
}

}  // namespace

extern "C" {

int btx_lstm_bwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, const void* h0,
                 const void* c0, const void* hidden_seq, const void* saved, const void* d_hidden_seq, const void* d_c_seq,
                 void* dx, void* dh0, void* dc0, const BtxLstmGrads* g_ih, const BtxLstmGrads* g_hh, int B, int I, int H, int T,
                 int act_dtype, int prec, void* workspace, size_t ws_bytes, void* stream) {
  if (!ih || !hh || !x || !hidden_seq || !saved || !workspace) return BTX_E_NULL;
  if (!ih->mu_w || !ih->rho_w || !hh->mu_w || !hh->rho_w) return BTX_E_NULL;
  if ((ih->mu_b == nullptr) != (ih->rho_b == nullptr) || (hh->mu_b == nullptr) != (hh->rho_b == nullptr)) return BTX_E_NULL;
  if ((h0 == nullptr) != (c0 == nullptr)) return BTX_E_NULL;
  int rc;
  if ((rc = check_grads(g_ih, ih)) != 0 || (rc = check_grads(g_hh, hh)) != 0) return rc;
  if (kind != BTX_KIND_REPARAM && kind != BTX_KIND_FLIPOUT) return BTX_E_UNSUPPORTED;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // as the forward: f32 and bf16 forms only
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16) return BTX_E_DTYPE;
  if (B <= 0 || I <= 0 || H <= 0 || T <= 0) return BTX_E_SHAPE;
  const int Ir = I % 8 ? (I + 7) / 8 * 8 : I, Hr = H % 8 ? (H + 7) / 8 * 8 : H;
  if ((uint64_t)4 * H * Ir > 0xfffffff0ull || (uint64_t)4 * H * Hr > 0xfffffff0ull || (uint64_t)B * 4 * H > 0xfffffff0ull ||
      (uint64_t)B * Ir > 0xfffffff0ull)
    return BTX_E_UNSUPPORTED;
  const uint64_t hblocks = ((uint64_t)H + BJ - 1) / BJ, iblocks = ((uint64_t)I + BJ - 1) / BJ;
  const uint64_t bblocks = ((uint64_t)B + BB - 1) / BB;
  if (iblocks * T > 0x7fffffffull || bblocks > 65535 || ((uint64_t)I + WK - 1) / WK > 65535 ||
      ((uint64_t)H + WK - 1) / WK > 65535)
    return BTX_E_UNSUPPORTED;
  if (ws_bytes < btx_lstm_train_workspace_bytes(B, H, T)) return BTX_E_WORKSPACE;

  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  float* dG = (float*)workspace;
  LstmBArgs sa = {};
  sa.mu_w = hh->mu_w; sa.rho_w = hh->rho_w;
  sa.sample_dev = (const uint32_t*)hh->sample_idx_dev; sa.sample = hh->sample_idx; sa.layer = hh->layer_id;
  sa.k0 = k0; sa.k1 = k1;
  sa.B = B; sa.K = H; sa.Kr = Hr; sa.H = H; sa.T = T; sa.kblocks = (int)hblocks;
  sa.dG = dG;
  sa.sg = (const float*)saved;
  sa.sc = (const float*)((const char*)saved + align256((size_t)T * B * 4 * H * sizeof(float)));
  sa.c0 = c0; sa.dhs = d_hidden_seq; sa.dcs = d_c_seq;
  sa.dcc = (float*)((char*)workspace + align256((size_t)T * B * 4 * H * sizeof(float)));
  sa.out = dh0; sa.out2 = dc0;
  LstmBArgs xa = sa;
  xa.mu_w = ih->mu_w; xa.rho_w = ih->rho_w;
  xa.sample_dev = (const uint32_t*)ih->sample_idx_dev; xa.sample = ih->sample_idx; xa.layer = ih->layer_id;
  xa.K = I; xa.Kr = Ir; xa.kblocks = (int)iblocks;
  xa.out = dx; xa.out2 = nullptr;

  LstmWArgs wi = {};
  wi.k0 = k0; wi.k1 = k1; wi.B = B; wi.H = H; wi.T = T; wi.dG = dG;
  LstmWArgs wh = wi;
  wi.rho_w = ih->rho_w; wi.rho_b = ih->rho_b;
  wi.sample_dev = (const uint32_t*)ih->sample_idx_dev; wi.sample = ih->sample_idx; wi.layer = ih->layer_id;
  wi.K = I; wi.Kr = Ir; wi.hh = 0; wi.in = x;
  if (g_ih) { wi.dmu_w = g_ih->dmu_w; wi.drho_w = g_ih->drho_w; wi.dmu_b = g_ih->dmu_b; wi.drho_b = g_ih->drho_b; }
  wh.rho_w = hh->rho_w; wh.rho_b = hh->rho_b;
  wh.sample_dev = (const uint32_t*)hh->sample_idx_dev; wh.sample = hh->sample_idx; wh.layer = hh->layer_id;
  wh.K = H; wh.Kr = Hr; wh.hh = 1; wh.in = hidden_seq; wh.h0 = h0;
  if (g_hh) { wh.dmu_w = g_hh->dmu_w; wh.drho_w = g_hh->drho_w; wh.dmu_b = g_hh->dmu_b; wh.drho_b = g_hh->drho_b; }

  hipStream_t st = (hipStream_t)stream;
  const bool wh0 = dh0 || dc0, wx = dx != nullptr, wgi = g_ih != nullptr, wgh = g_hh != nullptr;
  const int bb = (int)bblocks;
  hipError_t e;
  const bool bf = prec == BTX_PREC_BF16, xb = act_dtype == BTX_ACT_BF16;
  if (kind == BTX_KIND_FLIPOUT) {
    if (bf) e = xb ? launch_bwd<1, 1, __bf16>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st) : launch_bwd<1, 1, float>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st);
    else    e = xb ? launch_bwd<1, 0, __bf16>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st) : launch_bwd<1, 0, float>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st);
  } else {
    if (bf) e = xb ? launch_bwd<0, 1, __bf16>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st) : launch_bwd<0, 1, float>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st);
    else    e = xb ? launch_bwd<0, 0, __bf16>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st) : launch_bwd<0, 0, float>(sa, xa, wi, wh, wh0, wx, wgi, wgh, bb, st);
  }
  return (int)e;
}

}  // extern "C"
