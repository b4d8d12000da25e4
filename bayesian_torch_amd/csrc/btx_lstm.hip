// btx_lstm.hip — fused Bayesian LSTM inference (LSTMReparameterization / LSTMFlipout) for gfx950.
//
// One sequence = 1 + T launches on the caller's stream, enqueued from C++ (btx_lstm_fwd), so it can be captured whole:
//
//   * the input projection for ALL (lane, step) pairs in one launch:
//       G[l][t][b][n] = x_t . W_ih(s_l + t)^T + b_ih(s_l + t)          (f32 workspace; does not depend on h)
//   * one recurrent step launch per time step t:
//       gates = G[l][t] + h_{t-1} . W_hh(s_l + t)^T + b_hh(s_l + t);  c = s(f) c + s(i) tanh(g);  h = s(o) tanh(c)
//     written straight into hidden_seq[:, t] / c_seq[:, t]; c is carried in an f32 workspace row.
//
// Both are the same kernel body.  A workgroup owns LJ hidden units j0..j0+LJ and the four gate rows {j, H+j, 2H+j, 3H+j} of
// each (LR = 4*LJ rows), and LB batch rows (one per lane of a wave).  Per K chunk it samples its LR rows of W from (mu, rho)
// in registers (Philox + Box-Muller + softplus, BTX-RNG v1) and writes them to LDS only: the sampled weight never exists in
// HBM.  The 4 waves split the chunk's K and meet in an LDS reduction (fixed order); the gate / cell epilogue runs on the
// reduced sums in registers.  Flipout keeps a second accumulator set for (x o s_in) . Delta^T and applies s_out per (b, n).
//
// Noise indices are those of the eager path (a LinearFlipout / LinearReparameterization forward with sample index s + t):
// eps_w element n*Kr + k, Kr = K rounded up to 8 when K % 8 != 0 (the Linear layers' channel padding); eps_b element n;
// s_in element b*Kr + k of the lane's own [B][Kr] input; s_out element b*4H + n.  Every lane runs the same code on its
// own indices, so a lane is bit for bit a single-sample launch with that lane's index.
//
// Precision: f32 = f32 products, f32 accumulation; bf16 = operands (x, and the sampled w resp. mu / delta) rounded to bf16,
// exact products, f32 accumulation (what v_mfma_f32_32x32x16_bf16 computes).  No MFMA: at these shapes a step is
// sampling- and latency-bound.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/btx.h"
#include "btx_rng.h"

namespace {

constexpr int LJ = 4;            // hidden units per workgroup
constexpr int LR = 4 * LJ;       // gate rows per workgroup
constexpr int LB = 64;           // batch rows per workgroup: lane b of every wave
constexpr int LW = 4;            // waves; wave w owns k in [w*LKW, (w+1)*LKW) of each chunk
constexpr int LKC = 64;          // K per LDS chunk
constexpr int LKW = LKC / LW;    // K per wave per chunk
constexpr int LXS = LKC + 4;     // padded activation row (floats): conflict-free ds_read_b128 across b

struct LstmKArgs {
  const void* x;                 // projection: X [rows][T][I]
  const float* mu_w;             // [4H][K]
  const float* rho_w;
  const float* mu_b;             // [4H] or null
  const float* rho_b;
  const uint32_t* sample_dev;    // per-lane words, or null: sample + lane
  uint32_t sample, layer, k0, k1;
  int B, K, Kr, H, T, t, hblocks;
  long long x_lane;              // elements between the lanes' inputs (0: one input shared by all lanes)
  float* G;                      // [lanes][T][B][4H]
  const void* h0;                // [lanes*B][H] or null
  const void* c0;
  void* hs;                      // [lanes*B][T][H]
  void* cs;
  float* cst;                    // [lanes][B][H] f32 cell state
  const float* kl_i;             // projection launch, block 0: kl_out = sum over T of (kl_i + kl_h), eager order
  const float* kl_h;
  float* kl_out;
  float* sv_g;                   // training forward (STEP = 2): gate pre-activations [T][B][4H] f32
  float* sv_c;                   //   and the f32 cell state [T][B][H]
};

template <typename T> __device__ __forceinline__ float ld_f(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st_f(T* p, float v) { *p = (T)v; }
__device__ __forceinline__ float rbf(float v) { return (float)(__bf16)v; }

__device__ __forceinline__ bool sign_neg(uint32_t idx, uint32_t ka, uint32_t kb) {
  return (btx_sign_word(idx >> 5, ka, kb) >> btx_sign_bitpos(idx & 31u)) & 1u;
}

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

// STEP = 0: input projection (grid.x = hblocks * lanes * T, grid.y = batch blocks); 1: recurrent step t (grid.z = lanes);
// 2: the step of a training forward (one lane) — step 1 plus stores of the gate pre-activations and c_t for btx_lstm_bwd
template <int FLIP, int BFP, typename XT, int STEP>
__global__ __launch_bounds__(256) void lstm_kernel(LstmKArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[LB * LXS];
  __shared__ __attribute__((aligned(16))) float xd[FLIP ? LB * LXS : 4];
  __shared__ __attribute__((aligned(16))) float ws[LR * LKC];
  __shared__ __attribute__((aligned(16))) float wd[FLIP ? LR * LKC : 4];

  const int tid = threadIdx.x, lane_b = tid & 63, wave = tid >> 6;
  int hb, lane, t;
  if (STEP) {
    hb = blockIdx.x; lane = blockIdx.z; t = a.t;
  } else {
    const int pair = blockIdx.x / a.hblocks;
    hb = blockIdx.x - pair * a.hblocks;
    lane = pair / a.T;
    t = pair - lane * a.T;
  }
  const int j0 = hb * LJ, b0 = blockIdx.y * LB;
  const int B = a.B, K = a.K, Kr = a.Kr, H = a.H, N4 = 4 * H;
  uint32_t s = a.sample_dev ? __builtin_amdgcn_readfirstlane(a.sample_dev[lane]) : a.sample + (uint32_t)lane;
  s += (uint32_t)t;

  // projection: X row (b, t) of this lane; step: h_{t-1} (previous step's output slice, or h0, or zeros)
  const XT* src = nullptr;
  long long src_row = 0;
  if (STEP) {
    if (t > 0) { src = (const XT*)a.hs + (long long)lane * B * a.T * H + (long long)(t - 1) * H; src_row = (long long)a.T * H; }
    else if (a.h0) { src = (const XT*)a.h0 + (long long)lane * B * H; src_row = H; }
  } else {
    src = (const XT*)a.x + (long long)lane * a.x_lane + (long long)t * K;
    src_row = (long long)a.T * K;
  }
  uint32_t ka = 0, kb = 0;
  if (FLIP) {
    const BtxPhilox4 k = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_IN, a.k0, a.k1);
    ka = k.x[0]; kb = k.x[1];
  }

  float acc[LR], accd[LR];
#pragma unroll
  for (int r = 0; r < LR; ++r) { acc[r] = 0.f; accd[r] = 0.f; }

  // sampler role of this thread: row sr, k group sq*4 of the chunk (LR * LKC / 4 == 256 groups)
  const int sr = tid >> 4, sq = (tid & 15) * 4;
  const int sj = j0 + (sr & (LJ - 1));
  const int sn = (sr / LJ) * H + sj;

  // register double buffer: the global loads of chunk kc + LKC are in flight while chunk kc is contracted (a step is a
  // handful of chunks, each otherwise one full memory round trip)
  constexpr int XPT = LB * LKC / 256;  // activations per thread per chunk
  float xr[XPT], mr[4], rr[4];
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < XPT; ++e) {
      const int idx = tid + e * 256, b = idx / LKC, kk = idx - b * LKC, gb = b0 + b, k = kc + kk;
      xr[e] = (src && gb < B && k < K) ? ld_f(src + gb * src_row + k) : 0.f;
    }
    const int k = kc + sq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = sj < H && k + i < K;
      mr[i] = ok ? a.mu_w[(long long)sn * K + k + i] : 0.f;
      rr[i] = ok ? a.rho_w[(long long)sn * K + k + i] : 0.f;
    }
  };
  load(0);
  for (int kc = 0; kc < K; kc += LKC) {
    // ---- stage the activations (zero outside [B) x [K))
#pragma unroll
    for (int e = 0; e < XPT; ++e) {
      const int idx = tid + e * 256, b = idx / LKC, kk = idx - b * LKC, gb = b0 + b, k = kc + kk;
      const float v = BFP ? rbf(xr[e]) : xr[e];
      xs[b * LXS + kk] = v;
      if (FLIP) xd[b * LXS + kk] = (gb < B && k < K && sign_neg((uint32_t)gb * (uint32_t)Kr + (uint32_t)k, ka, kb)) ? -v : v;
    }
    // ---- sample LR rows x LKC of W in registers, to LDS only
    {
      float wv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
      const int k = kc + sq;
      if (sj < H && k < K) {
        float z[4];
        btx_normal4_hw(((uint32_t)sn * (uint32_t)Kr + (uint32_t)k) >> 2, s, a.layer, BTX_STREAM_EPS_W, a.k0, a.k1, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (k + i < K) {
            const float mu = mr[i], d = btx_softplus_hw(rr[i]) * z[i];
            if (FLIP) { wv[i] = mu; dv[i] = d; }
            else wv[i] = mu + d;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ws[sr * LKC + sq + i] = BFP ? rbf(wv[i]) : wv[i];
        if (FLIP) wd[sr * LKC + sq + i] = BFP ? rbf(dv[i]) : dv[i];
      }
    }
    __syncthreads();
    if (kc + LKC < K) load(kc + LKC);
    // ---- contract: wave w, lane b over its K slice
#pragma unroll
    for (int k4 = 0; k4 < LKW; k4 += 4) {
      const int kk = wave * LKW + k4;
      const float4 xv = *(const float4*)&xs[lane_b * LXS + kk];
      float4 xdv;
      if (FLIP) xdv = *(const float4*)&xd[lane_b * LXS + kk];
#pragma unroll
      for (int r = 0; r < LR; ++r) {
        const float4 w = *(const float4*)&ws[r * LKC + kk];
        acc[r] = fmaf(xv.x, w.x, acc[r]); acc[r] = fmaf(xv.y, w.y, acc[r]);
        acc[r] = fmaf(xv.z, w.z, acc[r]); acc[r] = fmaf(xv.w, w.w, acc[r]);
        if (FLIP) {
          const float4 d = *(const float4*)&wd[r * LKC + kk];
          accd[r] = fmaf(xdv.x, d.x, accd[r]); accd[r] = fmaf(xdv.y, d.y, accd[r]);
          accd[r] = fmaf(xdv.z, d.z, accd[r]); accd[r] = fmaf(xdv.w, d.w, accd[r]);
        }
      }
    }
    __syncthreads();
  }

  // ---- LDS reduction over the waves (reuses the activation images: LW * LR * LB <= LB * LXS)
  float* red = xs;
  float* redd = xd;
#pragma unroll
  for (int r = 0; r < LR; ++r) {
    red[(wave * LR + r) * LB + lane_b] = acc[r];
    if (FLIP) redd[(wave * LR + r) * LB + lane_b] = accd[r];
  }
  // kl: one thread of the projection launch folds the per-step KL terms in the eager order ((kl + kl_i) + kl_h per step)
  if (!STEP && a.kl_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    const float ki = *a.kl_i, kh = *a.kl_h;
    float k = 0.f;
    for (int i = 0; i < a.T; ++i) { k = k + ki; k = k + kh; }
    *a.kl_out = k;
  }
  __syncthreads();

  const int jj = tid >> 6, j = j0 + jj, gb = b0 + lane_b;
  if (j >= H || gb >= B) return;
  uint32_t koa = 0, kob = 0;
  if (FLIP) {
    const BtxPhilox4 k = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_OUT, a.k0, a.k1);
    koa = k.x[0]; kob = k.x[1];
  }
  float g[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = q * LJ + jj, n = q * H + j;
    float v = 0.f, vd = 0.f;
#pragma unroll
    for (int w = 0; w < LW; ++w) {
      v += red[(w * LR + r) * LB + lane_b];
      if (FLIP) vd += redd[(w * LR + r) * LB + lane_b];
    }
    if (a.mu_b) {
      const float eb = btx_normal1((unsigned long long)n, s, a.layer, BTX_STREAM_EPS_B, a.k0, a.k1);
      const float db = btx_softplus_fast(a.rho_b[n]) * eb;
      if (FLIP) { v += a.mu_b[n]; vd += db; }
      else v += a.mu_b[n] + db;
    }
    if (FLIP) v += sign_neg((uint32_t)gb * (uint32_t)N4 + (uint32_t)n, koa, kob) ? -vd : vd;
    float* gp = a.G + (((long long)lane * a.T + t) * B + gb) * N4 + n;
    if (STEP) g[q] = *gp + v;
    else *gp = v;
  }
  if (!STEP) return;
  const long long hrow = (long long)lane * B + gb;
  float c_prev;
  if (t > 0) c_prev = a.cst[hrow * H + j];
  else c_prev = a.c0 ? ld_f((const XT*)a.c0 + hrow * H + j) : 0.f;
  const float i_t = sigm(g[0]), f_t = sigm(g[1]), g_t = tanhf(g[2]), o_t = sigm(g[3]);
  const float c = f_t * c_prev + i_t * g_t;
  const float h = o_t * tanhf(c);
  if (STEP == 2) {
    float* sg = a.sv_g + ((long long)t * B + gb) * N4 + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) sg[q * H] = g[q];
    a.sv_c[((long long)t * B + gb) * H + j] = c;
  }
  a.cst[hrow * H + j] = c;
  st_f((XT*)a.hs + (hrow * a.T + t) * H + j, h);
  st_f((XT*)a.cs + (hrow * a.T + t) * H + j, c);
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

template <int FLIP, int BFP, typename XT, int STEP = 1>
hipError_t launch_all(LstmKArgs pa, LstmKArgs sa, int lanes, int bblocks, int T, hipStream_t st) {
  hipLaunchKernelGGL((lstm_kernel<FLIP, BFP, XT, 0>), dim3(pa.hblocks * lanes * T, bblocks, 1), dim3(256), 0, st, pa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int t = 0; t < T; ++t) {
    sa.t = t;
    hipLaunchKernelGGL((lstm_kernel<FLIP, BFP, XT, STEP>), dim3(sa.hblocks, bblocks, lanes), dim3(256), 0, st, sa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

int lstm_fwd_impl(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                  const void* h0, const void* c0, void* hidden_seq, void* c_seq, const float* kl_ih, const float* kl_hh,
                  float* kl_out, int lanes, int B, int I, int H, int T, int act_dtype, int prec, void* workspace,
                  size_t ws_bytes, void* saved, size_t saved_bytes, void* stream) {
  if (!ih || !hh || !x || !hidden_seq || !c_seq || !workspace) return BTX_E_NULL;
  if (!ih->mu_w || !ih->rho_w || !hh->mu_w || !hh->rho_w) return BTX_E_NULL;
  if ((ih->mu_b == nullptr) != (ih->rho_b == nullptr) || (hh->mu_b == nullptr) != (hh->rho_b == nullptr)) return BTX_E_NULL;
  if (kl_out && (!kl_ih || !kl_hh)) return BTX_E_NULL;
  if ((h0 == nullptr) != (c0 == nullptr)) return BTX_E_NULL;
  if (kind != BTX_KIND_REPARAM && kind != BTX_KIND_FLIPOUT) return BTX_E_UNSUPPORTED;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // the fused sequence has f32 and bf16 forms only
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16) return BTX_E_DTYPE;
  if (lanes <= 0 || lanes > 255 || B <= 0 || I <= 0 || H <= 0 || T <= 0) return BTX_E_SHAPE;
  const int Ir = I % 8 ? (I + 7) / 8 * 8 : I, Hr = H % 8 ? (H + 7) / 8 * 8 : H;
  // BTX-RNG v1 counters are 32 bits: every noise index of one layer must fit
  if ((uint64_t)4 * H * Ir > 0xfffffff0ull || (uint64_t)4 * H * Hr > 0xfffffff0ull || (uint64_t)B * 4 * H > 0xfffffff0ull ||
      (uint64_t)B * Ir > 0xfffffff0ull)
    return BTX_E_UNSUPPORTED;
  const uint64_t hblocks = ((uint64_t)H + LJ - 1) / LJ, bblocks = ((uint64_t)B + LB - 1) / LB;
  if (hblocks * lanes * T > 0x7fffffffull || bblocks > 65535) return BTX_E_UNSUPPORTED;
  if (ws_bytes < btx_lstm_workspace_bytes(lanes, B, H, T)) return BTX_E_WORKSPACE;
  if (saved && saved_bytes < btx_lstm_train_saved_bytes(B, H, T)) return BTX_E_WORKSPACE;

  LstmKArgs pa = {};
  pa.x = x;
  pa.mu_w = ih->mu_w; pa.rho_w = ih->rho_w; pa.mu_b = ih->mu_b; pa.rho_b = ih->rho_b;
  pa.sample_dev = (const uint32_t*)ih->sample_idx_dev; pa.sample = ih->sample_idx; pa.layer = ih->layer_id;
  pa.k0 = (uint32_t)seed; pa.k1 = (uint32_t)(seed >> 32);
  pa.B = B; pa.K = I; pa.Kr = Ir; pa.H = H; pa.T = T; pa.hblocks = (int)hblocks;
  pa.x_lane = x_shared ? 0 : (long long)B * T * I;
  pa.G = (float*)workspace;
  pa.kl_i = kl_ih; pa.kl_h = kl_hh; pa.kl_out = kl_out;
  LstmKArgs sa = pa;
  sa.x = nullptr; sa.x_lane = 0; sa.kl_out = nullptr;
  sa.mu_w = hh->mu_w; sa.rho_w = hh->rho_w; sa.mu_b = hh->mu_b; sa.rho_b = hh->rho_b;
  sa.sample_dev = (const uint32_t*)hh->sample_idx_dev; sa.sample = hh->sample_idx; sa.layer = hh->layer_id;
  sa.K = H; sa.Kr = Hr;
  sa.h0 = h0; sa.c0 = c0; sa.hs = hidden_seq; sa.cs = c_seq;
  sa.cst = (float*)((char*)workspace + align256((size_t)lanes * T * B * 4 * H * sizeof(float)));
  if (saved) {
    sa.sv_g = (float*)saved;
    sa.sv_c = (float*)((char*)saved + align256((size_t)T * B * 4 * H * sizeof(float)));
  }

  hipStream_t st = (hipStream_t)stream;
  const int bb = (int)bblocks;
  hipError_t e;
  const bool bf = prec == BTX_PREC_BF16, xb = act_dtype == BTX_ACT_BF16;
  if (saved) {  // training forward: one lane, the step form that keeps what btx_lstm_bwd needs
    if (kind == BTX_KIND_FLIPOUT) {
      if (bf) e = xb ? launch_all<1, 1, __bf16, 2>(pa, sa, 1, bb, T, st) : launch_all<1, 1, float, 2>(pa, sa, 1, bb, T, st);
      else    e = xb ? launch_all<1, 0, __bf16, 2>(pa, sa, 1, bb, T, st) : launch_all<1, 0, float, 2>(pa, sa, 1, bb, T, st);
    } else {
      if (bf) e = xb ? launch_all<0, 1, __bf16, 2>(pa, sa, 1, bb, T, st) : launch_all<0, 1, float, 2>(pa, sa, 1, bb, T, st);
      else    e = xb ? launch_all<0, 0, __bf16, 2>(pa, sa, 1, bb, T, st) : launch_all<0, 0, float, 2>(pa, sa, 1, bb, T, st);
    }
    return (int)e;
  }
  if (kind == BTX_KIND_FLIPOUT) {
    if (bf) e = xb ? launch_all<1, 1, __bf16>(pa, sa, lanes, bb, T, st) : launch_all<1, 1, float>(pa, sa, lanes, bb, T, st);
    else    e = xb ? launch_all<1, 0, __bf16>(pa, sa, lanes, bb, T, st) : launch_all<1, 0, float>(pa, sa, lanes, bb, T, st);
  } else {
    if (bf) e = xb ? launch_all<0, 1, __bf16>(pa, sa, lanes, bb, T, st) : launch_all<0, 1, float>(pa, sa, lanes, bb, T, st);
    else    e = xb ? launch_all<0, 0, __bf16>(pa, sa, lanes, bb, T, st) : launch_all<0, 0, float>(pa, sa, lanes, bb, T, st);
  }
  return (int)e;
}

}  // namespace

extern "C" {

size_t btx_lstm_workspace_bytes(int lanes, int B, int H, int T) {
  if (lanes <= 0 || B <= 0 || H <= 0 || T <= 0) return 0;
  return align256((size_t)lanes * T * B * 4 * H * sizeof(float)) + align256((size_t)lanes * B * H * sizeof(float));
}

size_t btx_lstm_train_saved_bytes(int B, int H, int T) {
  if (B <= 0 || H <= 0 || T <= 0) return 0;
  return align256((size_t)T * B * 4 * H * sizeof(float)) + align256((size_t)T * B * H * sizeof(float));
}

size_t btx_lstm_train_workspace_bytes(int B, int H, int T) {
  // the forward's projection G + f32 cell row; the backward's dgates [T][B][4H] + f32 dc carry: the same sizes
  return btx_lstm_workspace_bytes(1, B, H, T);
}

int btx_lstm_fwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                 const void* h0, const void* c0, void* hidden_seq, void* c_seq, const float* kl_ih, const float* kl_hh,
                 float* kl_out, int lanes, int B, int I, int H, int T, int act_dtype, int prec, void* workspace,
                 size_t ws_bytes, void* stream) {
  return lstm_fwd_impl(kind, ih, hh, seed, x, x_shared, h0, c0, hidden_seq, c_seq, kl_ih, kl_hh, kl_out, lanes, B, I, H, T,
                       act_dtype, prec, workspace, ws_bytes, nullptr, 0, stream);
}

int btx_lstm_fwd_train(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x,
                       const void* h0, const void* c0, void* hidden_seq, void* c_seq, const float* kl_ih, const float* kl_hh,
                       float* kl_out, int B, int I, int H, int T, int act_dtype, int prec, void* workspace, size_t ws_bytes,
                       void* saved, size_t saved_bytes, void* stream) {
  if (!saved) return BTX_E_NULL;
  return lstm_fwd_impl(kind, ih, hh, seed, x, 0, h0, c0, hidden_seq, c_seq, kl_ih, kl_hh, kl_out, 1, B, I, H, T, act_dtype,
                       prec, workspace, ws_bytes, saved, saved_bytes, stream);
}

}  // extern "C"
