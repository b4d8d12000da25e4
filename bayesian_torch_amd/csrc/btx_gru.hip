// btx_gru.hip — fused Bayesian GRU forward (GRUReparameterization / GRUFlipout) for gfx950: inference (btx_gru_fwd)
// and the training forward (btx_gru_fwd_train, §29: the same launches, the step's epilogue also saves what btx_gru_bwd needs).
//
// One sequence = 1 + T launches on the caller's stream, enqueued from C++ (btx_gru_fwd), so it can be captured whole:
//
//   * the input projection for ALL (lane, step) pairs in one launch:
//       Gi[l][t][b][n] = x_t . W_ih(s_l + t)^T + b_ih(s_l + t)          (f32 workspace; does not depend on h)
//   * one recurrent step launch per time step t, gh = h_{t-1} . W_hh(s_l + t)^T + b_hh(s_l + t):
//       r = s(Gi_r + gh_r);  z = s(Gi_z + gh_z);  n = tanh(Gi_n + r * gh_n);  h_t = (1 - z) n + z h_{t-1}
//     written straight into hidden_seq[:, t].  There is no cell state: h_{t-1} is read back from hidden_seq[:, t-1] (or h0).
//
// The reset gate multiplies the RECURRENT half of the candidate only, so — unlike an LSTM step — the projection and the
// recurrent sum of the n rows cannot meet before the nonlinearity: the three recurrent sums of a unit stay in registers, apart
// from Gi, until r is formed.  A workgroup therefore owns GJ hidden units j0..j0+GJ with ALL THREE gate rows {j, H+j, 2H+j} of
// each (GR = 3*GJ rows) and GB batch rows (one per lane of a wave): the thread that finishes (unit, batch row) holds r, z and
// the n row's sum together and needs no second pass.  Per K chunk the workgroup samples its GR rows of W from (mu, rho) in
// registers (Philox + Box-Muller + softplus, BTX-RNG v1) and writes them to LDS only: the sampled weight never exists in HBM.
// GR * GKC / 4 = 192 four-element Philox groups per chunk: waves 0..2 sample one each, wave 3 samples nothing and is first
// through the activation staging.  The 4 waves split the chunk's K and meet in an LDS reduction (fixed order: wave 0..3).
// Flipout keeps a second accumulator set for (h o s_in) . Delta^T and applies s_out per (b, n) before the gate math, on both
// halves (the projection launch applies it to Gi, the step launch to gh).
//
// Noise indices are those of the eager loop (a LinearFlipout / LinearReparameterization forward with sample index s + t):
// eps_w element n*Kr + k, Kr = K rounded up to 8 when K % 8 != 0 (the Linear layers' channel padding); eps_b element n;
// s_in element b*Kr + k of the lane's own [B][Kr] input; s_out element b*3H + n.  Every lane runs the same code on its own
// indices, so a lane is bit for bit a single-sample launch with that lane's index.
//
// Precision: f32 = f32 products, f32 accumulation; bf16 = operands (x / h, and the sampled w resp. mu / delta) rounded to bf16
// once, exact products, f32 accumulation.  The epilogue reads h_{t-1}[b][j] itself (unrounded) for the z h_{t-1} term.  No MFMA:
// a step is sampling- and latency-bound.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/btx_gru.h"
#include "../../include/btx_gru_train.h"
#include "btx_rng.h"

namespace {

constexpr int GJ = 4;            // hidden units per workgroup: one per wave in the epilogue
constexpr int GR = 3 * GJ;       // gate rows per workgroup (r, z, n of each unit)
constexpr int GB = 64;           // batch rows per workgroup: lane b of every wave
constexpr int GW = 4;            // waves; wave w owns k in [w*GKW, (w+1)*GKW) of each chunk
constexpr int GKC = 64;          // K per LDS chunk
constexpr int GKW = GKC / GW;    // K per wave per chunk
constexpr int GXS = GKC + 4;     // padded activation row (floats): lane b reads 16 bytes at b*GXS — conflict-free ds_read_b128
constexpr int GSAMP = GR * GKC / 4;  // sampler threads: one Philox group (4 consecutive k of one row) each
static_assert(GSAMP <= 256 && GW * GR * GB <= GB * GXS, "the reduction reuses the activation image");

struct GruKArgs {
  const void* x;                 // projection: X [rows][T][I]
  const float* mu_w;             // [3H][K]
  const float* rho_w;
  const float* mu_b;             // [3H] or null
  const float* rho_b;
  const uint32_t* sample_dev;    // per-lane words, or null: sample + lane
  uint32_t sample, layer, k0, k1;
  int B, K, Kr, H, T, t, hblocks;
  long long x_lane;              // elements between the lanes' inputs (0: one input shared by all lanes)
  float* G;                      // [lanes][T][B][3H]
  const void* h0;                // [lanes*B][H] or null
  void* hs;                      // [lanes*B][T][H]
  const float* kl_i;             // projection launch, block 0: kl_out = sum over T of (kl_i + kl_h), eager order
  const float* kl_h;
  float* kl_out;
  float* sv;                     // training step (SAVE): [T][B][4H] f32 planes r_t, z_t, n_t, gh_n,t
};

template <typename T> __device__ __forceinline__ float ld_f(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st_f(T* p, float v) { *p = (T)v; }
__device__ __forceinline__ float rbf(float v) { return (float)(__bf16)v; }

__device__ __forceinline__ bool sign_neg(uint32_t idx, uint32_t ka, uint32_t kb) {
  return (btx_sign_word(idx >> 5, ka, kb) >> btx_sign_bitpos(idx & 31u)) & 1u;
}

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

// STEP = 0: input projection (grid.x = hblocks * lanes * T, grid.y = batch blocks); 1: recurrent step t (grid.z = lanes)
// SAVE (step launches of btx_gru_fwd_train, one lane): the epilogue also keeps the gates and the n row's recurrent sum
template <int FLIP, int BFP, typename XT, int STEP, int SAVE = 0>
__global__ __launch_bounds__(256) void gru_kernel(GruKArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[GB * GXS];
  __shared__ __attribute__((aligned(16))) float xd[FLIP ? GB * GXS : 4];
  __shared__ __attribute__((aligned(16))) float ws[GR * GKC];
  __shared__ __attribute__((aligned(16))) float wd[FLIP ? GR * GKC : 4];

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
  const int j0 = hb * GJ, b0 = blockIdx.y * GB;
  const int B = a.B, K = a.K, Kr = a.Kr, H = a.H, N3 = 3 * H;
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

  float acc[GR], accd[GR];
#pragma unroll
  for (int r = 0; r < GR; ++r) { acc[r] = 0.f; accd[r] = 0.f; }

  // sampler role (waves 0..2): LDS row sr = gate * GJ + unit, k group sq of the chunk
  const bool sampler = tid < GSAMP;
  const int sr = tid >> 4, sq = (tid & 15) * 4;
  const int sj = j0 + sr % GJ;
  const int sn = (sr / GJ) * H + sj;
  const bool srow = sampler && sj < H;

  // register double buffer: the global loads of chunk kc + GKC are in flight while chunk kc is contracted
  constexpr int XPT = GB * GKC / 256;  // activations per thread per chunk
  float xr[XPT], mr[4], rr[4];
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < XPT; ++e) {
      const int idx = tid + e * 256, b = idx / GKC, kk = idx - b * GKC, gb = b0 + b, k = kc + kk;
      xr[e] = (src && gb < B && k < K) ? ld_f(src + gb * src_row + k) : 0.f;
    }
    const int k = kc + sq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = srow && k + i < K;
      mr[i] = ok ? a.mu_w[(long long)sn * K + k + i] : 0.f;
      rr[i] = ok ? a.rho_w[(long long)sn * K + k + i] : 0.f;
    }
  };
  load(0);
  for (int kc = 0; kc < K; kc += GKC) {
    // ---- stage the activations (zero outside [B) x [K))
#pragma unroll
    for (int e = 0; e < XPT; ++e) {
      const int idx = tid + e * 256, b = idx / GKC, kk = idx - b * GKC, gb = b0 + b, k = kc + kk;
      const float v = BFP ? rbf(xr[e]) : xr[e];
      xs[b * GXS + kk] = v;
      if (FLIP) xd[b * GXS + kk] = (gb < B && k < K && sign_neg((uint32_t)gb * (uint32_t)Kr + (uint32_t)k, ka, kb)) ? -v : v;
    }
    // ---- sample GR rows x GKC of W in registers, to LDS only
    if (sampler) {
      float wv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
      const int k = kc + sq;
      if (srow && k < K) {
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
        ws[sr * GKC + sq + i] = BFP ? rbf(wv[i]) : wv[i];
        if (FLIP) wd[sr * GKC + sq + i] = BFP ? rbf(dv[i]) : dv[i];
      }
    }
    __syncthreads();
    if (kc + GKC < K) load(kc + GKC);
    // ---- contract: wave w, lane b over its K slice; the weight reads are wave-wide broadcasts
#pragma unroll
    for (int k4 = 0; k4 < GKW; k4 += 4) {
      const int kk = wave * GKW + k4;
      const float4 xv = *(const float4*)&xs[lane_b * GXS + kk];
      float4 xdv;
      if (FLIP) xdv = *(const float4*)&xd[lane_b * GXS + kk];
#pragma unroll
      for (int r = 0; r < GR; ++r) {
        const float4 w = *(const float4*)&ws[r * GKC + kk];
        acc[r] = fmaf(xv.x, w.x, acc[r]); acc[r] = fmaf(xv.y, w.y, acc[r]);
        acc[r] = fmaf(xv.z, w.z, acc[r]); acc[r] = fmaf(xv.w, w.w, acc[r]);
        if (FLIP) {
          const float4 d = *(const float4*)&wd[r * GKC + kk];
          accd[r] = fmaf(xdv.x, d.x, accd[r]); accd[r] = fmaf(xdv.y, d.y, accd[r]);
          accd[r] = fmaf(xdv.z, d.z, accd[r]); accd[r] = fmaf(xdv.w, d.w, accd[r]);
        }
      }
    }
    __syncthreads();
  }

  // ---- LDS reduction over the waves (reuses the activation images)
  float* red = xs;
  float* redd = xd;
#pragma unroll
  for (int r = 0; r < GR; ++r) {
    red[(wave * GR + r) * GB + lane_b] = acc[r];
    if (FLIP) redd[(wave * GR + r) * GB + lane_b] = accd[r];
  }
  // kl: one thread of the projection launch folds the per-step KL terms in the eager order ((kl + kl_i) + kl_h per step)
  if (!STEP && a.kl_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    const float ki = *a.kl_i, kh = *a.kl_h;
    float k = 0.f;
    for (int i = 0; i < a.T; ++i) { k = k + ki; k = k + kh; }
    *a.kl_out = k;
  }
  __syncthreads();

  // ---- epilogue: wave jj finishes unit j0 + jj for the 64 batch rows; the three sums of the unit meet in one thread
  const int jj = wave, j = j0 + jj, gb = b0 + lane_b;
  if (j >= H || gb >= B) return;
  uint32_t koa = 0, kob = 0;
  if (FLIP) {
    const BtxPhilox4 k = btx_philox4x32_10(0u, s, a.layer, BTX_STREAM_SIGN_OUT, a.k0, a.k1);
    koa = k.x[0]; kob = k.x[1];
  }
  float gh[3], gi[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int r = q * GJ + jj, n = q * H + j;
    float v = 0.f, vd = 0.f;
#pragma unroll
    for (int w = 0; w < GW; ++w) {
      v += red[(w * GR + r) * GB + lane_b];
      if (FLIP) vd += redd[(w * GR + r) * GB + lane_b];
    }
    if (a.mu_b) {
      const float eb = btx_normal1((unsigned long long)n, s, a.layer, BTX_STREAM_EPS_B, a.k0, a.k1);
      const float db = btx_softplus_fast(a.rho_b[n]) * eb;
      if (FLIP) { v += a.mu_b[n]; vd += db; }
      else v += a.mu_b[n] + db;
    }
    if (FLIP) v += sign_neg((uint32_t)gb * (uint32_t)N3 + (uint32_t)n, koa, kob) ? -vd : vd;
    float* gp = a.G + (((long long)lane * a.T + t) * B + gb) * N3 + n;
    if (STEP) { gi[q] = *gp; gh[q] = v; }
    else *gp = v;
  }
  if (!STEP) return;
  const float h_prev = src ? ld_f(src + gb * src_row + j) : 0.f;
  const float r_t = sigm(gi[0] + gh[0]);
  const float z_t = sigm(gi[1] + gh[1]);
  const float n_t = tanhf(gi[2] + r_t * gh[2]);
  const float h = (1.0f - z_t) * n_t + z_t * h_prev;
  st_f((XT*)a.hs + (((long long)lane * B + gb) * a.T + t) * H + j, h);
  if (SAVE) {  // what btx_gru_bwd needs: with these it evaluates no transcendental and never re-reads Gi
    float* sp = a.sv + ((long long)t * B + gb) * 4 * H + j;
    sp[0] = r_t; sp[H] = z_t; sp[2 * H] = n_t; sp[3 * H] = gh[2];
  }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

template <int FLIP, int BFP, typename XT, int SAVE = 0>
hipError_t launch_all(GruKArgs pa, GruKArgs sa, int lanes, int bblocks, int T, hipStream_t st) {
  hipLaunchKernelGGL((gru_kernel<FLIP, BFP, XT, 0>), dim3(pa.hblocks * lanes * T, bblocks, 1), dim3(256), 0, st, pa);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int t = 0; t < T; ++t) {
    sa.t = t;
    hipLaunchKernelGGL((gru_kernel<FLIP, BFP, XT, 1, SAVE>), dim3(sa.hblocks, bblocks, lanes), dim3(256), 0, st, sa);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// saved != null: the training forward (one lane), whose step launches are the SAVE form
int gru_fwd_impl(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                 const void* h0, void* hidden_seq, const float* kl_ih, const float* kl_hh, float* kl_out, int lanes, int B,
                 int I, int H, int T, int act_dtype, int prec, void* workspace, size_t ws_bytes, void* saved,
                 size_t saved_bytes, void* stream) {
  if (!ih || !hh || !x || !hidden_seq || !workspace) return BTX_E_NULL;
  if (!ih->mu_w || !ih->rho_w || !hh->mu_w || !hh->rho_w) return BTX_E_NULL;
  if ((ih->mu_b == nullptr) != (ih->rho_b == nullptr) || (hh->mu_b == nullptr) != (hh->rho_b == nullptr)) return BTX_E_NULL;
  if (kl_out && (!kl_ih || !kl_hh)) return BTX_E_NULL;
  if (kind != BTX_KIND_REPARAM && kind != BTX_KIND_FLIPOUT) return BTX_E_UNSUPPORTED;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // the fused sequence has f32 and bf16 forms only
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16) return BTX_E_DTYPE;
  if (lanes <= 0 || lanes > 255 || B <= 0 || I <= 0 || H <= 0 || T <= 0) return BTX_E_SHAPE;
  const int Ir = I % 8 ? (I + 7) / 8 * 8 : I, Hr = H % 8 ? (H + 7) / 8 * 8 : H;
  // BTX-RNG v1 counters are 32 bits: every noise index of one layer must fit
  if ((uint64_t)3 * H * Ir > 0xfffffff0ull || (uint64_t)3 * H * Hr > 0xfffffff0ull || (uint64_t)B * 3 * H > 0xfffffff0ull ||
      (uint64_t)B * Ir > 0xfffffff0ull || (uint64_t)B * Hr > 0xfffffff0ull)
    return BTX_E_UNSUPPORTED;
  const uint64_t hblocks = ((uint64_t)H + GJ - 1) / GJ, bblocks = ((uint64_t)B + GB - 1) / GB;
  if (hblocks * lanes * T > 0x7fffffffull || bblocks > 65535) return BTX_E_UNSUPPORTED;
  if (ws_bytes < (saved ? btx_gru_train_workspace_bytes(B, H, T) : btx_gru_workspace_bytes(lanes, B, H, T))) return BTX_E_WORKSPACE;
  if (saved && saved_bytes < btx_gru_train_saved_bytes(B, H, T)) return BTX_E_WORKSPACE;

  GruKArgs pa = {};
  pa.x = x;
  pa.mu_w = ih->mu_w; pa.rho_w = ih->rho_w; pa.mu_b = ih->mu_b; pa.rho_b = ih->rho_b;
  pa.sample_dev = (const uint32_t*)ih->sample_idx_dev; pa.sample = ih->sample_idx; pa.layer = ih->layer_id;
  pa.k0 = (uint32_t)seed; pa.k1 = (uint32_t)(seed >> 32);
  pa.B = B; pa.K = I; pa.Kr = Ir; pa.H = H; pa.T = T; pa.hblocks = (int)hblocks;
  pa.x_lane = x_shared ? 0 : (long long)B * T * I;
  pa.G = (float*)workspace;
  pa.kl_i = kl_ih; pa.kl_h = kl_hh; pa.kl_out = kl_out;
  GruKArgs sa = pa;
  sa.x = nullptr; sa.x_lane = 0; sa.kl_out = nullptr;
  sa.mu_w = hh->mu_w; sa.rho_w = hh->rho_w; sa.mu_b = hh->mu_b; sa.rho_b = hh->rho_b;
  sa.sample_dev = (const uint32_t*)hh->sample_idx_dev; sa.sample = hh->sample_idx; sa.layer = hh->layer_id;
  sa.K = H; sa.Kr = Hr;
  sa.h0 = h0; sa.hs = hidden_seq; sa.sv = (float*)saved;

  hipStream_t st = (hipStream_t)stream;
  const int bb = (int)bblocks;
  hipError_t e;
  const bool bf = prec == BTX_PREC_BF16, xb = act_dtype == BTX_ACT_BF16;
  if (saved) {
    if (kind == BTX_KIND_FLIPOUT) {
      if (bf) e = xb ? launch_all<1, 1, __bf16, 1>(pa, sa, 1, bb, T, st) : launch_all<1, 1, float, 1>(pa, sa, 1, bb, T, st);
      else    e = xb ? launch_all<1, 0, __bf16, 1>(pa, sa, 1, bb, T, st) : launch_all<1, 0, float, 1>(pa, sa, 1, bb, T, st);
    } else {
      if (bf) e = xb ? launch_all<0, 1, __bf16, 1>(pa, sa, 1, bb, T, st) : launch_all<0, 1, float, 1>(pa, sa, 1, bb, T, st);
      else    e = xb ? launch_all<0, 0, __bf16, 1>(pa, sa, 1, bb, T, st) : launch_all<0, 0, float, 1>(pa, sa, 1, bb, T, st);
    }
  } else if (kind == BTX_KIND_FLIPOUT) {
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

size_t btx_gru_workspace_bytes(int lanes, int B, int H, int T) {
  if (lanes <= 0 || B <= 0 || H <= 0 || T <= 0) return 0;
  return align256((size_t)lanes * T * B * 3 * H * sizeof(float));
}

size_t btx_gru_train_saved_bytes(int B, int H, int T) {
  if (B <= 0 || H <= 0 || T <= 0) return 0;
  return align256((size_t)T * B * 4 * H * sizeof(float));
}

size_t btx_gru_train_workspace_bytes(int B, int H, int T) {
  // the backward's dG [T][B][4H] + the f32 z-carry [B][H]; the forward's projection Gi [T][B][3H] fits in the first part
  if (B <= 0 || H <= 0 || T <= 0) return 0;
  return align256((size_t)T * B * 4 * H * sizeof(float)) + align256((size_t)B * H * sizeof(float));
}

int btx_gru_fwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                const void* h0, void* hidden_seq, const float* kl_ih, const float* kl_hh, float* kl_out, int lanes, int B,
                int I, int H, int T, int act_dtype, int prec, void* workspace, size_t ws_bytes, void* stream) {
  return gru_fwd_impl(kind, ih, hh, seed, x, x_shared, h0, hidden_seq, kl_ih, kl_hh, kl_out, lanes, B, I, H, T, act_dtype, prec,
                      workspace, ws_bytes, nullptr, 0, stream);
}

int btx_gru_fwd_train(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, const void* h0,
                      void* hidden_seq, const float* kl_ih, const float* kl_hh, float* kl_out, int B, int I, int H, int T,
                      int act_dtype, int prec, void* workspace, size_t ws_bytes, void* saved, size_t saved_bytes, void* stream) {
  if (!saved) return BTX_E_NULL;
  return gru_fwd_impl(kind, ih, hh, seed, x, 0, h0, hidden_seq, kl_ih, kl_hh, kl_out, 1, B, I, H, T, act_dtype, prec, workspace,
                      ws_bytes, saved, saved_bytes, stream);
}

}  // extern "C"
