// btx_lrt.hip — training of the local reparameterization layers (BTX-LRT v1, DESIGN.md §21 "Backward"): btx_lrt_fwd_train and
// btx_lrt_bwd.  gfx950 only.
//
//   forward   the kind-2 launch of btx_contract_fwd_ex (contract_kernel VAR = 1) with one more store: root[i] = r_i =
//             sqrtf(v_i + sigma_b^2), f32, in the layout of `out`
//   backward  with g = dL/dy, zeta the forward's draw (regenerated: stream 4, index of the element in the output tensor):
//               c  = r > 0 ? zeta / (2 r) : 0          gv = act(g * c)        (rounded ONCE, to the activation dtype)
//               dmu = corr(x, g)                       dS = corr(act(x * x), gv)       drho   = dS   * 2 sigma   sigmoid(rho)
//               dmu_b = sum_p g                        dS_b = sum_p gv                 drho_b = dS_b * 2 sigma_b sigmoid(rho_b)
//               dx = act(A + 2 x (.) B),  A = act(op^T(g, mu)),  B = act(op^T(gv, sigma^2))
//             launches: lrt_gv_kernel; btx_bias_grad on g and on gv (fixed order); lrt_square_kernel; btx_contract_wgrad_ws twice
//             (kind 0, slabs); lrt_rho_scale_kernel on dS and dS_b; lrt_dgrad_weights_kernel (mu^T and (sigma^2)^T in one launch);
//             two noise-free contractions (contract_kernel VAR = 2) on the geometry of the data gradient; lrt_combine_kernel.
//             No host read, no allocation, no memset: all scratch is the caller's workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/btx.h"
#include "btx_contract.h"
#include "btx_rng.h"

using namespace btx;

namespace {

struct LrtRng {
  uint32_t k0, k1, sample, layer;
  const uint32_t* sample_ptr;
};

template <typename ACT>
__device__ __forceinline__ void load4(const ACT* p, bool vec, int nv, float* f) {
  if (vec) {
    if constexpr (sizeof(ACT) == 4) {
      const f32x4 v = *(const f32x4*)p;
      f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    } else {
      const u32x2 v = *(const u32x2*)p;
      f[0] = u2f(v[0] << 16); f[1] = u2f(v[0] & 0xffff0000u); f[2] = u2f(v[1] << 16); f[3] = u2f(v[1] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = e < nv ? (float)p[e] : 0.f;
  }
}
template <typename ACT>
__device__ __forceinline__ void store4(ACT* p, bool vec, int nv, const float* f) {
  if (vec) {
    if constexpr (sizeof(ACT) == 4) {
      *(f32x4*)p = (f32x4){f[0], f[1], f[2], f[3]};
    } else {
      const f32x4 fv = {f[0], f[1], f[2], f[3]};
      *(bf16x4*)p = __builtin_convertvector(fv, bf16x4);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < nv) p[e] = (ACT)f[e];
  }
}
template <typename ACT>
__host__ __device__ __forceinline__ bool run_aligned(const void* p) { return (((uintptr_t)p) & (4 * sizeof(ACT) - 1)) == 0; }

// gv[i] = act(g[i] * c_i), c_i = r_i > 0 ? zeta_i / (2 r_i) : 0; one thread per aligned group of four output elements = one Philox
// block of stream 4 (the group btx_fill_eps and the forward's store draw together)
template <typename ACT>
__global__ __launch_bounds__(256) void lrt_gv_kernel(const ACT* __restrict__ dy, const float* __restrict__ root, ACT* __restrict__ gv,
                                                     size_t n, const LrtRng rg) {
  const uint32_t smp = rg.sample_ptr ? __builtin_amdgcn_readfirstlane(*rg.sample_ptr) : rg.sample;
  const size_t nblk = (n + 3) >> 2;
  const bool al_dy = run_aligned<ACT>(dy), al_r = run_aligned<float>(root);  // gv lives in the workspace: always on the grid
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (size_t)gridDim.x * 256) {
    const size_t i = b << 2;
    const int nv = (int)((n - i) < 4 ? (n - i) : 4);
    float g[4], r[4], z[4], o[4];
    load4<ACT>(dy + i, al_dy && nv == 4, nv, g);
    load4<float>(root + i, al_r && nv == 4, nv, r);
    btx_normal4((uint32_t)b, smp, rg.layer, BTX_STREAM_OUT_NOISE, rg.k0, rg.k1, z);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float c = r[e] > 0.f ? z[e] / (2.0f * r[e]) : 0.f;
      o[e] = g[e] * c;
    }
    store4<ACT>(gv + i, nv == 4, nv, o);
  }
}

// x2[i] = act(f32(x[i]) * f32(x[i])): the activation operand of the second weight gradient, rounded once
template <typename ACT>
__global__ __launch_bounds__(256) void lrt_square_kernel(const ACT* __restrict__ x, ACT* __restrict__ x2, size_t n) {
  const size_t nblk = (n + 3) >> 2;
  const bool al = run_aligned<ACT>(x);
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (size_t)gridDim.x * 256) {
    const size_t i = b << 2;
    const int nv = (int)((n - i) < 4 ? (n - i) : 4);
    float f[4];
    load4<ACT>(x + i, al && nv == 4, nv, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = f[e] * f[e];
    store4<ACT>(x2 + i, nv == 4, nv, f);
  }
}

// dx[i] = act(f32(dx[i]) + 2 x[i] * B[i]): dx holds A on entry
template <typename ACT>
__global__ __launch_bounds__(256) void lrt_combine_kernel(ACT* __restrict__ dx, const ACT* __restrict__ x, const ACT* __restrict__ B,
                                                          size_t n) {
  const size_t nblk = (n + 3) >> 2;
  const bool al_x = run_aligned<ACT>(x), al_dx = run_aligned<ACT>(dx);
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < nblk; b += (size_t)gridDim.x * 256) {
    const size_t i = b << 2;
    const int nv = (int)((n - i) < 4 ? (n - i) : 4);
    float a[4], xv[4], bv[4];
    load4<ACT>(dx + i, al_dx && nv == 4, nv, a);
    load4<ACT>(x + i, al_x && nv == 4, nv, xv);
    load4<ACT>(B + i, nv == 4, nv, bv);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = __builtin_fmaf(2.0f * xv[e], bv[e], a[e]);
    store4<ACT>(dx + i, al_dx && nv == 4, nv, a);
  }
}

// d[i] = d[i] * (2 sigma sigmoid(rho[i])), sigma = btx_softplus_fast(rho[i]): dS -> drho in place (weights and bias)
__global__ __launch_bounds__(256) void lrt_rho_scale_kernel(float* __restrict__ d, const float* __restrict__ rho, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float r = rho[i];
    const float sg = btx_softplus_fast(r);
    d[i] = d[i] * ((2.0f * sg) * (1.0f / (1.0f + expf(-r))));
  }
}

// The weight operands of the two data-gradient contractions in one launch (modelled on dgrad_weights_kernel, btx_wgrad.hip):
// omu[c][tp][n] = mu[n][flip ? T-1-tp : tp][c], os2[c][tp][n] = f32(sigma * sigma) of the same source element.  32 x 32 (n, c) tiles
// of one tap through LDS: reads run along c, writes along n.
__global__ __launch_bounds__(256) void lrt_dgrad_weights_kernel(const float* __restrict__ mu, const float* __restrict__ rho,
                                                                float* __restrict__ omu, float* __restrict__ os2, int N, int T, int C,
                                                                int flip, int ctiles, int ntiles, int vec) {
  __shared__ float tm[32][33], ts[32][33];
  const int b = blockIdx.x;
  const int ct = b % ctiles, nt = (b / ctiles) % ntiles, t = b / (ctiles * ntiles);
  const int tp = flip ? T - 1 - t : t;
  const int tid = threadIdx.x;
  {
    const int r = tid >> 3, q = tid & 7;
    const int n = nt * 32 + r, c0 = ct * 32 + 4 * q;
    float m4[4] = {0.f, 0.f, 0.f, 0.f}, s4[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < N && c0 < C) {
      const size_t e0 = ((size_t)n * T + t) * C + c0;
      if (vec) {  // C % 4 == 0 and both pointers on the 16-byte grid
        const f32x4 a = *(const f32x4*)(mu + e0), bq = *(const f32x4*)(rho + e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { m4[e] = a[e]; const float sg = btx_softplus_fast(bq[e]); s4[e] = sg * sg; }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < C) { m4[e] = mu[e0 + e]; const float sg = btx_softplus_fast(rho[e0 + e]); s4[e] = sg * sg; }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { tm[r][4 * q + e] = m4[e]; ts[r][4 * q + e] = s4[e]; }
  }
  __syncthreads();
  {
    const int cc = tid >> 3, q = tid & 7;
    const int c = ct * 32 + cc, n0 = nt * 32 + 4 * q;
    if (c < C && n0 < N) {
      const size_t o0 = ((size_t)c * T + tp) * N + n0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < N) { omu[o0 + e] = tm[4 * q + e][cc]; os2[o0 + e] = ts[4 * q + e][cc]; }
    }
  }
}

size_t pad256(size_t v) { return (v + 255) & ~(size_t)255; }

// what btx_lrt_bwd runs on: the geometry of the data gradient and the sections of the workspace
struct LrtPlan {
  int Ho, Wo, T, flip;
  long long M, Mx;   // output / input pixels
  BtxGeom gT;        // the data gradient's contraction: Linear on W^T, stride 1 on the flipped kernel, else the transposed geometry
  uint32_t fT;       // its flags
  size_t o_gv, o_x2, o_mu, o_s2, o_B, o_wg, o_bg, wg_bytes, bg_bytes, total;
};

int lrt_plan(const BtxGeom* g, int act_dtype, int prec, LrtPlan* lp) {
  if (!g) return BTX_E_NULL;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16 && prec != BTX_PREC_BF16X3) return BTX_E_DTYPE;
  int32_t Do, Ho, Wo;
  int rc = btx_out_shape(g, 0, &Do, &Ho, &Wo);
  if (rc) return rc;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // as in the forward
  // Linear and 2-D convolutions with groups == 1 (autograd.fast_dgrad_ok): no depth axis, and at stride 1 the padding of the
  // flipped-kernel convolution, d (k - 1) - p, must not be negative
  if (g->groups != 1 || g->D != 1 || g->KD != 1 || g->sd != 1 || g->pd != 0 || g->dd != 1 || Do != 1) return BTX_E_UNSUPPORTED;
  const bool s1 = g->sh == 1 && g->sw == 1;
  if (s1 && (g->dh * (g->KH - 1) - g->ph < 0 || g->dw * (g->KW - 1) - g->pw < 0)) return BTX_E_UNSUPPORTED;
  memset(lp, 0, sizeof(*lp));
  lp->Ho = Ho; lp->Wo = Wo; lp->T = g->KH * g->KW;
  lp->M = (long long)g->NB * Ho * Wo;
  lp->Mx = (long long)g->NB * g->H * g->W;
  if ((unsigned long long)lp->M * (unsigned long long)g->N > 0xfffffffcULL) return BTX_E_UNSUPPORTED;  // BTX-RNG v1 block index: 32 bits
  if (lp->Mx > 0x7fffffffLL || lp->M > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  BtxGeom& t = lp->gT;
  t = *g;
  t.H = Ho; t.W = Wo; t.C = g->N; t.N = g->C;
  t.od = t.oh = t.ow = 0;
  if (s1) {
    t.ph = g->dh * (g->KH - 1) - g->ph; t.pw = g->dw * (g->KW - 1) - g->pw;
    lp->flip = 1; lp->fT = 0;
  } else {
    t.oh = (g->H + 2 * g->ph - g->dh * (g->KH - 1) - 1) % g->sh;
    t.ow = (g->W + 2 * g->pw - g->dw * (g->KW - 1) - 1) % g->sw;
    lp->flip = 0; lp->fT = BTX_FLAG_TRANSPOSED;
  }
  {  // the data gradient's contraction must land on x's extent
    int32_t d2, h2, w2;
    rc = btx_out_shape(&t, lp->fT, &d2, &h2, &w2);
    if (rc) return rc;
    if (h2 != g->H || w2 != g->W) return BTX_E_UNSUPPORTED;
  }
  const size_t esz = act_dtype == BTX_ACT_BF16 ? 2 : 4;
  const size_t E = (size_t)g->N * lp->T * g->C;
  lp->wg_bytes = btx_wgrad_workspace_bytes(BTX_KIND_REPARAM, g, act_dtype, 0);
  if (lp->wg_bytes == 0) return BTX_E_UNSUPPORTED;
  lp->bg_bytes = btx_bias_grad_workspace_bytes(lp->M, g->N);
  size_t o = 0;
  lp->o_gv = o; o += pad256((size_t)lp->M * g->N * esz);
  lp->o_x2 = o; o += pad256((size_t)lp->Mx * g->C * esz);
  lp->o_mu = o; o += pad256(E * 4);
  lp->o_s2 = o; o += pad256(E * 4);
  lp->o_B = o; o += pad256((size_t)lp->Mx * g->C * esz);
  lp->o_wg = o; o += pad256(lp->wg_bytes);
  lp->o_bg = o; o += pad256(lp->bg_bytes);
  lp->total = o + 256;  // the sections start at the first 256-byte boundary inside the caller's buffer
  return 0;
}

int ew_blocks(size_t n4) {
  size_t b = (n4 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" {

int btx_lrt_fwd_train(const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w, const float* mu_b, const float* rho_b,
                      void* out, float* root, const BtxRng* rng, int act_dtype, int prec, uint32_t flags, void* stream) {
  if (!g || !x || !mu_w || !rho_w || !out || !root || !rng) return BTX_E_NULL;
  if ((mu_b == nullptr) != (rho_b == nullptr)) return BTX_E_NULL;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16 && prec != BTX_PREC_BF16X3) return BTX_E_DTYPE;
  if (flags & ~(BTX_FLAG_GATHER | BTX_FLAG_REVERSE | BTX_FLAG_CONCURRENT)) return BTX_E_UNSUPPORTED;
  return contract_var(1, g, x, mu_w, rho_w, mu_b, rho_b, out, root, rng, act_dtype, prec, flags, stream);
}

int btx_lrt_bwd_workspace_bytes(const BtxGeom* g, int act_dtype, int prec, size_t* bytes) {
  if (!g || !bytes) return BTX_E_NULL;
  LrtPlan lp;
  const int rc = lrt_plan(g, act_dtype, prec, &lp);
  if (rc) return rc;
  *bytes = lp.total;
  return 0;
}

int btx_lrt_bwd(const BtxGeom* g, const void* x, const void* dy, const float* root, const float* mu_w, const float* rho_w,
                const float* rho_b, const BtxLrtGrads* out, const BtxRng* rng, int act_dtype, int prec, void* ws, size_t ws_bytes,
                void* stream) {
  if (!g || !x || !dy || !root || !mu_w || !rho_w || !out || !rng) return BTX_E_NULL;
  if (out->drho_b && !rho_b) return BTX_E_NULL;
  LrtPlan lp;
  int rc = lrt_plan(g, act_dtype, prec, &lp);
  if (rc) return rc;
  if (!ws || ws_bytes < lp.total) return BTX_E_WORKSPACE;
  unsigned char* base = (unsigned char*)((((uintptr_t)ws) + 255) & ~(uintptr_t)255);
  hipStream_t st = (hipStream_t)stream;
  const bool bf = act_dtype == BTX_ACT_BF16;
  const size_t n_out = (size_t)lp.M * g->N, n_in = (size_t)lp.Mx * g->C, E = (size_t)g->N * lp.T * g->C;
  void* gv = base + lp.o_gv;
  void* x2 = base + lp.o_x2;
  float* muT = (float*)(base + lp.o_mu);
  float* s2T = (float*)(base + lp.o_s2);
  void* Bb = base + lp.o_B;
  const bool want_gv = out->drho_w || out->drho_b || out->dx;
  if (want_gv) {
    const LrtRng rg = {(uint32_t)rng->seed, (uint32_t)(rng->seed >> 32), rng->sample_idx, rng->layer_id, rng->sample_idx_dev};
    const int nb = ew_blocks((n_out + 3) / 4);
    if (bf) hipLaunchKernelGGL(lrt_gv_kernel<__bf16>, dim3(nb), dim3(256), 0, st, (const __bf16*)dy, root, (__bf16*)gv, n_out, rg);
    else hipLaunchKernelGGL(lrt_gv_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)dy, root, (float*)gv, n_out, rg);
    rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  if (out->dmu_b) {
    rc = btx_bias_grad(BTX_KIND_REPARAM, dy, lp.M, g->N, act_dtype, out->dmu_b, nullptr, rng, nullptr, 0, base + lp.o_bg, lp.bg_bytes, stream);
    if (rc) return rc;
  }
  if (out->drho_b) {
    rc = btx_bias_grad(BTX_KIND_REPARAM, gv, lp.M, g->N, act_dtype, out->drho_b, nullptr, rng, nullptr, 0, base + lp.o_bg, lp.bg_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lrt_rho_scale_kernel, dim3(ew_blocks((size_t)g->N)), dim3(256), 0, st, out->drho_b, rho_b, (size_t)g->N);
    rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  if (out->dmu_w) {
    rc = btx_contract_wgrad_ws(BTX_KIND_REPARAM, g, x, dy, out->dmu_w, nullptr, nullptr, nullptr, rng, nullptr, act_dtype, 0,
                               base + lp.o_wg, lp.wg_bytes, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  if (out->drho_w) {
    const int nb = ew_blocks((n_in + 3) / 4);
    if (bf) hipLaunchKernelGGL(lrt_square_kernel<__bf16>, dim3(nb), dim3(256), 0, st, (const __bf16*)x, (__bf16*)x2, n_in);
    else hipLaunchKernelGGL(lrt_square_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)x, (float*)x2, n_in);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    rc = btx_contract_wgrad_ws(BTX_KIND_REPARAM, g, x2, gv, out->drho_w, nullptr, nullptr, nullptr, rng, nullptr, act_dtype, 0,
                               base + lp.o_wg, lp.wg_bytes, nullptr, nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(lrt_rho_scale_kernel, dim3(ew_blocks(E)), dim3(256), 0, st, out->drho_w, rho_w, E);
    rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  if (out->dx) {
    const int ctiles = (g->C + 31) / 32, ntiles = (g->N + 31) / 32;
    const long long nwg = (long long)ctiles * ntiles * lp.T;
    if (nwg > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
    const int vec = ((g->C & 3) == 0 && ((((uintptr_t)mu_w) | ((uintptr_t)rho_w)) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(lrt_dgrad_weights_kernel, dim3((int)nwg), dim3(256), 0, st, mu_w, rho_w, muT, s2T, g->N, lp.T, g->C, lp.flip,
                       ctiles, ntiles, vec);
    rc = (int)hipGetLastError();
    if (rc) return rc;
    rc = contract_var(2, &lp.gT, gv, s2T, s2T, nullptr, nullptr, Bb, nullptr, rng, act_dtype, prec, lp.fT, stream);
    if (rc) return rc;
    rc = contract_var(2, &lp.gT, dy, muT, muT, nullptr, nullptr, out->dx, nullptr, rng, act_dtype, prec, lp.fT, stream);
    if (rc) return rc;
    const int nb = ew_blocks((n_in + 3) / 4);
    if (bf) hipLaunchKernelGGL(lrt_combine_kernel<__bf16>, dim3(nb), dim3(256), 0, st, (__bf16*)out->dx, (const __bf16*)x, (const __bf16*)Bb, n_in);
    else hipLaunchKernelGGL(lrt_combine_kernel<float>, dim3(nb), dim3(256), 0, st, (float*)out->dx, (const float*)x, (const float*)Bb, n_in);
    rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
