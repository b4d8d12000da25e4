// btx_contract_dw.h — BTX-DW v1: depthwise Bayesian 2-D convolutions (groups == C == N) as a VALU stencil for gfx950.
//
// A depthwise layer is 9 (.. 49) multiply-adds per output element: memory-bound, and with Cg = 1 no MFMA family fits it (the gather
// kernel spends a 64-channel MFMA tile per channel).  Here nothing multiplies matrices:
//   * a workgroup of 256 threads owns DW_CB = 64 channels (128 bytes of bf16: one full line per pixel) x a TH x TW output tile of one
//     image (btx_plan.cpp make_dw_plan); thread (gc, slot): gc = tid % granules is the 16-byte channel granule and runs fastest, so
//     every global load, LDS access and store of a wave covers whole contiguous lines; `slot` walks runs of R = DW_R adjacent output
//     pixels along W;
//   * prologue: the block's T x 64 weights are sampled ONCE per workgroup into LDS as f32 [t][c] — noise index c * T + t, the block's
//     indices c0 * T .. (c0 + 64) * T - 1 are one contiguous 4-aligned range, so every Philox call is used whole; same
//     btx_normal4_hw / btx_softplus_hw and the same roundings as the sampling pre-pass of the MFMA families (btx_presample.h);
//   * the halo'd input patch goes to LDS in 16-byte granules through registers (zero-filled outside the image, ragged channel
//     blocks and the sign bytes below rule the LDS-DMA out); Flipout: a granule lies inside one 32-sign word — the loading thread
//     hashes the word once and leaves the granule's sign bits in a byte plane beside the patch; the compute loop forms x * s_in by
//     XOR on the sign bit;
//   * f32 FMAs into R x G accumulators (twice for Flipout), taps in row-major order whatever the pixel's place in the tile; the
//     3x3 / dilation 1 / stride 1 | 2 forms keep a register window along W ((R - 1) * s + 3 LDS reads per kernel row instead of
//     3 * R); weights are read per tap from LDS (all lanes of a granule read one address: a broadcast);
//   * store straight from the registers: bias, s_out combine (one hash per granule), scale / shift, residual (one 16-byte load),
//     activation, convert, one 16-byte store.  No LDS staging, no barrier behind the compute loop.
// BTX_FLAG_TRANSPOSED: the gather rule of contract_kernel (output pixel o reads input (o + pad - k * dil) / stride where that is a
// whole, in-range number) on the same patch machinery — the data gradient of a depthwise layer.
#pragma once
#include "btx_contract.h"

namespace btx {

constexpr int DW_THREADS = 256;

template <typename ACT, int KIND, int SPEC>  // SPEC: 0 run-time taps (and every transposed launch); 1 | 2: 3x3, dilation 1, stride SPEC
__global__ __launch_bounds__(DW_THREADS, 2) void contract_dw_kernel(const ContractParams pk) {
  constexpr int G = 16 / (int)sizeof(ACT);    // channels per 16-byte granule
  constexpr int NGC = DW_CB / G;              // granules per pixel of the block
  constexpr int SLOTS = DW_THREADS / NGC;     // pixel runs in flight
  constexpr int R = DW_R;
  constexpr int PIXB = DW_CB * (int)sizeof(ACT);
  int logical = xcd_logical();
  const ContractParams p = lane_view(pk, logical);
  const RngLive rl = rng_live<KIND>(p);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int T = p.KH * p.KW;
  float* w_m = (float*)smem;                           // [T][64]: W, or mu for Flipout
  float* w_d = w_m + T * DW_CB;                        // [T][64]: sigma * eps (Flipout)
  float* cst = w_m + (KIND == 1 ? 2 : 1) * T * DW_CB;  // [4][64]: bias mean | bias delta | scale | shift
  unsigned char* patch = (unsigned char*)(cst + 4 * DW_CB);  // [PH * PW][64 channels]
  unsigned char* sgn = patch + p.pt_PP * PIXB;         // [PH * PW][NGC]: the s_in bits of each granule (Flipout)

  // ---- workgroup -> (image, row tile, column tile, channel block); channel blocks of one tile are neighbours (adjacent lines of x)
  uint32_t cb, t1, ct, t2, rt, nb;
  fdivmod((uint32_t)logical, p.fd_ntiles, (uint32_t)p.ntiles, t1, cb);
  fdivmod(t1, p.fd_ncs, (uint32_t)p.pt_ncs, t2, ct);
  fdivmod(t2, p.fd_rtiles, (uint32_t)p.pt_rtiles, nb, rt);
  const int c0 = (int)cb * DW_CB;
  const int nch = min(DW_CB, p.C - c0);  // a whole number of granules (host: C % G == 0)
  const int gc = tid % NGC, slot = tid / NGC;
  const bool g_ok = gc * G < nch;
  const int oh0 = (int)rt * p.pt_R, ow0 = (int)ct * p.pt_Wt;
  const int th_n = min(p.pt_R, p.Ho - oh0), tw_n = min(p.pt_Wt, p.Wo - ow0);
  const int PW = p.pt_Wp;
  int ih0, iw0;  // input pixel of patch element (0, 0)
  if (!p.transposed) {
    ih0 = oh0 * p.sh - p.ph; iw0 = ow0 * p.sw - p.pw;
  } else {
    ih0 = (int)fdiv((uint32_t)max(0, oh0 + p.ph - (p.KH - 1) * p.dh), p.fd_sh);
    iw0 = (int)fdiv((uint32_t)max(0, ow0 + p.pw - (p.KW - 1) * p.dw), p.fd_sw);
  }

  // ---- prologue 1: sample the block's weights, one quad (4 consecutive noise indices = one Philox call) per thread and step
  {
    const uint32_t nq = (uint32_t)(nch * T) >> 2, e_base = (uint32_t)c0 * (uint32_t)T;
    for (uint32_t q = (uint32_t)tid; q < nq; q += DW_THREADS) {
      const uint32_t e0 = e_base + 4u * q;
      const f32x4 m4 = *(const f32x4*)(p.mu + e0), r4 = *(const f32x4*)(p.rho + e0);
      float eps[4];
      if (p.eps_w) {  // explicit noise (the data gradient regenerates the forward's eps in its own layout)
        const f32x4 e4 = *(const f32x4*)(p.eps_w + e0);
        eps[0] = e4[0]; eps[1] = e4[1]; eps[2] = e4[2]; eps[3] = e4[3];
      } else {
        btx_normal4_hw(e0 >> 2, rl.sample, p.layer, 0u, p.seed_lo, p.seed_hi, eps);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t cl, t;
        fdivmod(4u * q + (uint32_t)j, p.fd_inner, (uint32_t)T, cl, t);
        const float sg = btx_softplus_hw(r4[j]);
        float wm, wd = 0.f;
        if constexpr (KIND == 0) wm = __builtin_fmaf(sg, eps[j], m4[j]);
        else { wm = m4[j]; wd = sg * eps[j]; }
        if (p.dw_round) { wm = (float)(__bf16)wm; wd = (float)(__bf16)wd; }  // bf16 contraction: operands rounded once, to nearest even
        w_m[t * DW_CB + cl] = wm;
        if constexpr (KIND == 1) w_d[t * DW_CB + cl] = wd;
      }
    }
  }
  // ---- prologue 2: per-channel constants of the store (as ep_store_constants of btx_epilogue.h draws the bias)
  const bool has_bias = p.mu_b != nullptr, has_aff = (p.ep_scale != nullptr) || (p.ep_shift != nullptr);
  if (tid < DW_CB) {
    float bm = 0.f, bd = 0.f, sc = 1.f, sh = 0.f;
    if (tid < nch) {
      const int c = c0 + tid;
      if (has_bias) {
        const float eb = p.eps_b ? p.eps_b[c] : btx_normal1((unsigned long long)c, rl.sample, p.layer, 1u, p.seed_lo, p.seed_hi);
        const float sb_ = btx_softplus_fast(p.rho_b[c]);
        if constexpr (KIND == 0) { bm = __builtin_fmaf(sb_, eb, p.mu_b[c]); }
        else { bm = p.mu_b[c]; bd = sb_ * eb; }
      }
      if (p.ep_scale) sc = p.ep_scale[c];
      if (p.ep_shift) sh = p.ep_shift[c];
    }
    cst[tid] = bm; cst[DW_CB + tid] = bd; cst[2 * DW_CB + tid] = sc; cst[3 * DW_CB + tid] = sh;
  }
  // ---- prologue 3: the input patch, 16 bytes per thread and step; gc is the thread's granule in every step (256 % NGC == 0)
  {
    const ACT* __restrict__ xptr = (const ACT*)p.x;
    const int npix = p.pt_PP;
    for (int pix = slot; pix < npix; pix += SLOTS) {
      uint32_t pr, pc;
      fdivmod((uint32_t)pix, p.fd_ptWp, (uint32_t)PW, pr, pc);
      const int ih = ih0 + (int)pr, iw = iw0 + (int)pc;
      const bool ok = g_ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      u32x4 v = {0u, 0u, 0u, 0u};
      uint32_t sbyte = 0;
      if (ok) {
        const long long off = (((long long)nb * p.H + ih) * p.W + iw) * p.C + c0 + gc * G;
        v = *(const u32x4*)(xptr + off);
        if constexpr (sizeof(ACT) == 4) {
          if (p.dw_round) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = f2u((float)(__bf16)u2f(v[j]));
          }
        }
        if constexpr (KIND == 1) {
          // element e = off & 31 of the word sits at bit btx_sign_bitpos(e); shifted so that the granule's elements 0, 1, 2, .. sit
          // at bits 15, 31, 14, 30, .. (the order sign_mask_bf16 reads)
          const unsigned long long i0 = (unsigned long long)off;
          const uint32_t w = btx_sign_word((uint32_t)(i0 >> 5), rl.kin_a, rl.kin_b);
          const uint32_t ws = w << ((int)((i0 >> 3) & 3) * 4 + (G == 4 ? (int)((i0 >> 2) & 1) * 2 : 0));
          if constexpr (G == 8) sbyte = ((ws >> 12) & 0xFu) | ((ws >> 24) & 0xF0u);  // bits 15..12 | 31..28
          else sbyte = ((ws >> 14) & 0x3u) | ((ws >> 28) & 0xCu);                    // bits 15..14 | 31..30
        }
      }
      *(u32x4*)(patch + pix * PIXB + gc * 16) = v;
      if constexpr (KIND == 1) sgn[pix * NGC + gc] = (unsigned char)sbyte;
    }
  }
  __syncthreads();

  // one tap of one pixel: G channels of granule `a` (sign byte `sb`) against the tap's weights
  auto fma_tap = [&](const u32x4 a, uint32_t sb, const f32x4* wm, const f32x4* wd, float* am, float* ad) __attribute__((always_inline)) {
    if constexpr (G == 8) {
      const uint32_t e = ((sb & 0xFu) << 12) | ((sb & 0xF0u) << 24);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        am[2 * d] = __builtin_fmaf(u2f(a[d] << 16), wm[d >> 1][(2 * d) & 3], am[2 * d]);
        am[2 * d + 1] = __builtin_fmaf(u2f(a[d] & 0xffff0000u), wm[d >> 1][(2 * d + 1) & 3], am[2 * d + 1]);
        if constexpr (KIND == 1) {
          const uint32_t a2 = a[d] ^ ((e << d) & 0x80008000u);
          ad[2 * d] = __builtin_fmaf(u2f(a2 << 16), wd[d >> 1][(2 * d) & 3], ad[2 * d]);
          ad[2 * d + 1] = __builtin_fmaf(u2f(a2 & 0xffff0000u), wd[d >> 1][(2 * d + 1) & 3], ad[2 * d + 1]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        am[j] = __builtin_fmaf(u2f(a[j]), wm[0][j], am[j]);
        if constexpr (KIND == 1) {
          const int sft = (j == 0) ? 30 : (j == 1) ? 28 : (j == 2) ? 31 : 29;  // byte bits 1, 3, 0, 2 hold elements 0, 1, 2, 3
          ad[j] = __builtin_fmaf(u2f(a[j] ^ ((sb << sft) & 0x80000000u)), wd[0][j], ad[j]);
        }
      }
    }
  };
  auto load_w = [&](int tap, f32x4* wm, f32x4* wd) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < G / 4; ++i) {
      wm[i] = *(const f32x4*)(w_m + tap * DW_CB + gc * G + 4 * i);
      if constexpr (KIND == 1) wd[i] = *(const f32x4*)(w_d + tap * DW_CB + gc * G + 4 * i);
    }
  };

  // ---- compute + store: runs of R adjacent output pixels, `RW` runs per tile row
  const int RW = p.pt_NI, nruns = th_n * RW;
  for (int run = slot; run < nruns; run += SLOTS) {
    uint32_t tr, rc;
    fdivmod((uint32_t)run, p.fd_ptR, (uint32_t)RW, tr, rc);
    const int oh = oh0 + (int)tr, owb = (int)rc * R;  // owb: the run's first column inside the tile
    if (!g_ok || owb >= tw_n) continue;
    float am[R][G], ad[KIND == 1 ? R : 1][G];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < G; ++j) { am[r][j] = 0.f; if constexpr (KIND == 1) ad[r][j] = 0.f; }
    f32x4 wm[G / 4], wd[G / 4];

    if constexpr (SPEC != 0) {
      constexpr int S = SPEC, WN = (R - 1) * S + 3;  // the register window of one kernel row
#pragma unroll 1  // (unrolled, the scheduler requests all three rows' windows and all nine taps' weights at once: scratch)
      for (int kh = 0; kh < 3; ++kh) {
        const int base = ((int)tr * S + kh) * PW, col = owb * S;
        u32x4 win[WN];
        uint32_t sb[WN];
#pragma unroll
        for (int i = 0; i < WN; ++i) {  // columns beyond the patch belong to pixels beyond the tile, which are not stored
          const int pix = base + min(col + i, PW - 1);
          win[i] = *(const u32x4*)(patch + pix * PIXB + gc * 16);
          sb[i] = 0;
          if constexpr (KIND == 1) sb[i] = sgn[pix * NGC + gc];
        }
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          load_w(kh * 3 + kw, wm, wd);
#pragma unroll
          for (int r = 0; r < R; ++r) fma_tap(win[r * S + kw], sb[r * S + kw], wm, wd, am[r], ad[KIND == 1 ? r : 0]);
        }
      }
    } else if (!p.transposed) {
      for (int kh = 0; kh < p.KH; ++kh) {
        const int base = ((int)tr * p.sh + kh * p.dh) * PW;
        for (int kw = 0; kw < p.KW; ++kw) {
          load_w(kh * p.KW + kw, wm, wd);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int pix = base + min((owb + r) * p.sw + kw * p.dw, PW - 1);
            uint32_t sb = 0;
            if constexpr (KIND == 1) sb = sgn[pix * NGC + gc];
            fma_tap(*(const u32x4*)(patch + pix * PIXB + gc * 16), sb, wm, wd, am[r], ad[KIND == 1 ? r : 0]);
          }
        }
      }
    } else {
      // ConvTranspose gather rule: tap (kh, kw) reaches output (oh, ow) from input ((oh + ph - kh * dh) / sh, ..) where that is whole
      for (int kh = 0; kh < p.KH; ++kh) {
        const int th = oh + p.ph - kh * p.dh;
        if (th < 0) continue;
        const int ih = (int)fdiv((uint32_t)th, p.fd_sh);
        if (ih * p.sh != th || ih >= p.H || ih - ih0 >= p.pt_Rp) continue;
        const int base = (ih - ih0) * PW;
        for (int kw = 0; kw < p.KW; ++kw) {
          load_w(kh * p.KW + kw, wm, wd);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int tw = ow0 + owb + r + p.pw - kw * p.dw;
            const int iw = (int)fdiv((uint32_t)max(tw, 0), p.fd_sw);
            if (tw < 0 || iw * p.sw != tw || iw >= p.W || iw - iw0 >= PW) continue;
            const int pix = base + iw - iw0;
            uint32_t sb = 0;
            if constexpr (KIND == 1) sb = sgn[pix * NGC + gc];
            fma_tap(*(const u32x4*)(patch + pix * PIXB + gc * 16), sb, wm, wd, am[r], ad[KIND == 1 ? r : 0]);
          }
        }
      }
    }

    // ---- store, straight from the registers
    float bm[G], bd[G], sc[G], sh[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      bm[j] = cst[gc * G + j]; bd[j] = cst[DW_CB + gc * G + j];
      sc[j] = cst[2 * DW_CB + gc * G + j]; sh[j] = cst[3 * DW_CB + gc * G + j];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (owb + r >= tw_n) continue;
      const long long o = (((long long)nb * p.Ho + oh) * p.Wo + (ow0 + owb + r)) * p.N + c0 + gc * G;
      uint32_t ws = 0;
      if constexpr (KIND == 1) {
        const unsigned long long i0 = (unsigned long long)o;
        ws = btx_sign_word((uint32_t)(i0 >> 5), rl.kout_a, rl.kout_b) << ((int)((i0 >> 3) & 3) * 4 + (G == 4 ? (int)((i0 >> 2) & 1) * 2 : 0));
      }
      float v[G];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        float val = am[r][j];
        if (has_bias) val += bm[j];
        if constexpr (KIND == 1) {
          float dl = ad[r][j];
          if (has_bias) dl += bd[j];
          const int bit = ((j & 1) ? 31 : 15) - (j >> 1);
          val += u2f(f2u(dl) ^ ((ws << (31 - bit)) & 0x80000000u));
        }
        if (has_aff) val = __builtin_fmaf(val, sc[j], sh[j]);
        v[j] = val;
      }
      if (p.ep_res) {
        if (p.out_bf16) {
          const __bf16* rp = (const __bf16*)p.ep_res + o;
          uint32_t rw[G / 2];
          if constexpr (G == 8) { const u32x4 t = *(const u32x4*)rp; rw[0] = t[0]; rw[1] = t[1]; rw[2] = t[2]; rw[3] = t[3]; }
          else { const u32x2 t = *(const u32x2*)rp; rw[0] = t[0]; rw[1] = t[1]; }
#pragma unroll
          for (int j = 0; j < G / 2; ++j) { v[2 * j] += u2f(rw[j] << 16); v[2 * j + 1] += u2f(rw[j] & 0xffff0000u); }
        } else {
          const float* rp = (const float*)p.ep_res + o;
#pragma unroll
          for (int i = 0; i < G / 4; ++i) {
            const f32x4 t = *(const f32x4*)(rp + 4 * i);
            v[4 * i] += t[0]; v[4 * i + 1] += t[1]; v[4 * i + 2] += t[2]; v[4 * i + 3] += t[3];
          }
        }
      }
      if (p.ep_relu) {
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
        if (p.ep_relu == 2) {
#pragma unroll
          for (int j = 0; j < G; ++j) v[j] = v[j] < 6.f ? v[j] : 6.f;
        }
      }
      if (p.out_bf16) {
        __bf16* dst = (__bf16*)p.out + o;
        if constexpr (G == 8) {
          const f32x8 f = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
          *(bf16x8*)dst = __builtin_convertvector(f, bf16x8);
        } else {
          const f32x4 f = {v[0], v[1], v[2], v[3]};
          *(bf16x4*)dst = __builtin_convertvector(f, bf16x4);
        }
      } else {
        float* dst = (float*)p.out + o;
#pragma unroll
        for (int i = 0; i < G / 4; ++i) *(f32x4*)(dst + 4 * i) = (f32x4){v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
      }
    }
  }
}

template <typename ACT>
static int launch_contract_dw_impl(int kind, const ContractParams& p, int nwg, hipStream_t st) {
  const int spec = (!p.transposed && p.KH == 3 && p.KW == 3 && p.dh == 1 && p.dw == 1 && p.sh == p.sw && (p.sh == 1 || p.sh == 2)) ? p.sh : 0;
#define BTX_LAUNCH_DW(KIND, SPEC)                                                                                     \
  do {                                                                                                                \
    auto kfn = contract_dw_kernel<ACT, KIND, SPEC>;                                                                   \
    static bool attr_done = false;                                                                                    \
    if (!attr_done) {                                                                                                 \
      hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, DW_LDS_CAP);   \
      if (e != hipSuccess) return (int)e;                                                                             \
      attr_done = true;                                                                                               \
    }                                                                                                                 \
    hipLaunchKernelGGL(kfn, dim3(nwg), dim3(DW_THREADS), p.pt_lds, st, p);                                            \
  } while (0)
  if (kind == 0) { if (spec == 1) BTX_LAUNCH_DW(0, 1); else if (spec == 2) BTX_LAUNCH_DW(0, 2); else BTX_LAUNCH_DW(0, 0); }
  else           { if (spec == 1) BTX_LAUNCH_DW(1, 1); else if (spec == 2) BTX_LAUNCH_DW(1, 2); else BTX_LAUNCH_DW(1, 0); }
#undef BTX_LAUNCH_DW
  return (int)hipGetLastError();
}

}  // namespace btx
