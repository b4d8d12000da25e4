// btx_contract_dw_wgrad.h — BTX-DW v1: the WEIGHT gradient of a depthwise Bayesian 2-D convolution (groups == C == N)
// as a VALU stencil reduction for gfx950.  In the GEMM-major order [C][T] of mu_w:
//
//   dw_mu[c][t]    = sum over (n, oh, ow) of  x[n, oh*sh - ph + kh*dh, ow*sw - pw + kw*dw, c] * dy[n, oh, ow, c]        t = kh * KW + kw
//   dw_delta[c][t] = the same sum of (x * s_in) * (dy * s_out)                                                          (Flipout)
//
// s_in / s_out: the hashed BTX-RNG v1 signs at the element's linear index in x / dy (what wgrad_kernel and contract_dw_kernel draw).
// A per-channel reduction over all pixels — memory-bound; the generic kernel spends a 64 x 64 MFMA tile per (channel, tap) and reads
// x and dy T times at 1/64 of every line.  Here (btx_plan.cpp make_dw_wgrad_plan):
//   * a workgroup of 256 threads owns DW_CB = 64 channels (one full 128-byte line of bf16 per pixel), one tap group and one SLAB: a run
//     of consecutive TH x TW output tiles in (image, row tile, column tile) order; thread (gc, slot): gc = tid % granules is the
//     16-byte channel granule and runs fastest, so every global load and LDS access of a wave covers whole contiguous lines;
//   * per tile the halo'd x patch goes to LDS in 16-byte granules through registers, zero-filled outside the image; Flipout: the
//     loading thread hashes the granule's 32-sign word once and leaves its sign bits in a byte plane beside the patch (the layout of
//     contract_dw_kernel);
//   * the thread then walks the tile's pixels slot, slot + SLOTS, ..: the dy granule comes from global memory with one 16-byte load
//     (two pixels ahead of the one being multiplied), s_out by XOR (one hash per granule); per tap one 16-byte LDS read of the patch
//     and G FMAs into f32 registers, one accumulator per (tap, channel of the granule) — twice for Flipout, on the sign-flipped
//     operands.  The accumulators live across all tiles of the slab;
//   * FORM 1 (3x3, dilation 1): all nine taps in one pass, 9 x G accumulators (x 2).  FORM 0 (run-time taps, T <= 49, KW <= 7): a
//     workgroup takes ONE kernel row (7 x G accumulators, x 2) and stages only the input rows that row reads; the KH rows are
//     workgroups of their own, so nothing spills and a 7x7 layer has seven times the workgroups to fill the chip with;
//   * fixed summation order: a thread adds its pixels in order and its tiles in tile order; the slots of a granule are added through
//     LDS in slot order; the workgroup leaves plain stores of its [nk][64 x taps] sums in its slab (or, with one slab, in dw_*).  No
//     atomics.  wgrad_finish_kernel (btx_wgrad.hip) adds the slabs in slab order and forms drho.
// Bounds: global reads happen only for in-image patch pixels / in-tile output pixels of channels < C (g_ok), at offsets below the
// element counts the planner checked against 2^31; LDS pixel indices stay below rows x PW because PW = (TW - 1) sw + (KW - 1) dw + 1
// and a tile row reads patch row tr * sh + kh <= (th - 1) sh + 2 (FORM 1) or tr (FORM 0); a workgroup stores channels c0 .. c0 + nch - 1
// of its own slab only, and slabs = ceil(tiles / tps) leaves no slab without tiles.  Threads of a ragged block's missing granules
// stage zeros, accumulate nothing and take part in every barrier.
#pragma once
#include "btx_contract.h"

namespace btx {

struct DwWgradParams {
  const void* x;
  const void* dy;
  float* out_m;  // one slab: the sums ARE the result
  float* out_d;
  float* slab;   // [slab][mean | delta][C * T]
  int NB, H, W, C, Ho, Wo, KH, KW, T, sh, sw, ph, pw, dh, dw;
  int TH, TW, PW, rtiles, ctiles, cblocks, ngrp, tiles, tps, direct;
  uint32_t kin_a, kin_b, kout_a, kout_b;
  const uint32_t* sample_ptr;  // BtxRng.sample_idx_dev: the sign keys are then derived on the device (captured training steps)
  uint32_t seed_lo, seed_hi, layer;
  int swap;
  FastDiv fd_cblocks, fd_ngrp, fd_ctiles, fd_rtiles, fd_TW, fd_PW;
};

template <typename ACT, int KIND, int FORM>
__global__ __launch_bounds__(DW_THREADS, 2) void dw_wgrad_kernel(const DwWgradParams p) {
  constexpr int G = 16 / (int)sizeof(ACT);  // channels per 16-byte granule
  constexpr int NGC = DW_CB / G;            // granules per pixel of the block
  constexpr int SLOTS = DW_THREADS / NGC;   // pixels in flight
  constexpr int PIXB = DW_CB * (int)sizeof(ACT);
  constexpr int NKH = FORM ? 3 : 1, NKW = FORM ? 3 : 7, NT = NKH * NKW;
  constexpr int RT = DWW_RED_TAPS;
  static_assert(RT * DW_CB == DW_THREADS, "the closing reduction gives every thread one (tap of the round, channel)");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  // sign keys of this (sample, layer): the host's, or — with a device-resident sample index — derived here, as wgrad_kernel does
  uint32_t kin_a = p.kin_a, kin_b = p.kin_b, kout_a = p.kout_a, kout_b = p.kout_b;
  if (KIND == 1 && p.sample_ptr) {
    const uint32_t smp = __builtin_amdgcn_readfirstlane(*p.sample_ptr);
    const uint32_t si = p.swap ? BTX_STREAM_SIGN_OUT : BTX_STREAM_SIGN_IN, so = p.swap ? BTX_STREAM_SIGN_IN : BTX_STREAM_SIGN_OUT;
    const BtxPhilox4 ki = btx_philox4x32_10(0u, smp, p.layer, si, p.seed_lo, p.seed_hi);
    const BtxPhilox4 ko = btx_philox4x32_10(0u, smp, p.layer, so, p.seed_lo, p.seed_hi);
    kin_a = __builtin_amdgcn_readfirstlane(ki.x[0]); kin_b = __builtin_amdgcn_readfirstlane(ki.x[1]);
    kout_a = __builtin_amdgcn_readfirstlane(ko.x[0]); kout_b = __builtin_amdgcn_readfirstlane(ko.x[1]);
  }

  // ---- workgroup -> (slab, tap group, channel block); channel blocks of one slab are neighbours (adjacent lines of x and dy)
  uint32_t cb, u1, grp, slab;
  fdivmod(blockIdx.x, p.fd_cblocks, (uint32_t)p.cblocks, u1, cb);
  fdivmod(u1, p.fd_ngrp, (uint32_t)p.ngrp, slab, grp);
  const int c0 = (int)cb * DW_CB;
  const int nch = min(DW_CB, p.C - c0);  // a whole number of granules (host: C % G == 0)
  const int gc = tid % NGC, slot = tid / NGC;
  const bool g_ok = gc * G < nch;
  const int kh0 = FORM ? 0 : (int)grp;   // FORM 0: the kernel row of this workgroup
  const int PW = p.PW;
  unsigned char* patch = smem;                                   // [rows * PW][64 channels]
  unsigned char* sgn = patch + (FORM ? (p.TH - 1) * p.sh + 3 : p.TH) * PW * PIXB;  // [rows * PW][NGC]: the s_in bits of each granule

  float am[NT][G], ad[KIND == 1 ? NT : 1][G];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < G; ++j) { am[t][j] = 0.f; if constexpr (KIND == 1) ad[t][j] = 0.f; }

  const ACT* __restrict__ xptr = (const ACT*)p.x;
  const ACT* __restrict__ yptr = (const ACT*)p.dy;
  const int u_end = min(p.tiles, ((int)slab + 1) * p.tps);
  for (int u = (int)slab * p.tps; u < u_end; ++u) {
    uint32_t t1, ct, rt, nb;
    fdivmod((uint32_t)u, p.fd_ctiles, (uint32_t)p.ctiles, t1, ct);
    fdivmod(t1, p.fd_rtiles, (uint32_t)p.rtiles, nb, rt);
    const int oh0 = (int)rt * p.TH, ow0 = (int)ct * p.TW;
    const int th_n = min(p.TH, p.Ho - oh0), tw_n = min(p.TW, p.Wo - ow0);
    // patch row pr holds input row ih0 + pr * rstep: the whole footprint (FORM 1), the rows kernel row kh0 reads (FORM 0)
    const int ih0 = oh0 * p.sh - p.ph + kh0 * p.dh, iw0 = ow0 * p.sw - p.pw;
    const int rstep = FORM ? 1 : p.sh, nrows = FORM ? (th_n - 1) * p.sh + 3 : th_n;

    __syncthreads();  // the previous tile's readers are done with the patch
    // ---- the input patch, 16 bytes per thread and step, four loads in flight; gc is the thread's granule in every step
    {
      const int npix = nrows * PW;
      for (int pix0 = slot; pix0 < npix; pix0 += 4 * SLOTS) {
        u32x4 v[4];
        uint32_t sbyte[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int pix = pix0 + k * SLOTS;
          uint32_t pr, pc;
          fdivmod((uint32_t)min(pix, npix - 1), p.fd_PW, (uint32_t)PW, pr, pc);
          const int ih = ih0 + (int)pr * rstep, iw = iw0 + (int)pc;
          const bool ok = pix < npix && g_ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
          v[k] = (u32x4){0u, 0u, 0u, 0u};
          sbyte[k] = 0;
          if (ok) {
            const long long off = (((long long)nb * p.H + ih) * p.W + iw) * p.C + c0 + gc * G;
            v[k] = *(const u32x4*)(xptr + off);
            if constexpr (KIND == 1) {
              // element e = off & 31 of the word sits at bit btx_sign_bitpos(e); shifted so that the granule's elements 0, 1, 2, .. sit
              // at bits 15, 31, 14, 30, .. (contract_dw_kernel)
              const unsigned long long i0 = (unsigned long long)off;
              const uint32_t w = btx_sign_word((uint32_t)(i0 >> 5), kin_a, kin_b);
              const uint32_t ws = w << ((int)((i0 >> 3) & 3) * 4 + (G == 4 ? (int)((i0 >> 2) & 1) * 2 : 0));
              if constexpr (G == 8) sbyte[k] = ((ws >> 12) & 0xFu) | ((ws >> 24) & 0xF0u);  // bits 15..12 | 31..28
              else sbyte[k] = ((ws >> 14) & 0x3u) | ((ws >> 28) & 0xCu);                    // bits 15..14 | 31..30
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int pix = pix0 + k * SLOTS;
          if (pix < npix) {
            *(u32x4*)(patch + pix * PIXB + gc * 16) = v[k];
            if constexpr (KIND == 1) sgn[pix * NGC + gc] = (unsigned char)sbyte[k];
          }
        }
      }
    }
    __syncthreads();

    // ---- the tile's pixels: i = tr * TW + col, this thread's are slot, slot + SLOTS, ..; dy two pixels ahead
    struct Dy {
      u32x4 v;
      uint32_t o;  // element offset of the granule in dy (its sign word)
      int tr, col;
      bool ok;
    };
    const int npx = th_n * p.TW;
    auto fetch = [&](int i) __attribute__((always_inline)) -> Dy {
      Dy d;
      uint32_t tr, col;
      fdivmod((uint32_t)i, p.fd_TW, (uint32_t)p.TW, tr, col);
      d.tr = (int)tr; d.col = (int)col;
      d.ok = g_ok && i < npx && (int)col < tw_n;
      d.v = (u32x4){0u, 0u, 0u, 0u};
      d.o = 0;
      if (d.ok) {
        const long long o = (((long long)nb * p.Ho + oh0 + (int)tr) * p.Wo + ow0 + (int)col) * p.C + c0 + gc * G;
        d.v = *(const u32x4*)(yptr + o);
        d.o = (uint32_t)o;
      }
      return d;
    };
    auto accumulate = [&](const Dy& d) __attribute__((always_inline)) {
      if (!d.ok) return;
      float yf[G], ys[KIND == 1 ? G : 1];
      uint32_t ws = 0;
      if constexpr (KIND == 1)
        ws = btx_sign_word(d.o >> 5, kout_a, kout_b) << ((int)((d.o >> 3) & 3) * 4 + (G == 4 ? (int)((d.o >> 2) & 1) * 2 : 0));
      if constexpr (G == 8) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          yf[2 * q] = u2f(d.v[q] << 16); yf[2 * q + 1] = u2f(d.v[q] & 0xffff0000u);
          if constexpr (KIND == 1) {
            const uint32_t y2 = d.v[q] ^ ((ws << q) & 0x80008000u);
            ys[2 * q] = u2f(y2 << 16); ys[2 * q + 1] = u2f(y2 & 0xffff0000u);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          yf[j] = u2f(d.v[j]);
          if constexpr (KIND == 1) {
            const int bit = ((j & 1) ? 31 : 15) - (j >> 1);
            ys[j] = u2f(d.v[j] ^ ((ws << (31 - bit)) & 0x80000000u));
          }
        }
      }
      const int prow = FORM ? d.tr * p.sh : d.tr, pcol = d.col * p.sw;
#pragma unroll
      for (int kh = 0; kh < NKH; ++kh)
#pragma unroll
        for (int kw = 0; kw < NKW; ++kw) {
          if (FORM == 0 && kw >= p.KW) continue;  // uniform
          const int t = kh * NKW + kw;
          const int pix = (prow + kh) * PW + pcol + (FORM ? kw : kw * p.dw);
          const u32x4 a = *(const u32x4*)(patch + pix * PIXB + gc * 16);
          if constexpr (G == 8) {
            uint32_t e = 0;
            if constexpr (KIND == 1) { const uint32_t sb = sgn[pix * NGC + gc]; e = ((sb & 0xFu) << 12) | ((sb & 0xF0u) << 24); }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              am[t][2 * q] = __builtin_fmaf(u2f(a[q] << 16), yf[2 * q], am[t][2 * q]);
              am[t][2 * q + 1] = __builtin_fmaf(u2f(a[q] & 0xffff0000u), yf[2 * q + 1], am[t][2 * q + 1]);
              if constexpr (KIND == 1) {
                const uint32_t a2 = a[q] ^ ((e << q) & 0x80008000u);
                ad[t][2 * q] = __builtin_fmaf(u2f(a2 << 16), ys[2 * q], ad[t][2 * q]);
                ad[t][2 * q + 1] = __builtin_fmaf(u2f(a2 & 0xffff0000u), ys[2 * q + 1], ad[t][2 * q + 1]);
              }
            }
          } else {
            uint32_t sb = 0;
            if constexpr (KIND == 1) sb = sgn[pix * NGC + gc];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              am[t][j] = __builtin_fmaf(u2f(a[j]), yf[j], am[t][j]);
              if constexpr (KIND == 1) {
                const int sft = (j == 0) ? 30 : (j == 1) ? 28 : (j == 2) ? 31 : 29;  // byte bits 1, 3, 0, 2 hold elements 0, 1, 2, 3
                ad[t][j] = __builtin_fmaf(u2f(a[j] ^ ((sb << sft) & 0x80000000u)), ys[j], ad[t][j]);
              }
            }
          }
        }
    };
    Dy d0 = fetch(slot), d1 = fetch(slot + SLOTS);
    for (int i = slot; i < npx; i += SLOTS) {
      const Dy d2 = fetch(i + 2 * SLOTS);
      accumulate(d0);
      d0 = d1; d1 = d2;
    }
  }

  // ---- the slots of a granule, in slot order, RT taps per round through LDS (the patch is dead); then one plain store of the block
  float* red = (float*)smem;               // [RT][SLOTS][64]
  float* fin = red + RT * SLOTS * DW_CB;   // [nk][NT][64]
  auto reduce_set = [&](const float (&acc)[NT][G], int which) __attribute__((always_inline)) {
#pragma unroll
    for (int r0 = 0; r0 < NT; r0 += RT) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        if (r0 + q < NT) {
#pragma unroll
          for (int i = 0; i < G / 4; ++i)
            *(f32x4*)(red + (q * SLOTS + slot) * DW_CB + gc * G + 4 * i) =
                (f32x4){acc[r0 + q][4 * i], acc[r0 + q][4 * i + 1], acc[r0 + q][4 * i + 2], acc[r0 + q][4 * i + 3]};
        }
      }
      __syncthreads();
      const int q = tid >> 6, c = tid & 63;
      if (r0 + q < NT) {
        float s = red[(q * SLOTS) * DW_CB + c];
        for (int k = 1; k < SLOTS; ++k) s += red[(q * SLOTS + k) * DW_CB + c];
        fin[(which * NT + r0 + q) * DW_CB + c] = s;
      }
    }
  };
  reduce_set(am, 0);
  if constexpr (KIND == 1) reduce_set(ad, 1);
  __syncthreads();
  const int ntw = FORM ? 9 : p.KW, t0 = FORM ? 0 : kh0 * p.KW;  // the taps this workgroup owns: t0 .. t0 + ntw - 1
  const size_t E = (size_t)p.C * p.T;
#pragma unroll
  for (int which = 0; which < (KIND == 1 ? 2 : 1); ++which) {
    float* dst = p.direct ? (which ? p.out_d : p.out_m) : p.slab + ((size_t)slab * (KIND == 1 ? 2 : 1) + which) * E;
    for (int i = tid; i < nch * ntw; i += DW_THREADS) {
      const int c = i / ntw, tl = i - c * ntw;
      dst[(size_t)(c0 + c) * p.T + t0 + tl] = fin[(which * NT + tl) * DW_CB + c];
    }
  }
}

template <typename ACT>
static int launch_dw_wgrad_impl(int kind, int form, const DwWgradParams& p, int nwg, int lds, hipStream_t st) {
#define BTX_LAUNCH_DWW(KIND, FORM)                                                                                    \
  do {                                                                                                                \
    auto kfn = dw_wgrad_kernel<ACT, KIND, FORM>;                                                                      \
    static bool attr_done = false;                                                                                    \
    if (!attr_done) {                                                                                                 \
      hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, DWW_LDS_CAP);  \
      if (e != hipSuccess) return (int)e;                                                                             \
      attr_done = true;                                                                                               \
    }                                                                                                                 \
    hipLaunchKernelGGL(kfn, dim3(nwg), dim3(DW_THREADS), lds, st, p);                                                 \
  } while (0)
  if (kind == 0) { if (form) BTX_LAUNCH_DWW(0, 1); else BTX_LAUNCH_DWW(0, 0); }
  else           { if (form) BTX_LAUNCH_DWW(1, 1); else BTX_LAUNCH_DWW(1, 0); }
#undef BTX_LAUNCH_DWW
  return (int)hipGetLastError();
}

}  // namespace btx
