// btx_attn_bwd.hip — flash-attention backward for gfx950 (include/btx_attn_train.h).
//
// Two passes of ONE kernel template, launched one after the other on the stream.  Each pass gives one side of the score matrix to the
// lanes (the OWN side: 128 tokens per workgroup, 32 per wave, one per lane pair (l31, h)) and walks the other side (the STREAMED side)
// in tiles of BS tokens through LDS — the forward's structure, with every contraction computed transposed so that the own token is
// the accumulator column:
//
//                 own      streamed   R1 / R2 in LDS (row-major)   accumulators
//   dQ pass       queries  keys       K / V                        dQ^T += K^T dS^T
//   dK/dV pass    keys     queries    Q / dO                       dK^T += Q^T dS,   dV^T += dO^T P
//
//   S^T  = R1 own1^T   A = R1 fragment from LDS (M = 32 streamed tokens), B = the own fragment (q | k) in registers for the whole loop
//   dP^T = R2 own2^T   the same with R2 and the second own fragment (dO | v)
//          lane (l31, h) then holds, of each 32-token block, the streamed tokens 8*(r/4) + 4h + r%4 (r = 0..15) of its own token:
//          P = exp2(c S - L) (0 by select where masked) and dS = P (dP - delta) are formed in place in those registers.
//   acc += T^T B       A = the TRANSPOSED streamed tile [D][BS] (M = 32 head channels), B = dS (or P) straight from the registers, as the
//          forward takes P: k slot (h, e) of MFMA step s is streamed token 16s + 8*(e/4) + 4h + e%4.
// L and delta belong to the query: per-lane scalars in the dQ pass (delta = dO . O is computed in its prologue from the lane's own
// channels plus one exchange between the half-waves, and stored for the second pass), per accumulator row in the dK/dV pass (read from
// LDS, 16 bytes per four queries).  Under `causal` the dQ pass stops at the diagonal and the dK/dV pass starts at it.
//
// LDS, two stages (tile t+1 is fetched from global memory into registers before tile t is computed and written into the other stage
// after it: one barrier per tile):
//   R1, R2 [BS][D] row-major in the operand type (bf16: rounded once on the way in), rows padded by 16 bytes
//   T1     bf16 only: R1 transposed, [D][BS] bf16, rows padded by 8 bytes; written from the same staging registers with 2-byte stores.
//   T2     bf16, dK/dV pass only: R2 transposed.  (f32: the 32x32x2 MFMA takes one f32 per lane and step, read from R1 / R2.)
//   aux    dQ pass: [BS] bytes, key masked (key >= Tk or key_pad);  dK/dV pass: L [BS] f32 (+inf past Tq), delta [BS] f32
// BS = 64 under bf16 with D <= 64, 32 otherwise (D = 128 would not hold S, dP and two accumulator sets in registers at 64).
// Rows of masked keys and of tokens past the end are written as zeros and never read from memory; nothing is stored past the end.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/btx_attn_bias.h"
#include "btx_attn_tile.h"

namespace {

constexpr int NT = 256, BO = 128;
constexpr float INF = __builtin_huge_valf();
enum { X_Q, X_K, X_V, X_O, X_DO, X_DQ, X_DK, X_DV };

struct BwdArgs {
  const void* in[5];  // q, k, v, out, d_out
  void* g[3];         // dq, dk, dv
  const float* lse;
  float* delta;
  const uint8_t* pad;
  int64_t s[16];      // element strides (row, token) of the eight tensors
  int Tq, Tk, heads, pad_rows, causal, not_;  // not_: own tiles per (row, head)
  float c, scale;     // scale * log2(e); scale
  uint32_t vec;       // bit x: tensor x sits on the 16-byte grid
};

struct BwdBiasArgs : BwdArgs {
  BiasOp b;  // the BIAS instantiations only: the kernel argument of the others is BwdArgs as it was
};

// BIAS (include/btx_attn_bias.h): P = exp2(fma(S, c, b log2 e) - L), b = bias[row % rows][head][query][key].
//   dQ pass     the lane's four consecutive streamed tokens are four consecutive KEYS of its own query: one 16 / 8 / 4-byte load per
//               group straight into registers, as in the forward (requested when the previous tile's have been consumed)
//   dK/dV pass  they are four consecutive QUERIES of its own key — four strided reads.  The [BS queries][128 own keys] tile goes through
//               LDS instead: read from global memory along the key axis (thread u: query u / 32, keys 4 (u % 32) .. +3, coalesced) with
//               the K / V fetch, stored as f32 rows of 128 + 8 words behind L and delta in `aux`, read per accumulator entry as one
//               word at [query][own key].  A wave's 64 lanes read keys l31 of query rows kk + e and kk + e + 4 (h): 4 * 136 words = 32
//               banks apart, so the 64 words fall on 64 different banks.
constexpr int BROW = (BO + 8) * 4;

template <int ACT, int PREC, int D, bool KV, bool BIAS>
__global__ __launch_bounds__(NT) void attn_bwd_kernel(const typename std::conditional<BIAS, BwdBiasArgs, BwdArgs>::type a) {
  constexpr bool BF = PREC == BTX_PREC_BF16;
  constexpr int BS = (BF && D <= 64) ? 64 : 32, NSB = BS / 32;  // streamed tokens per tile, 32-token MFMA blocks per tile
  constexpr int ESZ = BF ? 2 : 4, EPU = 16 / ESZ;               // operand bytes, elements per 16-byte unit
  constexpr int UPR = D / EPU, NU = BS * UPR / NT;              // units per row; units per thread, tile and tensor
  constexpr int NDC = D / 32, NF = BF ? D / 16 : D / 8;         // 32-channel blocks; 16-byte units of an own fragment
  constexpr int RROW = D * ESZ + 16, R_BYTES = BS * RROW;
  constexpr int TROW = BS * 2 + 8, T_BYTES = BF ? D * TROW : 0, NTR = KV ? 2 : 1;
  constexpr int B_BYTES = (KV && BIAS) ? BS * BROW : 0, NG = BS * 32 / NT;  // the bias tile; its four-key groups per thread
  constexpr int AUX = KV ? BS * 8 + B_BYTES : BS;
  // the f32 D = 128 dK/dV pass has no registers left to hold a next tile across the MFMAs once the bias is added (492 of 512
  // without it; the compiler spills): it fetches tile t+1 after the MFMAs of tile t, right before it writes it, and pays that
  // latency once per tile (section 32.3)
  constexpr bool LATE = KV && BIAS && !BF && D == 128;
  constexpr int STAGE = 2 * R_BYTES + NTR * T_BYTES + AUX;
  constexpr int XO1 = KV ? X_K : X_Q, XO2 = KV ? X_V : X_DO, XS1 = KV ? X_Q : X_K, XS2 = KV ? X_DO : X_V;
  static_assert(BS * UPR == NU * NT && STAGE % 16 == 0, "tile plan");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int ot = blockIdx.x % a.not_, rh = blockIdx.x / a.not_, head = rh % a.heads, row = rh / a.heads;
  const int Tq = a.Tq, Tk = a.Tk, To = KV ? Tk : Tq, Ts = KV ? Tq : Tk;
  const uint8_t* pad = a.pad ? a.pad + (int64_t)(row % a.pad_rows) * Tk : nullptr;
  const int64_t plane = ((int64_t)row * a.heads + head) * Tq;  // of lse and delta
  auto vec = [&](int x) -> bool { return (a.vec >> x) & 1; };
  auto at = [&](int x, int tok) -> int64_t { return (int64_t)row * a.s[2 * x] + (int64_t)tok * a.s[2 * x + 1] + (int64_t)head * D; };
  auto kmasked = [&](int key) -> bool { return key >= Tk || (pad && pad[key]); };

  // ---- the own fragments: B operands, in registers for the whole loop -----------------------------------------------------------
  const int w0 = ot * BO + wave * 32, oidx = w0 + l31;
  const bool ook = oidx < To;
  const bool oload = KV ? !kmasked(oidx) : ook;  // a masked key's rows are never read: zeros
  u32x4 f1[NF], f2[NF];
  float L_own = INF, d_own = 0.f;
  {
    const int64_t o1 = at(XO1, oidx), o2 = at(XO2, oidx), oo = at(X_O, oidx);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      float x1[EPU], x2[EPU];
#pragma unroll
      for (int e = 0; e < EPU; ++e) x1[e] = x2[e] = 0.f;
      // bf16: MFMA step i contracts channels 16i + 8h + 0..7; f32: steps 4i .. 4i+3 contract channel 8i + 4h + e in slot h
      const int ch = BF ? 16 * i + 8 * h : 8 * i + 4 * h;
      if (oload) {
        load_elems<ACT, EPU>(a.in[XO1], o1 + ch, vec(XO1), x1);
        load_elems<ACT, EPU>(a.in[XO2], o2 + ch, vec(XO2), x2);
      }
      f1[i] = pack_unit<PREC>(x1);
      f2[i] = pack_unit<PREC>(x2);
      if constexpr (!KV) {
        // delta = dO . O over the lane's half of the channels, in f32, from the dO the MFMAs see (bf16: the rounded one), so that
        // sum_j P_ij (dP_ij - delta_i) cancels as it does in exact arithmetic — a query with one visible key gets dS = 0
        if (oload) {
          float y[EPU];
          load_elems<ACT, EPU>(a.in[X_O], oo + ch, vec(X_O), y);
#pragma unroll
          for (int e = 0; e < EPU; ++e) {
            const float d = BF ? u2f(e & 1 ? f2[i][e >> 1] & 0xffff0000u : f2[i][e >> 1] << 16) : x2[e];
            d_own = __builtin_fmaf(d, y[e], d_own);
          }
        }
      }
    }
  }
  if constexpr (!KV) {
    d_own += __shfl_xor(d_own, 32);
    if (ook) {
      L_own = a.lse[plane + oidx];
      if (h == 0) a.delta[plane + oidx] = d_own;
    }
  }

  // streamed tiles [t0, t1): under `causal` the dQ pass stops at the diagonal, the dK/dV pass starts at it
  int t0 = 0, t1 = (Ts + BS - 1) / BS;
  if (a.causal) {
    if constexpr (KV) t0 = ot * BO / BS;
    else t1 = min(t1, (ot * BO + BO - 1) / BS + 1);
  }

  // ---- staging registers of the next tile ---------------------------------------------------------------------------------------
  u32x4 r1[NU], r2[NU];
  float auxL = 0.f, auxD = 0.f;
  uint32_t flag = 0;
  f32x4 bst[(KV && BIAS) ? NG : 1];              // dK/dV pass: the thread's part of the next bias tile
  float bb[(!KV && BIAS) ? NSB * 16 : 1];  // dQ pass: the lane's bias of the next tile, [32-key block][group][key of the group]
  if constexpr (!KV && BIAS) {  // a lane without a query never loads: its (unstored) column computes on zeros
#pragma unroll
    for (int i = 0; i < NSB * 16; ++i) bb[i] = 0.f;
  }
  [[maybe_unused]] int64_t bbase = 0;
  if constexpr (BIAS) bbase = (int64_t)(row % a.b.rows) * a.b.s[0] + (int64_t)head * a.b.s[1];
  auto fetch_bias = [&](int t) {  // dQ pass; elements past Tq / Tk are not read
    if constexpr (!KV && BIAS) {
      const int s0 = t * BS;
      if (!ook || (a.causal && s0 > w0 + 31)) return;  // no query, or a tile the wave skips
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = s0 + sb * 32 + 8 * g + 4 * h;
          float f[4] = {0.f, 0.f, 0.f, 0.f};
          if (key < Tk) load_bias4(a.b, bbase + (int64_t)oidx * a.b.s[2] + key, min(4, Tk - key), f);
#pragma unroll
          for (int e = 0; e < 4; ++e) bb[sb * 16 + 4 * g + e] = f[e];
        }
    }
  };
  // dK/dV pass: group u of the bias tile at s0 — query s0 + u / 32, own keys 4 (u % 32) .. +3; elements past Tq / Tk are not read
  auto bias_group = [&](int s0, int u) -> f32x4 {
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KV && BIAS) {
      const int tok = s0 + (u >> 5), key = ot * BO + (u & 31) * 4;
      if (tok < Tq && key < Tk) load_bias4(a.b, bbase + (int64_t)tok * a.b.s[2] + key, min(4, Tk - key), f);
    }
    return (f32x4){f[0], f[1], f[2], f[3]};
  };
  auto fetch = [&](int t) {
    const int s0 = t * BS;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * NT, tok = s0 + u / UPR, cu = u % UPR;
      float x1[EPU], x2[EPU];
#pragma unroll
      for (int e = 0; e < EPU; ++e) x1[e] = x2[e] = 0.f;
      if (KV ? tok < Tq : !kmasked(tok)) {
        load_elems<ACT, EPU>(a.in[XS1], at(XS1, tok) + cu * EPU, vec(XS1), x1);
        load_elems<ACT, EPU>(a.in[XS2], at(XS2, tok) + cu * EPU, vec(XS2), x2);
      }
      r1[i] = pack_unit<PREC>(x1);
      r2[i] = pack_unit<PREC>(x2);
    }
    if constexpr (KV && BIAS) {
#pragma unroll
      for (int i = 0; i < NG; ++i) bst[i] = bias_group(s0, tid + i * NT);
    }
    if (tid < BS) {
      const int tok = s0 + tid;
      if constexpr (KV) {
        auxL = tok < Tq ? a.lse[plane + tok] : INF;
        auxD = tok < Tq ? a.delta[plane + tok] : 0.f;
      } else {
        flag = kmasked(tok) ? 1u : 0u;
      }
    }
  };
  auto stash = [&](int stage) {
    unsigned char* R1 = lds + stage * STAGE;
    unsigned char* R2 = R1 + R_BYTES;
    unsigned char* T1 = R2 + R_BYTES;
    unsigned char* T2 = T1 + T_BYTES;
    unsigned char* A = T1 + NTR * T_BYTES;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * NT, tok = u / UPR, cu = u % UPR;
      *(u32x4*)(R1 + tok * RROW + cu * 16) = r1[i];
      *(u32x4*)(R2 + tok * RROW + cu * 16) = r2[i];
      if constexpr (BF) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          *(uint16_t*)(T1 + (8 * cu + e) * TROW + tok * 2) = (uint16_t)(r1[i][e >> 1] >> (16 * (e & 1)));
          if constexpr (KV) *(uint16_t*)(T2 + (8 * cu + e) * TROW + tok * 2) = (uint16_t)(r2[i][e >> 1] >> (16 * (e & 1)));
        }
      }
    }
    if constexpr (KV && BIAS) {
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const int u = tid + i * NT;
        *(f32x4*)(A + BS * 8 + (u >> 5) * BROW + (u & 31) * 16) = bst[i];
      }
    }
    if (tid < BS) {
      if constexpr (KV) {
        *(float*)(A + tid * 4) = auxL;
        *(float*)(A + BS * 4 + tid * 4) = auxD;
      } else {
        A[tid] = (unsigned char)flag;
      }
    }
  };

  // ---- the loop over the streamed side ------------------------------------------------------------------------------------------
  f32x16 acc1[NDC], acc2[KV ? NDC : 1];  // dQ^T | dK^T (unscaled); dV^T
#pragma unroll
  for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc1[dc][r] = 0.f;
      if constexpr (KV) acc2[dc][r] = 0.f;
    }

  fetch(t0);
  stash(t0 & 1);
  if constexpr (BIAS) fetch_bias(t0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int s0 = t * BS;
    if constexpr (!LATE) {
      if (t + 1 < t1) fetch(t + 1);
    }
    const unsigned char* R1 = lds + (t & 1) * STAGE;
    const unsigned char* R2 = R1 + R_BYTES;
    const unsigned char* T1 = R2 + R_BYTES;
    const unsigned char* T2 = T1 + T_BYTES;
    const unsigned char* A = T1 + NTR * T_BYTES;
    // the wave has own tokens, and the tile is not entirely on the masked side of its diagonal
    const bool live = w0 < To && !(a.causal && (KV ? s0 + BS - 1 < w0 : s0 > w0 + 31));
    if (live) {
      f32x16 s[NSB], dp[NSB];
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[sb][r] = dp[sb][r] = 0.f;
        const unsigned char* p1 = R1 + (sb * 32 + l31) * RROW;
        const unsigned char* p2 = R2 + (sb * 32 + l31) * RROW;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          if constexpr (BF) {
            const u32x4 x1 = *(const u32x4*)(p1 + (16 * i + 8 * h) * 2), x2 = *(const u32x4*)(p2 + (16 * i + 8 * h) * 2);
            s[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x1), __builtin_bit_cast(bf16x8, f1[i]), s[sb], 0, 0, 0);
            dp[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x2), __builtin_bit_cast(bf16x8, f2[i]), dp[sb], 0, 0, 0);
          } else {
            const u32x4 x1 = *(const u32x4*)(p1 + (8 * i + 4 * h) * 4), x2 = *(const u32x4*)(p2 + (8 * i + 4 * h) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(x1[e]), u2f(f1[i][e]), s[sb], 0, 0, 0);
              dp[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(x2[e]), u2f(f2[i][e]), dp[sb], 0, 0, 0);
            }
          }
        }
      }
      // P = exp2(c S - L) and dS = P (dP - delta), in place; masks as a select (never arithmetic on a masked score)
      const bool need_mask = KV || s0 + BS > Tk || pad != nullptr || (a.causal && s0 + BS - 1 > w0);
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kk = sb * 32 + 8 * g + 4 * h;  // the lane's streamed tokens kk .. kk+3 of this tile
          float Lq[4], dq[4];
          uint32_t fw = 0;
          if constexpr (KV) {
            const f32x4 l4 = *(const f32x4*)(A + kk * 4), d4 = *(const f32x4*)(A + BS * 4 + kk * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { Lq[e] = l4[e]; dq[e] = d4[e]; }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { Lq[e] = L_own; dq[e] = d_own; }
            if (need_mask) fw = *(const uint32_t*)(A + kk);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int tok = s0 + kk + e;
            bool m;
            if constexpr (KV) m = !oload || (a.causal && oidx > tok);
            else m = need_mask && (((fw >> (8 * e)) & 0xffu) || (a.causal && tok > oidx));
            float p;
            if constexpr (BIAS) {
              float b;
              if constexpr (KV) b = *(const float*)(A + BS * 8 + (kk + e) * BROW + (wave * 32 + l31) * 4);
              else b = bb[sb * 16 + 4 * g + e];
              p = m ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(s[sb][4 * g + e], a.c, b * BIAS_LOG2E) - Lq[e]);
            } else {
              p = m ? 0.f : __builtin_amdgcn_exp2f(s[sb][4 * g + e] * a.c - Lq[e]);
            }
            s[sb][4 * g + e] = p;
            dp[sb][4 * g + e] = m ? 0.f : p * (dp[sb][4 * g + e] - dq[e]);
          }
        }
      if constexpr (BIAS)
        if (t + 1 < t1) fetch_bias(t + 1);  // bb is consumed: the next tile's loads fly under the MFMAs below and the next fetch
      // acc1 += T1^T dS;  dK/dV pass: acc2 += T2^T P
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        if constexpr (BF) {
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            const u32x4 db = {pk_bf16(dp[sb][8 * st], dp[sb][8 * st + 1]), pk_bf16(dp[sb][8 * st + 2], dp[sb][8 * st + 3]),
                              pk_bf16(dp[sb][8 * st + 4], dp[sb][8 * st + 5]), pk_bf16(dp[sb][8 * st + 6], dp[sb][8 * st + 7])};
            const u32x4 pb = {pk_bf16(s[sb][8 * st], s[sb][8 * st + 1]), pk_bf16(s[sb][8 * st + 2], s[sb][8 * st + 3]),
                              pk_bf16(s[sb][8 * st + 4], s[sb][8 * st + 5]), pk_bf16(s[sb][8 * st + 6], s[sb][8 * st + 7])};
#pragma unroll
            for (int dc = 0; dc < NDC; ++dc) {
              const int off = (dc * 32 + l31) * TROW + (sb * 32 + 16 * st + 4 * h) * 2;
              const u32x2 lo = *(const u32x2*)(T1 + off), hi = *(const u32x2*)(T1 + off + 16);
              const u32x4 x = {lo[0], lo[1], hi[0], hi[1]};
              acc1[dc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, db), acc1[dc], 0, 0, 0);
              if constexpr (KV) {
                const u32x2 lo2 = *(const u32x2*)(T2 + off), hi2 = *(const u32x2*)(T2 + off + 16);
                const u32x4 x2 = {lo2[0], lo2[1], hi2[0], hi2[1]};
                acc2[dc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x2), __builtin_bit_cast(bf16x8, pb), acc2[dc], 0, 0, 0);
              }
            }
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int tok = sb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
#pragma unroll
            for (int dc = 0; dc < NDC; ++dc) {
              const float x = *(const float*)(R1 + tok * RROW + (dc * 32 + l31) * 4);
              acc1[dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, dp[sb][r], acc1[dc], 0, 0, 0);
              if constexpr (KV) {
                const float x2 = *(const float*)(R2 + tok * RROW + (dc * 32 + l31) * 4);
                acc2[dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(x2, s[sb][r], acc2[dc], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    if constexpr (LATE) {
      if (t + 1 < t1) fetch(t + 1);
    }
    if (t + 1 < t1) stash((t + 1) & 1);
    __syncthreads();
  }

  // ---- every own token inside the tensor stores its gradient rows, zeros included ------------------------------------------------
  if (!ook) return;
  constexpr int XG1 = KV ? X_DK : X_DQ;
  const int64_t g1 = at(XG1, oidx), g2 = at(X_DV, oidx);
#pragma unroll
  for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float r4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r4[e] = acc1[dc][4 * g + e] * a.scale;
      store4<ACT>(a.g[XG1 - X_DQ], g1 + dc * 32 + 8 * g + 4 * h, vec(XG1), r4);
      if constexpr (KV) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r4[e] = acc2[dc][4 * g + e];
        store4<ACT>(a.g[2], g2 + dc * 32 + 8 * g + 4 * h, vec(X_DV), r4);
      }
    }
}

template <int ACT, int PREC, int D, bool BIAS>
hipError_t launch_passes(BwdBiasArgs a, uint32_t grid_q, uint32_t grid_k, int nqt, int nkt, hipStream_t st) {
  a.not_ = nqt;
  hipLaunchKernelGGL((attn_bwd_kernel<ACT, PREC, D, false, BIAS>), dim3(grid_q), dim3(NT), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  a.not_ = nkt;
  hipLaunchKernelGGL((attn_bwd_kernel<ACT, PREC, D, true, BIAS>), dim3(grid_k), dim3(NT), 0, st, a);
  return hipGetLastError();
}

template <int ACT, int PREC, bool BIAS>
hipError_t launch_d(const BwdBiasArgs& a, int D, uint32_t grid_q, uint32_t grid_k, int nqt, int nkt, hipStream_t st) {
  switch (D) {
    case 32: return launch_passes<ACT, PREC, 32, BIAS>(a, grid_q, grid_k, nqt, nkt, st);
    case 64: return launch_passes<ACT, PREC, 64, BIAS>(a, grid_q, grid_k, nqt, nkt, st);
    default: return launch_passes<ACT, PREC, 128, BIAS>(a, grid_q, grid_k, nqt, nkt, st);
  }
}

template <bool BIAS>
hipError_t launch_p(const BwdBiasArgs& a, int D, int act_dtype, int prec, uint32_t grid_q, uint32_t grid_k, int nqt, int nkt, hipStream_t st) {
  if (act_dtype == BTX_ACT_F32)
    return prec == BTX_PREC_F32 ? launch_d<BTX_ACT_F32, BTX_PREC_F32, BIAS>(a, D, grid_q, grid_k, nqt, nkt, st)
                                : launch_d<BTX_ACT_F32, BTX_PREC_BF16, BIAS>(a, D, grid_q, grid_k, nqt, nkt, st);
  return prec == BTX_PREC_F32 ? launch_d<BTX_ACT_BF16, BTX_PREC_F32, BIAS>(a, D, grid_q, grid_k, nqt, nkt, st)
                              : launch_d<BTX_ACT_BF16, BTX_PREC_BF16, BIAS>(a, D, grid_q, grid_k, nqt, nkt, st);
}

// the argument checks and the launches of both entry points; bias == nullptr: no bias (the kernels without the BIAS flag, whose
// argument is the BwdArgs part of `a`)
int attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out, const float* lse, float* delta, void* dq,
             void* dk, void* dv, int rows, int Tq, int Tk, int heads, int D, const int64_t strides[16], const uint8_t* key_pad,
             int pad_rows, int causal, float scale, int act_dtype, int prec, void* stream, const void* bias, int bias_dtype,
             int bias_rows, const int64_t* bias_strides) {
  if (!q || !k || !v || !out || !d_out || !lse || !delta || !dq || !dk || !dv || !strides) return BTX_E_NULL;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // f32 and bf16 forms only
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16) return BTX_E_DTYPE;
  if (rows <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || D <= 0 || (causal != 0 && causal != 1)) return BTX_E_SHAPE;
  if (key_pad && pad_rows <= 0) return BTX_E_SHAPE;
  if (D != 32 && D != 64 && D != 128) return BTX_E_UNSUPPORTED;
  const uint64_t nqt = ((uint64_t)Tq + BO - 1) / BO, nkt = ((uint64_t)Tk + BO - 1) / BO;
  const uint64_t grid_q = nqt * (uint64_t)heads * (uint64_t)rows, grid_k = nkt * (uint64_t)heads * (uint64_t)rows;
  if (grid_q > 0x7fffffffull || grid_k > 0x7fffffffull) return BTX_E_UNSUPPORTED;
  if ((uintptr_t)lse % 4 || (uintptr_t)delta % 4) return BTX_E_ALIGN;
  BwdBiasArgs a = {};
  if (bias) {
    const int rc = bias_operand(bias, bias_dtype, bias_rows, bias_strides, a.b);
    if (rc) return rc;
  }
  a.in[X_Q] = q; a.in[X_K] = k; a.in[X_V] = v; a.in[X_O] = out; a.in[X_DO] = d_out;
  a.g[0] = dq; a.g[1] = dk; a.g[2] = dv;
  a.lse = lse; a.delta = delta; a.pad = key_pad;
  const uintptr_t base[8] = {(uintptr_t)q, (uintptr_t)k, (uintptr_t)v, (uintptr_t)out, (uintptr_t)d_out, (uintptr_t)dq, (uintptr_t)dk, (uintptr_t)dv};
  const int64_t esz = act_dtype == BTX_ACT_F32 ? 4 : 2;
  for (int x = 0; x < 8; ++x) {
    a.s[2 * x] = strides[2 * x];
    a.s[2 * x + 1] = strides[2 * x + 1];
    if (base[x] % esz) return BTX_E_ALIGN;  // below the element's own alignment
    if (base[x] % 16 == 0 && (strides[2 * x] * esz) % 16 == 0 && (strides[2 * x + 1] * esz) % 16 == 0) a.vec |= 1u << x;
  }
  a.Tq = Tq; a.Tk = Tk; a.heads = heads; a.pad_rows = key_pad ? pad_rows : 1; a.causal = causal;
  a.c = scale * 1.44269504088896340736f;
  a.scale = scale;
  hipStream_t st = (hipStream_t)stream;
  return (int)(bias ? launch_p<true>(a, D, act_dtype, prec, (uint32_t)grid_q, (uint32_t)grid_k, (int)nqt, (int)nkt, st)
                    : launch_p<false>(a, D, act_dtype, prec, (uint32_t)grid_q, (uint32_t)grid_k, (int)nqt, (int)nkt, st));
}

}  // namespace

extern "C" int btx_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out, const float* lse,
                            float* delta, void* dq, void* dk, void* dv, int rows, int Tq, int Tk, int heads, int D,
                            const int64_t strides[16], const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype,
                            int prec, void* stream) {
  return attn_bwd(q, k, v, out, d_out, lse, delta, dq, dk, dv, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale,
                  act_dtype, prec, stream, nullptr, 0, 1, nullptr);
}

extern "C" int btx_attn_bias_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out, const float* lse,
                                 float* delta, void* dq, void* dk, void* dv, int rows, int Tq, int Tk, int heads, int D,
                                 const int64_t strides[16], const uint8_t* key_pad, int pad_rows, int causal, float scale,
                                 int act_dtype, int prec, void* stream, const void* bias, int bias_dtype, int bias_rows,
                                 const int64_t bias_strides[3]) {
  return attn_bwd(q, k, v, out, d_out, lse, delta, dq, dk, dv, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale,
                  act_dtype, prec, stream, bias, bias_dtype, bias_rows, bias_strides);
}

