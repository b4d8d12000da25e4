// btx_attn.hip — fused multi-head attention forward for gfx950 (include/btx_attn.h).
//
// One workgroup of four waves per (row, head, tile of BQ = 128 queries); wave w owns queries 32w .. 32w+31 of the tile.  The key
// axis is walked in tiles of BK keys (64 under bf16, 32 under f32) with the online-softmax recurrence, so no score ever reaches
// memory.  Both contractions are computed TRANSPOSED, which keeps every per-query quantity inside one lane pair:
//
//   S^T = K Q^T      A = K fragment from LDS (M = 32 keys), B = Q fragment held in registers for the whole key loop (N = 32 queries).
//                    In the 32x32 accumulator layout lane (j = lane % 32, h = lane / 32) then holds query column j and the 16 keys
//                    8*(r/4) + 4h + r%4, r = 0..15, of each 32-key block: the row maximum and the row sum are an in-lane reduction
//                    plus one exchange between the two half-waves, and the running m, l, alpha are per-lane scalars.
//   O^T += V^T P^T   A = V^T fragment from LDS (M = 32 head channels), B = P^T straight from the S accumulator registers: the k slot
//                    (h, e) of MFMA step s is key 16s + 8*(e/4) + 4h + e%4 — exactly the keys the lane already holds in registers
//                    8s .. 8s+7 — and the V^T fragment is read from LDS in that same permuted key order (two 8-byte reads), so P
//                    never makes a round trip through LDS.  The O^T accumulator has the lane's own query as its column, so alpha
//                    rescales it in place and the final 1/l needs no exchange.
//
// LDS, two stages (tile t+1 is fetched from global memory into registers before tile t is computed and written into the other
// stage after it: one barrier per tile):
//   K   [BK][D] row-major in the operand type (bf16: rounded once on the way in; f32), rows padded by 16 bytes
//   V   bf16: V^T [D][BK], two keys per dword, rows padded to 136 bytes — the transposition happens once per tile on the write
//       side, shared by the four waves;  f32: [BK][D] row-major like K (the 32x32x2 MFMA takes one f32 per lane and step)
//   flags [BK] bytes: key masked (key >= Tk or key_pad)
// Rows of masked keys are written as zeros (never multiplied, whatever bits they hold), keys and queries past the end are not read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/btx_attn_bias.h"
#include "btx_attn_tile.h"

namespace {

constexpr int NT = 256, BQ = 128;
constexpr float NEG_INF = -__builtin_huge_valf();

struct AttnArgs {
  const void *q, *k, *v;
  void* out;
  const uint8_t* pad;
  int64_t s[8];  // element strides (row, token) of q, k, v, out
  int Tq, Tk, heads, pad_rows, causal, nqt;
  float c;       // scale * log2(e): the softmax runs in base 2
  uint32_t vec;  // bit x: tensor x (q, k, v, out) sits on the 16-byte grid
  float* lse;    // [rows][heads][Tq], the training forward only (btx_attn_fwd_train)
};
struct AttnBiasArgs : AttnArgs {
  BiasOp b;  // the BIAS instantiations only: the kernel argument of the others is AttnArgs as it was
};

// LSE: the training forward — the same kernel, and each query also stores L = m + log2(l), the base-2 log-sum-exp of its scaled
// scores (+inf for a query whose keys are all masked: every probability exp2(c s - L) the backward recomputes is then 0)
//
// BIAS (include/btx_attn_bias.h): the score becomes fma(s, c, b log2 e) with b = bias[row % rows][head][query][key].
// Lane (l31, h) holds four consecutive keys of its own query per group g: one 16 / 8 / 4-byte load per group, every element used by
// one lane once, so the bias goes from global memory to registers (no LDS).  Tile t+1's is requested as soon as the scores of tile t
// have consumed tile t's (ONE register set): the loads fly under the P V MFMAs, the barrier and the next tile's S MFMAs.  A query
// stride of 0 (key-only bias) makes the 32 lanes of a half-wave read the same address: one transaction.
template <int ACT, int PREC, int D, bool LSE, bool BIAS>
__global__ __launch_bounds__(NT) void attn_fwd_kernel(const typename std::conditional<BIAS, AttnBiasArgs, AttnArgs>::type a) {
  constexpr bool BF = PREC == BTX_PREC_BF16;
  constexpr int BK = BF ? 64 : 32, NKB = BK / 32;  // keys per tile, 32-key MFMA blocks per tile
  constexpr int ESZ = BF ? 2 : 4, EPU = 16 / ESZ;  // operand bytes, elements per 16-byte unit
  constexpr int UPR = D / EPU, NU = D / 32;        // units per row; row-major units per thread and tile (BK * UPR == NU * NT)
  constexpr int NDC = D / 32;                      // 32-channel blocks of the output
  constexpr int KROW = D * ESZ + 16, K_BYTES = BK * KROW;
  constexpr int VROW = BF ? BK * 2 + 8 : KROW, V_BYTES = BF ? D * VROW : BK * VROW;
  constexpr int VT_UNITS = (BK / 2) * (D / 8), NUV = (VT_UNITS + NT - 1) / NT;  // bf16 V: (key pair, 8 channels) units
  constexpr int STAGE = K_BYTES + V_BYTES + BK;
  static_assert(BK * UPR == NU * NT && STAGE % 16 == 0, "tile plan");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % a.nqt, rh = blockIdx.x / a.nqt, head = rh % a.heads, row = rh / a.heads;
  const int Tq = a.Tq, Tk = a.Tk;
  const bool vq = a.vec & 1, vk = a.vec & 2, vv = a.vec & 4, vo = a.vec & 8;
  const uint8_t* pad = a.pad ? a.pad + (int64_t)(row % a.pad_rows) * Tk : nullptr;
  const int64_t kbase = (int64_t)row * a.s[2] + (int64_t)head * D, vbase = (int64_t)row * a.s[4] + (int64_t)head * D;

  // ---- Q fragments: the B operand of S^T = K Q^T, in registers for the whole key loop -------------------------------------------
  const int wq0 = qt * BQ + wave * 32, qidx = wq0 + l31;
  const bool qok = qidx < Tq;
  constexpr int NQF = BF ? D / 16 : D / 8;
  u32x4 qf[NQF];
  {
    const int64_t qoff = (int64_t)row * a.s[0] + (int64_t)qidx * a.s[1] + (int64_t)head * D;
#pragma unroll
    for (int i = 0; i < NQF; ++i) {
      float f[EPU];
#pragma unroll
      for (int e = 0; e < EPU; ++e) f[e] = 0.f;
      // bf16: MFMA step i contracts channels 16i + 8h + 0..7; f32: steps 4i .. 4i+3 contract channel 8i + 4h + e in slot h
      if (qok) load_elems<ACT, EPU>(a.q, qoff + (BF ? 16 * i + 8 * h : 8 * i + 4 * h), vq, f);
      qf[i] = pack_unit<PREC>(f);
    }
  }

  int nkt = (Tk + BK - 1) / BK;
  if (a.causal) nkt = min(nkt, (qt * BQ + BQ - 1) / BK + 1);  // key tiles entirely above the diagonal are never visited

  // ---- staging registers of the next tile ---------------------------------------------------------------------------------------
  u32x4 kreg[NU], vreg[BF ? 2 * NUV : NU];
  uint32_t flag = 0;
  auto masked = [&](int key) -> bool { return key >= Tk || (pad && pad[key]); };
  auto fetch = [&](int t) {
    const int k0 = t * BK;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * NT, key = k0 + u / UPR, c = u % UPR;
      float f[EPU];
#pragma unroll
      for (int e = 0; e < EPU; ++e) f[e] = 0.f;
      const bool ok = !masked(key);
      if (ok) load_elems<ACT, EPU>(a.k, kbase + (int64_t)key * a.s[3] + c * EPU, vk, f);
      kreg[i] = pack_unit<PREC>(f);
      if constexpr (!BF) {
#pragma unroll
        for (int e = 0; e < EPU; ++e) f[e] = 0.f;
        if (ok) load_elems<ACT, EPU>(a.v, vbase + (int64_t)key * a.s[5] + c * EPU, vv, f);
        vreg[i] = pack_unit<PREC>(f);
      }
    }
    if constexpr (BF) {
#pragma unroll
      for (int i = 0; i < NUV; ++i) {
        const int u = tid + i * NT;
        float f0[8], f1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f0[e] = f1[e] = 0.f;
        if (u < VT_UNITS) {
          const int key = k0 + 2 * (u / (D / 8)), c = u % (D / 8);
          if (!masked(key)) load_elems<ACT, 8>(a.v, vbase + (int64_t)key * a.s[5] + c * 8, vv, f0);
          if (!masked(key + 1)) load_elems<ACT, 8>(a.v, vbase + (int64_t)(key + 1) * a.s[5] + c * 8, vv, f1);
        }
        // dword e: channel 8c + e of the key pair (even key in the low half)
        vreg[2 * i] = (u32x4){pk_bf16(f0[0], f1[0]), pk_bf16(f0[1], f1[1]), pk_bf16(f0[2], f1[2]), pk_bf16(f0[3], f1[3])};
        vreg[2 * i + 1] = (u32x4){pk_bf16(f0[4], f1[4]), pk_bf16(f0[5], f1[5]), pk_bf16(f0[6], f1[6]), pk_bf16(f0[7], f1[7])};
      }
    }
    if (tid < BK) flag = masked(k0 + tid) ? 1u : 0u;
  };
  auto stash = [&](int stage) {
    unsigned char* Ks = lds + stage * STAGE;
    unsigned char* Vs = Ks + K_BYTES;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = tid + i * NT, key = u / UPR, c = u % UPR;
      *(u32x4*)(Ks + key * KROW + c * 16) = kreg[i];
      if constexpr (!BF) *(u32x4*)(Vs + key * VROW + c * 16) = vreg[i];
    }
    if constexpr (BF) {
#pragma unroll
      for (int i = 0; i < NUV; ++i) {
        const int u = tid + i * NT;
        if (u < VT_UNITS) {
          const int p = u / (D / 8), c = u % (D / 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) *(uint32_t*)(Vs + (8 * c + e) * VROW + p * 4) = vreg[2 * i + (e >> 2)][e & 3];
        }
      }
    }
    if (tid < BK) Vs[V_BYTES + tid] = (unsigned char)flag;
  };

  // ---- BIAS: the lane's bias of the next tile, [32-key block][group][key of the group]; elements past Tq / Tk are not read -------
  constexpr int NBB = BIAS ? NKB * 16 : 1;
  float bb[NBB];
  if constexpr (BIAS) {  // a lane without a query never loads: its (unstored) column computes on zeros
#pragma unroll
    for (int i = 0; i < NBB; ++i) bb[i] = 0.f;
  }
  [[maybe_unused]] int64_t boff = 0;
  if constexpr (BIAS) boff = (int64_t)(row % a.b.rows) * a.b.s[0] + (int64_t)head * a.b.s[1] + (int64_t)qidx * a.b.s[2];
  auto fetch_bias = [&](int t) {
    if constexpr (BIAS) {
      const int k0 = t * BK;
      if (!qok || (a.causal && k0 > wq0 + 31)) return;  // no query, or a tile the wave skips
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int key = k0 + kb * 32 + 8 * g + 4 * h;
          float f[4] = {0.f, 0.f, 0.f, 0.f};
          if (key < Tk) load_bias4(a.b, boff + key, min(4, Tk - key), f);
#pragma unroll
          for (int e = 0; e < 4; ++e) bb[kb * 16 + 4 * g + e] = f[e];
        }
    }
  };

  // ---- the key loop -------------------------------------------------------------------------------------------------------------
  f32x16 o[NDC];
#pragma unroll
  for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dc][r] = 0.f;
  float m_run = NEG_INF, l_run = 0.f;  // running maximum (base-2 scores) and this lane's half of the running sum

  fetch(0);
  stash(0);
  fetch_bias(0);
  __syncthreads();
  for (int t = 0; t < nkt; ++t) {
    const int k0 = t * BK;
    if (t + 1 < nkt) fetch(t + 1);
    const unsigned char* Ks = lds + (t & 1) * STAGE;
    const unsigned char* Vs = Ks + K_BYTES;
    if (wq0 < Tq && !(a.causal && k0 > wq0 + 31)) {  // the wave has queries, and the tile is not entirely above its diagonal
      f32x16 s[NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
        const unsigned char* kr = Ks + (kb * 32 + l31) * KROW;
#pragma unroll
        for (int i = 0; i < NQF; ++i) {
          if constexpr (BF) {
            const u32x4 kf = *(const u32x4*)(kr + (16 * i + 8 * h) * 2);
            s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf), __builtin_bit_cast(bf16x8, qf[i]), s[kb], 0, 0, 0);
          } else {
            const u32x4 kf = *(const u32x4*)(kr + (8 * i + 4 * h) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(u2f(kf[e]), u2f(qf[i][e]), s[kb], 0, 0, 0);
          }
        }
      }
      // scores in base 2, masks as a select (never arithmetic on a masked score), tile maximum
      const bool need_mask = k0 + BK > Tk || pad != nullptr || (a.causal && k0 + BK - 1 > wq0);
      float mx = NEG_INF;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kk = kb * 32 + 8 * g + 4 * h;  // the lane's keys kk .. kk+3 of this tile
          uint32_t fw = 0;
          if (need_mask) fw = *(const uint32_t*)(Vs + V_BYTES + kk);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v;
            if constexpr (BIAS) v = __builtin_fmaf(s[kb][4 * g + e], a.c, bb[kb * 16 + 4 * g + e] * BIAS_LOG2E);
            else v = s[kb][4 * g + e] * a.c;
            if (need_mask && (((fw >> (8 * e)) & 0xffu) || (a.causal && k0 + kk + e > qidx))) v = NEG_INF;
            s[kb][4 * g + e] = v;
            mx = fmaxf(mx, v);
          }
        }
      if (t + 1 < nkt) fetch_bias(t + 1);  // bb is consumed: the next tile's loads fly under the P V MFMAs and the next K / V fetch
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      const float m_use = m_new == NEG_INF ? 0.f : m_new;  // every key so far masked: p = exp2(-inf) = 0, alpha = 0
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      float ps = 0.f;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(s[kb][r] - m_use);
          s[kb][r] = p;
          ps += p;
        }
      l_run = l_run * alpha + ps;
      m_run = m_new;
#pragma unroll
      for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dc][r] *= alpha;
      // O^T += V^T P^T
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if constexpr (BF) {
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            const u32x4 pb = {pk_bf16(s[kb][8 * st], s[kb][8 * st + 1]), pk_bf16(s[kb][8 * st + 2], s[kb][8 * st + 3]),
                              pk_bf16(s[kb][8 * st + 4], s[kb][8 * st + 5]), pk_bf16(s[kb][8 * st + 6], s[kb][8 * st + 7])};
#pragma unroll
            for (int dc = 0; dc < NDC; ++dc) {
              const unsigned char* vp = Vs + (dc * 32 + l31) * VROW + (kb * 32 + 16 * st + 4 * h) * 2;
              const u32x2 lo = *(const u32x2*)vp, hi = *(const u32x2*)(vp + 16);
              const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
              o[dc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), __builtin_bit_cast(bf16x8, pb), o[dc], 0, 0, 0);
            }
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
#pragma unroll
            for (int dc = 0; dc < NDC; ++dc) {
              const float vf = *(const float*)(Vs + key * VROW + (dc * 32 + l31) * 4);
              o[dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf, s[kb][r], o[dc], 0, 0, 0);
            }
          }
        }
      }
    }
    if (t + 1 < nkt) stash((t + 1) & 1);
    __syncthreads();
  }

  // ---- out = O / l; a query with every key masked stores zeros -------------------------------------------------------------------
  const float l = l_run + __shfl_xor(l_run, 32);
  if (!qok) return;
  if constexpr (LSE) {
    if (h == 0) a.lse[((int64_t)row * a.heads + head) * Tq + qidx] = l > 0.f ? m_run + log2f(l) : __builtin_huge_valf();
  }
  const float inv = 1.0f / l;
  const int64_t ooff = (int64_t)row * a.s[6] + (int64_t)qidx * a.s[7] + (int64_t)head * D;
#pragma unroll
  for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float r4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r4[e] = l > 0.f ? o[dc][4 * g + e] * inv : 0.f;
      store4<ACT>(a.out, ooff + dc * 32 + 8 * g + 4 * h, vo, r4);
    }
}

template <int ACT, int PREC, bool LSE, bool BIAS>
hipError_t launch_d(const AttnBiasArgs& a, int D, uint32_t grid, hipStream_t st) {
  switch (D) {
    case 32: hipLaunchKernelGGL((attn_fwd_kernel<ACT, PREC, 32, LSE, BIAS>), dim3(grid), dim3(NT), 0, st, a); break;
    case 64: hipLaunchKernelGGL((attn_fwd_kernel<ACT, PREC, 64, LSE, BIAS>), dim3(grid), dim3(NT), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_fwd_kernel<ACT, PREC, 128, LSE, BIAS>), dim3(grid), dim3(NT), 0, st, a); break;
  }
  return hipGetLastError();
}

template <bool LSE, bool BIAS>
hipError_t launch_p(const AttnBiasArgs& a, int D, int act_dtype, int prec, uint32_t grid, hipStream_t st) {
  if (act_dtype == BTX_ACT_F32) return prec == BTX_PREC_F32 ? launch_d<BTX_ACT_F32, BTX_PREC_F32, LSE, BIAS>(a, D, grid, st)
                                                            : launch_d<BTX_ACT_F32, BTX_PREC_BF16, LSE, BIAS>(a, D, grid, st);
  return prec == BTX_PREC_F32 ? launch_d<BTX_ACT_BF16, BTX_PREC_F32, LSE, BIAS>(a, D, grid, st)
                              : launch_d<BTX_ACT_BF16, BTX_PREC_BF16, LSE, BIAS>(a, D, grid, st);
}

// the argument checks and the launch of all four entry points; lse == nullptr: the inference kernel; bias == nullptr: no bias (the
// kernel without the BIAS flag, whose argument is the AttnArgs part of `a`)
template <bool LSE>
int attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int rows, int Tq, int Tk, int heads, int D,
             const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype, int prec,
             void* stream, const void* bias = nullptr, int bias_dtype = 0, int bias_rows = 1, const int64_t* bias_strides = nullptr) {
  if (!q || !k || !v || !out || !strides) return BTX_E_NULL;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;  // f32 and bf16 forms only
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16) return BTX_E_DTYPE;
  if (rows <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || D <= 0 || (causal != 0 && causal != 1)) return BTX_E_SHAPE;
  if (key_pad && pad_rows <= 0) return BTX_E_SHAPE;
  if (D != 32 && D != 64 && D != 128) return BTX_E_UNSUPPORTED;
  const uint64_t nqt = ((uint64_t)Tq + BQ - 1) / BQ, grid = nqt * (uint64_t)heads * (uint64_t)rows;
  if (grid > 0x7fffffffull) return BTX_E_UNSUPPORTED;
  if (LSE && (uintptr_t)lse % 4) return BTX_E_ALIGN;
  AttnBiasArgs a = {};
  if (bias) {
    const int rc = bias_operand(bias, bias_dtype, bias_rows, bias_strides, a.b);
    if (rc) return rc;
  }
  a.lse = lse;
  a.q = q; a.k = k; a.v = v; a.out = out; a.pad = key_pad;
  const uintptr_t base[4] = {(uintptr_t)q, (uintptr_t)k, (uintptr_t)v, (uintptr_t)out};
  const int64_t esz = act_dtype == BTX_ACT_F32 ? 4 : 2;
  for (int x = 0; x < 4; ++x) {
    a.s[2 * x] = strides[2 * x];
    a.s[2 * x + 1] = strides[2 * x + 1];
    if (base[x] % esz) return BTX_E_ALIGN;  // below the element's own alignment
    if (base[x] % 16 == 0 && (strides[2 * x] * esz) % 16 == 0 && (strides[2 * x + 1] * esz) % 16 == 0) a.vec |= 1u << x;
  }
  a.Tq = Tq; a.Tk = Tk; a.heads = heads; a.pad_rows = key_pad ? pad_rows : 1; a.causal = causal; a.nqt = (int)nqt;
  a.c = scale * 1.44269504088896340736f;
  hipStream_t st = (hipStream_t)stream;
  return (int)(bias ? launch_p<LSE, true>(a, D, act_dtype, prec, (uint32_t)grid, st)
                    : launch_p<LSE, false>(a, D, act_dtype, prec, (uint32_t)grid, st));
}

}  // namespace

extern "C" int btx_attn_fwd(const void* q, const void* k, const void* v, void* out, int rows, int Tq, int Tk, int heads, int D,
                            const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype,
                            int prec, void* stream) {
  return attn_fwd<false>(q, k, v, out, nullptr, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale, act_dtype, prec, stream);
}

extern "C" int btx_attn_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int rows, int Tq, int Tk,
                                  int heads, int D, const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal,
                                  float scale, int act_dtype, int prec, void* stream) {
  if (!lse) return BTX_E_NULL;
  return attn_fwd<true>(q, k, v, out, lse, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale, act_dtype, prec, stream);
}

extern "C" int btx_attn_bias_fwd(const void* q, const void* k, const void* v, void* out, int rows, int Tq, int Tk, int heads, int D,
                                 const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale,
                                 int act_dtype, int prec, void* stream, const void* bias, int bias_dtype, int bias_rows,
                                 const int64_t bias_strides[3]) {
  return attn_fwd<false>(q, k, v, out, nullptr, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale, act_dtype, prec, stream,
                         bias, bias_dtype, bias_rows, bias_strides);
}

extern "C" int btx_attn_bias_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int rows, int Tq, int Tk,
                                       int heads, int D, const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal,
                                       float scale, int act_dtype, int prec, void* stream, const void* bias, int bias_dtype,
                                       int bias_rows, const int64_t bias_strides[3]) {
  if (!lse) return BTX_E_NULL;
  return attn_fwd<true>(q, k, v, out, lse, rows, Tq, Tk, heads, D, strides, key_pad, pad_rows, causal, scale, act_dtype, prec, stream,
                        bias, bias_dtype, bias_rows, bias_strides);
}

