// btx_contract_gemm8.h — pointwise Flipout contractions with a long K (1x1x1 convolutions without padding, any stride, and
// Linear layers, K >= 128: the "reduce" and 3x3-neighbour 1x1 convolutions of a ResNet50 bottleneck, reference
// models/deterministic/resnet_large.py:85-105, layers/flipout_layers/conv_flipout.py:376-417) as ONE 8-wave workgroup per CU
// with the K loop of the tap-unrolled kernel (gfx950; bf16, and the f32 / split-bf16 precisions on f32 activations).
//
// contract_dma_kernel runs these GEMMs at 0.23-0.29 of the MFMA peak: its 256-pixel tile needs 16 KB of activations per
// K-stage, rings of three is all that fits twice into a CU's LDS, so a stage reads its own fragments (LDS latency exposed every
// stage), waits on a run-time vmcnt and has its DMAs two stages ahead of an HBM latency of three.  A 1x1 convolution has no
// patch to reuse, so the room has to come from the occupancy: one workgroup per CU, 160 KB of LDS —
//
//   * tile 256 pixels x 128 channels: waves 0-3 own n-tile 2j, waves 4-7 n-tile 2j+1, on the SAME pixels (wave = 64 pixels x
//     64 channels, two accumulator sets: 128 registers).  One 16-KB activation stage serves both halves: half the L2 -> LDS
//     bytes per FLOP of the 64-channel tile;
//   * rings of FOUR for activations (64 KB), weight tiles (2 x 8 KB per stage: 64 KB) and s_in words: stage s+3 is requested
//     while stage s multiplies and stage s+1's fragments are read — the tap-unrolled kernel's loop: fragments double-buffered in
//     registers, ONE `s_waitcnt vmcnt(4)` immediate per stage (each wave issues exactly 2 + 2 DMA instructions per stage);
//   * staged store side of btx_epilogue.h (8 x 17 KB: the rings are dead by then), per-half constants.
//
// Same K order per output element as every other variant: bit-identical to contract_dma_kernel on the same launch.
// Host-checked (btx_plan.cpp): Flipout, bf16 activations and MFMA, pointwise geometry, K % 32 == 0, K >= 4 stages, an even
// number of whole n-tiles per group, one K split.  ContractParams: pt_rtiles = n-tile pairs per group.
#pragma once
#include <type_traits>
#include "btx_contract.h"
#include "btx_contract_dma.h"
#include "btx_contract_taps.h"
#include "btx_epilogue.h"
#include "btx_mma.h"
#include "btx_presample.h"

namespace btx {

struct G8Lds {
  static constexpr int TP = 256, RD = 4;
  static constexpr int A_STAGE = NG * TP * 16;   // 16384
  static constexpr int W_STAGE = 2 * DW_STAGE;   // 16384: [half][mu 4 KiB | delta 4 KiB]
  static constexpr int S_STAGE = TP * 4;
  static constexpr int A_OFF = 0;
  static constexpr int W_OFF = A_OFF + RD * A_STAGE;
  static constexpr int S_OFF = W_OFF + RD * W_STAGE;
  static constexpr int MAIN = S_OFF + RD * S_STAGE;         // 135168
  static constexpr int C_OFF = 8 * PT_EP_WAVE;              // 139264: constants of the two n-tiles behind the staging areas
  static constexpr int BYTES = C_OFF + 2 * 1024;            // 141312
};
static_assert(G8Lds::MAIN <= G8Lds::C_OFF && G8Lds::BYTES <= 163840, "LDS budget");

// The store side is staged through LDS.  A store side straight from the fragment registers (no LDS staging, about two thirds
// of the VALU work, but 32-byte pieces instead of whole lines) was measured here, where nothing covers the store side:
// bit-identical and slower — 9.4k / 11.9k cycles + 1k of drain against 3.8k + 4.2k for the two stages of the staged side on
// 256 -> 1024 at 14x14, 5-25 % on the layer call (profiles/r04_gemm8_phase_timers.txt).
template <int PREC, int KIND>
__global__ __launch_bounds__(512, 2) void contract_gemm8_kernel(const ContractParams) {
  static_assert(KIND == 1, "Flipout only: every wave issues the same number of weight DMAs per stage");
  BTX_SECTION_PARAMS_FLAT(p, logical);
  using LD = G8Lds;
  using ACT = typename std::conditional<PREC == 1, __bf16, float>::type;
  constexpr int G = (PREC == 1) ? 8 : 4, BK = NG * G, TP = LD::TP;
  constexpr uint32_t ESZ = (uint32_t)sizeof(ACT);
  // bf16: the NEXT stage's fragments are read while this one multiplies (two fragment sets).  f32 / split-bf16: a stage reads
  // its own fragments in its first part (the split's hi / lo halves take the registers of the second set) — their latency hides
  // behind the other wave group's MFMAs either way
  constexpr bool PF = (PREC == 1);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t smp = p.sample;
  if (p.sample_ptr) smp = sample_word_scalar(p.sample_ptr);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wave >> 2, w4 = wave & 3;
  const bool c_bias = p.mu_b != nullptr, c_aff = (p.ep_scale != nullptr) || (p.ep_shift != nullptr);

  // workgroup -> (pixel tile, group, n-tile pair): the pairs of a pixel tile are neighbours (its activations stay in one L2)
  uint32_t u_mtile, u_rem, u_group, u_pair;
  fdivmod((uint32_t)logical, p.fd_inner, (uint32_t)(p.pt_rtiles * p.groups), u_mtile, u_rem);
  fdivmod(u_rem, p.fd_rtiles, (uint32_t)p.pt_rtiles, u_group, u_pair);
  const int mtile = (int)u_mtile, group = (int)u_group, ntile0 = 2 * (int)u_pair;
  const int nstages = p.K / BK;  // host: >= 4
  // One workgroup per CU: nothing runs beside this workgroup's store side, so what the store needs and the K loop does not is
  // fetched here — the per-channel constants (bias parameters, BN scale / shift) of the two n-tiles, by waves 0 and 4: requested
  // in front of the first DMAs (they return first), turned into the store's [bias | bias delta | scale | shift] rows behind
  // the sign keys; their area lies behind the rings and the K loop's barriers publish it.
  EpRaw c_raw = {0.f, 0.f, 0.f, 1.f, 0.f};
  if ((c_bias || c_aff) && w4 == 0) c_raw = ep_load_constants(p, lane, ntile0 + half, group, c_bias, c_aff);

  const __amdgpu_buffer_rsrc_t wt_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.wt, 0, p.wt_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);

  // ---- weight loader: the stage's 16 rows of 1 KiB — (half 0|1) x (mu | delta) x (granule row 0..3) — rows 2w, 2w+1 to wave w
  uint32_t w_src[2];
  int w_dst[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 2 * wave + j, hf = r >> 3, set = (r >> 2) & 1, row = r & 3;
    w_src[j] = (uint32_t)(group * p.ntiles + ntile0 + hf) * (uint32_t)(p.K / G) * 1024u + (uint32_t)row * 1024u + (uint32_t)lane * 16u +
               (set ? p.wt_delta_off : 0u);
    w_dst[j] = LD::W_OFF + hf * DW_STAGE + set * 4096 + row * 1024;
  }
  // output pixel m -> input pixel: itself for stride 1 (a plain GEMM), else the strided position (1x1 down-sampling
  // convolutions: no padding, so every output pixel has its input pixel)
  auto pix_in = [&](int m) __attribute__((always_inline)) -> uint32_t {
    if (p.pointwise) return (uint32_t)m;
    uint32_t t, t2, ow, oh, od, nb;
    fdivmod((uint32_t)m, p.fd_Wo, (uint32_t)p.Wo, t, ow);
    fdivmod(t, p.fd_Ho, (uint32_t)p.Ho, t2, oh);
    fdivmod(t2, p.fd_Do, (uint32_t)p.Do, nb, od);
    return ((nb * (uint32_t)p.D + od * (uint32_t)p.sd) * (uint32_t)p.H + oh * (uint32_t)p.sh) * (uint32_t)p.W + ow * (uint32_t)p.sw;
  };
  // ---- activation loader: the stage's 16 pieces of 1 KiB (16 pixels x 64 B) — pieces 2w, 2w+1 to wave w; source-side XOR
  //      swizzle as in btx_contract_dma.h; out-of-range pixels read zeros
  const int g_lane = (lane & 3) ^ ((lane >> 4) & 3);
  uint32_t a_src[2];
  int a_dst[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int piece = 2 * wave + j;
    const int mq = mtile * TP + piece * 16 + (lane >> 2);
    a_src[j] = mq < p.M ? (pix_in(mq) * (uint32_t)p.C + (uint32_t)(group * p.Cg + G * g_lane)) * ESZ : DMA_OOB;
    a_dst[j] = LD::A_OFF + piece * 1024;
  }
  auto issue = [&](int s) __attribute__((always_inline)) {  // all L2 -> LDS traffic of stage s: 4 DMA instructions per wave
    const int slot = s & (LD::RD - 1);
    const uint32_t wo = (uint32_t)s * (uint32_t)NG * 1024u, ao = (uint32_t)(s * BK) * ESZ;
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(wt_rsrc, w_src[j] + wo, smem + w_dst[j] + slot * LD::W_STAGE);
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(x_rsrc, a_src[j] == DMA_OOB ? DMA_OOB : a_src[j] + ao, smem + a_dst[j] + slot * LD::A_STAGE);
  };
  issue(0);
  issue(1);
  issue(2);

  // ---- the sign keys of this (sample, layer), derived while the first DMAs travel
  RngLive rl = {smp, p.kin_a, p.kin_b, p.kout_a, p.kout_b};
  if (p.sample_ptr || p.lanes > 1) {
    rl.sample = __builtin_amdgcn_readfirstlane(smp);
    const uint32_t si = p.swap_signs ? 3u : 2u, so = p.swap_signs ? 2u : 3u;
    const BtxPhilox4 ki = btx_philox4x32_10(0u, rl.sample, p.layer, si, p.seed_lo, p.seed_hi);
    const BtxPhilox4 ko = btx_philox4x32_10(0u, rl.sample, p.layer, so, p.seed_lo, p.seed_hi);
    rl.kin_a = __builtin_amdgcn_readfirstlane(ki.x[0]); rl.kin_b = __builtin_amdgcn_readfirstlane(ki.x[1]);
    rl.kout_a = __builtin_amdgcn_readfirstlane(ko.x[0]); rl.kout_b = __builtin_amdgcn_readfirstlane(ko.x[1]);
  }
  // ---- s_in words: thread t < 256 hashes the word of pixel t for a stage (32 channels = one word)
  const int m_own = mtile * TP + (tid & 255);
  const uint32_t sg_off = pix_in(m_own < p.M ? m_own : 0) * (uint32_t)p.C + (uint32_t)(group * p.Cg);
  auto write_signs = [&](int s) __attribute__((always_inline)) {
    if (half == 0) {  // wave-uniform
      const uint32_t off = sg_off + (uint32_t)(s * BK);
      uint32_t w = p.sign_in ? sign_word_explicit(p.sign_in, off, p.x_bytes / ESZ) : btx_sign_word(off >> 5, rl.kin_a, rl.kin_b);
      if constexpr (G == 4) w <<= 8 * ((off >> 4) & 1);
      *(uint32_t*)(smem + LD::S_OFF + (s & (LD::RD - 1)) * LD::S_STAGE + (tid & 255) * 4) = w;
    }
  };
  write_signs(0);
  write_signs(1);
  write_signs(2);
  {
    // an opaque copy of the wave test: with the same condition on both blocks the compiler moves the first instruction of the
    // softplus up to the loads — and their s_waitcnt vmcnt(0) in front of the first DMAs of waves 0 and 4
    int w4b = w4;
    asm volatile("" : "+s"(w4b));
    if ((c_bias || c_aff) && w4b == 0) {
      asm volatile("" : "+v"(c_raw.mu), "+v"(c_raw.rho), "+v"(c_raw.eps), "+v"(c_raw.sc), "+v"(c_raw.sh));  // (nor speculated)
      ep_store_constants<KIND>(p, rl, c_raw, (float*)(smem + LD::C_OFF + half * 1024), lane, ntile0 + half, group, c_bias);
    }
  }

  // More work for the idle issue slots in front of the first barrier (the first stages are still travelling): what the store
  // side would otherwise compute with the matrix pipe idle — the four hashed s_out words of the lane's fragment blocks and the
  // address of the line this thread touches for the workgroup that follows on the CU (the store side's touch_next).  Five registers
  // across the K loop.
  uint32_t wsh_pre[4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const uint32_t orow = (uint32_t)(mtile * TP + w4 * 64 + mi * 32 + l31) * (uint32_t)p.N + (uint32_t)(group * p.Ng + (ntile0 + half) * BN);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) wsh_pre[mi * 2 + ni] = btx_sign_word((orow + 32u * ni) >> 5, rl.kout_a, rl.kout_b) << (2 * h);
  }
  uint32_t l2pf_off = 0xffffffffu;
  {
    const int nxt = logical + (p.reverse ? -32 : 32);
    if (nxt >= 0 && nxt < p.lane_nwg) {  // wave-uniform
      uint32_t n_mtile, n_rem, n_group, n_pair;
      fdivmod((uint32_t)nxt, p.fd_inner, (uint32_t)(p.pt_rtiles * p.groups), n_mtile, n_rem);
      fdivmod(n_rem, p.fd_rtiles, (uint32_t)p.pt_rtiles, n_group, n_pair);
      const int mq = (int)n_mtile * TP + (tid & 255);
      if (mq < p.M) {
        const size_t off = ((size_t)pix_in(mq) * (size_t)p.C + (size_t)((int)n_group * p.Cg)) * ESZ + (size_t)(tid >> 8) * 128u;
        if (off + 4 <= (size_t)p.x_bytes) l2pf_off = (uint32_t)off;
      }
    }
  }

  // (pinned here: left alone the compiler sinks both computations back to their use behind the K loop)
  asm volatile("" : "+v"(wsh_pre[0]), "+v"(wsh_pre[1]), "+v"(wsh_pre[2]), "+v"(wsh_pre[3]), "+v"(l2pf_off));

  f32x16 accm[2][2], accd[2][2];
  using Frag = StageFragT<2>;
  auto load_frag = [&](Frag& f, int s) __attribute__((always_inline)) {
    const int slot = s & (LD::RD - 1);
    const unsigned char* as = smem + LD::A_OFF + slot * LD::A_STAGE;
    const unsigned char* ss = smem + LD::S_OFF + slot * LD::S_STAGE;
    const unsigned char* ws = smem + LD::W_OFF + slot * LD::W_STAGE + half * DW_STAGE;
#pragma unroll
    for (int kk = 0; kk < NG / 2; ++kk) {
      const int row = 2 * kk + h;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        f.a[kk][mi] = *(const u32x4*)(as + (w4 * 64 + mi * 32 + l31) * 64 + ((row ^ ((l31 >> 2) & 3)) * 16));
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) f.wm[kk][ni] = *(const u32x4*)(ws + (row * BN + ni * 32 + l31) * 16);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) f.sw[mi] = *(const uint32_t*)(ss + (w4 * 64 + mi * 32 + l31) * 4);
  };

  // stages 0 and 1 landed (stage 2's four DMAs may be in flight); meet
  asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  Frag fa, fb;
  if constexpr (PF) load_frag(fa, 0);
  else {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accm[a][b][r] = 0.f; accd[a][b][r] = 0.f; }
  }
  // Eight waves marching in lock-step request, read and multiply together: the two waves of a SIMD queue for the matrix pipe
  // and then leave it idle together.  A stage is therefore two parts — A: this stage's delta fragments, the requests of stage
  // s+3, the next (bf16) or this (f32 / split-bf16) stage's fragments; B: the MFMAs — and waves 4-7 run one part behind waves
  // 0-3: on every SIMD one wave multiplies while the other loads (the K-group scheme of btx_contract_taps.h); a barrier behind
  // each part.
  // What a barrier has to guarantee (bf16): stage s+2 has landed (requested an interval ago: at most this
  // interval's four DMAs stay in flight) and nobody still reads the slot that is requested next — slot s, last read by
  // delta(s).  Part A therefore reads delta(s) FIRST and waits for it in front of its fragment reads (the requests and the sign
  // words are issued in between); the prefetched fragments stay in flight across the barrier — LDS returns in order, so they
  // are back when the next part A has its delta, a whole stage before their slot is requested again.  That wait is the
  // compiler's builtin: its own wait insertion sees it (an s_waitcnt inside inline asm it does not) and does not make the next
  // stage's MFMAs wait for reads that completed there.  f32 / split-bf16 (a stage multiplies the fragments it read in its own
  // part A): every barrier waits for all LDS reads.
  // Phase timers (profiles/r04_gemm8_phase_timers.txt): MFMAs + barriers alone 1280 cycles per stage (1030 = the matrix
  // pipe), s_in masks +200, DMA +70, sign words +55: 1480.  All eight waves in lock-step instead, every operand of a K-step
  // read half a stage before it is multiplied (two alternating sets, one barrier per stage): bit-identical and slower, 1 950 -
  // 2 040 cycles per stage against 1 500, cfg5 -1 %.
  constexpr bool RELAX = PF;  // bf16: no LDS wait at the barrier behind part A
  DeltaFrag df;
  auto a_body = [&](int s, Frag& f) __attribute__((always_inline)) {  // f: bf16 the set of stage s+1, else of stage s
    load_delta<KIND>(df, smem + LD::W_OFF + (s & (LD::RD - 1)) * LD::W_STAGE + half * DW_STAGE, l31, h);
    __builtin_amdgcn_sched_barrier(0);
    if (s + 3 < nstages) {  // wave-uniform
      issue(s + 3);
      write_signs(s + 3);
    }
    if constexpr (RELAX) {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (PF) { if (s + 1 < nstages) load_frag(f, s + 1); }
    else load_frag(f, s);
  };
  auto b_body = [&](Frag& cur, auto first_tag) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_tag)::value;
    // the parts stay apart in the instruction stream: loads hoisted over the MFMAs in front of them would need a third
    // fragment set (the compiler renames, then spills)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (FIRST && PREC == 1) stage_mma<PREC, KIND, 2, 2, true>(cur, df, accm, accd, l31, h);
    else stage_mma<PREC, KIND>(cur, df, accm, accd, l31, h);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto meet = [&](int s) __attribute__((always_inline)) {  // end of the interval in which stage s+3 was requested (or not)
    if constexpr (RELAX) {
      if (s + 3 < nstages) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    } else {
      if (s + 3 < nstages) end_stage<4>(); else end_stage<0>();
    }
  };
  using TT = std::true_type;
  using FF = std::false_type;
  if (half == 1) asm volatile("s_barrier" ::: "memory");
  if constexpr (PF) {
    a_body(0, fb); meet(0); b_body(fa, TT{}); meet(0);
    int s = 1;
    for (; s + 1 < nstages; s += 2) {
      a_body(s, fa); meet(s); b_body(fb, FF{}); meet(s);
      a_body(s + 1, fb); meet(s + 1); b_body(fa, FF{}); meet(s + 1);
    }
    if (s < nstages) { a_body(s, fa); meet(s); b_body(fb, FF{}); meet(s); }
  } else {
    for (int s = 0; s < nstages; ++s) { a_body(s, fa); meet(s); b_body(fa, FF{}); meet(s); }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (half == 0) asm volatile("s_barrier" ::: "memory");

  // =================== store side (btx_epilogue.h): every wave stages its own 64 x 64 tile ============================
  {
    BTX_SECTION_PARAMS_FLAT(pe, logical2);
    // what the store side reads, fetched in the same batch of scalar loads (else: one round trip per branch that tests one)
    asm volatile("" ::"s"(pe.N), "s"(pe.Ng), "s"(pe.M), "s"(pe.ksplits), "s"(pe.mu_b), "s"(pe.ep_scale), "s"(pe.ep_shift),
                 "s"(pe.sign_out), "s"(pe.out_bf16), "s"(pe.ep_relu));
    // The workgroup that follows this one on the CU is the one 32 slots further on in the XCD's range of logical ids (32 CUs
    // per XCD, one workgroup each; xcd_logical()).  Its first wait is the HBM round trip of its first activation stages —
    // 3.9k .. 7.3k cycles of prologue in the phase timers, longest on the layers that keep HBM busy.  Thread t touches one
    // 128-byte line of that tile (pixel t % 256, stages 0-1 | 2-3; address from the prologue), so the rows are in this XCD's L2
    // when they are asked for: prologue 5.0k -> 3.1k cycles on 256 -> 1024 at 14x14.  Issued from the store side's hook, BEHIND
    // the residual requests: in front of them stage 1 grew by what the prologue saved.
    uint32_t l2pf = 0;
    auto touch_next = [&]() __attribute__((always_inline)) {
      if (l2pf_off != 0xffffffffu) l2pf = *(const uint32_t*)((const unsigned char*)pe.x + l2pf_off);
    };
    const bool has_bias = pe.mu_b != nullptr;
    const bool has_aff = (pe.ep_scale != nullptr) || (pe.ep_shift != nullptr);
    float* ba = (float*)(smem + LD::C_OFF + half * 1024);
    const uint32_t m0 = (uint32_t)mtile * (uint32_t)TP;
    const PixContig pm = {m0, min(TP, pe.M - (int)m0)};
    // RES_PRE: the residual rows are requested in front of the store side's first stage
    staged_epilogue_pm<KIND, 8, PixContig, true, decltype(touch_next)>(pe, rl, accm, accd, smem, tid, wave, lane, ntile0 + half,
                                                                       group, 0, pm, w4, true, ba, touch_next, wsh_pre);
    asm volatile("" ::"v"(l2pf));  // the touch is "used"
  }
}

template <int PREC>
static int launch_contract_gemm8_impl(int kind, const ContractParams& p, int nwg, hipStream_t st) {
  if (kind != 1) return -3;
  auto kfn = contract_gemm8_kernel<PREC, 1>;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, G8Lds::BYTES);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  int rc = launch_presample_impl<PREC>(kind, p, st);
  if (rc) return rc;
  hipLaunchKernelGGL(kfn, dim3(nwg), dim3(512), G8Lds::BYTES, st, p);
  return (int)hipGetLastError();
}

}  // namespace btx
