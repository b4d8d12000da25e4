// btx_api.hip — the contraction entry points of libbtx.so (include/btx.h): the launch glue behind the host planner
// (btx_plan.cpp decides what runs; this file fills ContractParams and launches it) and the weight pre-sampling.  gfx950 only.
// The small HBM-bound kernels and their entry points are in btx_small.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "../../include/btx.h"
#include <stdlib.h>
#include "btx_contract.h"
#include "btx_rng.h"
#include "btx_presample.h"

using namespace btx;

static int contract_fwd_impl(int kind, const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w,
                             const float* mu_b, const float* rho_b, void* out, const BtxRng* rng, const BtxNoise* noise,
                             int act_dtype, int prec, uint32_t flags, void* ws, size_t ws_bytes, void* stream,
                             const BtxEpilogue* ep, const BtxLanes* ln, int var = 0, float* root = nullptr) {
  if (!g || !x || !mu_w || !rho_w || !out || !rng) return BTX_E_NULL;
  if (var == 1 && !root) return BTX_E_NULL;
  const int lanes = ln ? ln->n : 1;
  if ((mu_b == nullptr) != (rho_b == nullptr)) return BTX_E_NULL;
  // every pointer some fast family reads or writes in 16-byte granules (the residual: btx_epilogue.h stage 2).  The bias, the
  // scale / shift vectors, eps_b and the explicit sign arrays are read element by element in every family: no requirement.
  const uintptr_t al = (uintptr_t)x | (uintptr_t)mu_w | (uintptr_t)rho_w | (uintptr_t)out |
                       (uintptr_t)(noise && noise->eps_w ? noise->eps_w : nullptr) |
                       (uintptr_t)(ep && ep->residual ? ep->residual : nullptr) | (uintptr_t)root;
  FwdSel sel;
  // var 2 (noise-free kind-0 contraction of the LRT backward): planned as kind 2 — register-staged or gather kernel, one K range
  int rc = select_fwd(var == 2 ? BTX_KIND_LRT : kind, g, act_dtype, prec, flags, (al & 15) != 0, noise, ep, &sel);
  if (rc) return rc;
  const Plan& pl = sel.pl;
  const void* sampled_w = (noise && noise->sampled_w) ? noise->sampled_w : nullptr;
  if (sel.need && (!ws || ws_bytes < sel.need)) return BTX_E_WORKSPACE;
  if (sel.need && (((uintptr_t)ws) & 15)) return BTX_E_ALIGN;

  ContractParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.mu = mu_w; p.rho = rho_w; p.mu_b = mu_b; p.rho_b = rho_b; p.out = out; p.root = root;
  p.partial = pl.ksplits > 1 ? (float*)ws : nullptr;
  p.lanes = lanes; p.lane_nwg = pl.nwg; p.fd_lane_nwg = make_fastdiv((uint32_t)(pl.nwg > 0 ? pl.nwg : 1));
  if (lanes > 1) {
    p.lane_x = ln->x_stride; p.lane_out = ln->out_stride; p.lane_res = ln->res_stride;
    p.lane_partial = (long long)(plan_ws(pl, g, 1));
  }
  if (noise) {
    p.eps_w = noise->eps_w; p.eps_b = noise->eps_b;
    p.sign_in = noise->sign_in; p.sign_out = noise->sign_out;
  }
  p.NB = g->NB; p.D = g->D; p.H = g->H; p.W = g->W; p.C = g->C; p.Cg = pl.Cg;
  p.Do = pl.Do; p.Ho = pl.Ho; p.Wo = pl.Wo; p.N = g->N; p.Ng = pl.Ng;
  p.KD = g->KD; p.KH = g->KH; p.KW = g->KW;
  p.sd = g->sd; p.sh = g->sh; p.sw = g->sw; p.pd = g->pd; p.ph = g->ph; p.pw = g->pw;
  p.dd = g->dd; p.dh = g->dh; p.dw = g->dw;
  p.M = pl.M; p.K = pl.K;
  p.mtiles = pl.mtiles; p.ntiles = pl.ntiles; p.groups = g->groups; p.ksplits = pl.ksplits; p.kper = pl.kper;
  p.transposed = (flags & BTX_FLAG_TRANSPOSED) ? 1 : 0;
  p.pointwise = (!p.transposed && g->KD == 1 && g->KH == 1 && g->KW == 1 && g->sd == 1 && g->sh == 1 && g->sw == 1 &&
                 g->pd == 0 && g->ph == 0 && g->pw == 0) ? 1 : 0;
  p.out_bf16 = sel.out_bf16;
  if (ep) { p.ep_scale = ep->scale; p.ep_shift = ep->shift; p.ep_res = ep->residual; p.ep_relu = ep->relu; }
  if (flags & BTX_FLAG_ROWFUSE) {  // K = KH*(KW*C) unchanged; the pixel stride p.C stays C
    p.Cg = g->KW * g->C;
    p.KW = 1;
    p.sign_unaligned = 1;
  }
  p.fd_Cg = make_fastdiv((uint32_t)p.Cg); p.fd_KW = make_fastdiv((uint32_t)p.KW); p.fd_KH = make_fastdiv((uint32_t)p.KH);
  p.seed_lo = (uint32_t)rng->seed; p.seed_hi = (uint32_t)(rng->seed >> 32);
  p.sample = rng->sample_idx; p.layer = rng->layer_id;
  p.sample_ptr = rng->sample_idx_dev;
  // BTX_FLAG_SWAP_SIGNS (data gradient of a Flipout layer): the op's input carries the forward's s_out, its output the
  // forward's s_in
  p.fd_sd = make_fastdiv((uint32_t)g->sd); p.fd_sh = make_fastdiv((uint32_t)g->sh); p.fd_sw = make_fastdiv((uint32_t)g->sw);
  if (sel.par_major) {
    p.par_major = 1; p.par_Hh = pl.Ho / 2; p.par_Wh = pl.Wo / 2; p.par_Mq = g->NB * p.par_Hh * p.par_Wh; p.par_Mqp = sel.par_mqp;
    p.fd_par_Mqp = make_fastdiv((uint32_t)p.par_Mqp); p.fd_par_Hh = make_fastdiv((uint32_t)p.par_Hh);
    p.fd_par_Wh = make_fastdiv((uint32_t)p.par_Wh);
  }
  p.swap_signs = (flags & BTX_FLAG_SWAP_SIGNS) ? 1 : 0;
  p.reverse = (flags & BTX_FLAG_REVERSE) ? 1 : 0;
  sign_keys(rng, p.swap_signs ? BTX_STREAM_SIGN_OUT : BTX_STREAM_SIGN_IN, &p.kin_a, &p.kin_b);
  sign_keys(rng, p.swap_signs ? BTX_STREAM_SIGN_IN : BTX_STREAM_SIGN_OUT, &p.kout_a, &p.kout_b);
  {
    const long long in_elems = (long long)g->NB * g->D * g->H * g->W * g->C;
    const long long xb = in_elems * (act_dtype == BTX_ACT_BF16 ? 2 : 4), wb = (long long)g->N * pl.K * 4;
    p.x_bytes = xb < 0xffffffffLL ? (uint32_t)xb : 0xffffffffu;
    p.w_bytes = wb < 0xffffffffLL ? (uint32_t)wb : 0xffffffffu;
  }

  p.fd_inner = make_fastdiv((uint32_t)(pl.ntiles * g->groups * pl.ksplits)); p.fd_ksplits = make_fastdiv((uint32_t)pl.ksplits);
  p.fd_ntiles = make_fastdiv((uint32_t)pl.ntiles); p.fd_rtiles = make_fastdiv(1u);
  p.fd_mtiles = make_fastdiv((uint32_t)(pl.mtiles > 0 ? pl.mtiles : 1));
  {
    // XCD affinity of the workgroup order (block b runs on XCD b % 8; the remap gives every XCD a contiguous range of
    // logical ids): keep in one L2 whichever operand the neighbours would otherwise re-fetch more bytes of — the
    // activations of a pixel tile (read by its ntiles*ksplits workgroups) or the sampled weights of an (n-tile, k-split)
    // (read by its mtiles workgroups).  ResNet18 layer4 (7x7 maps, 512 channels): 9.4 MB of weight tiles against 3.2 MB
    // of activations; measured HBM-side traffic of that launch in round 1 order: 92 MB for 25 MB algorithmic.
    // Weight tiles up to ~3 MB stay resident in every XCD's 4-MB L2 whatever the order; beyond that the weight-major
    // order is what keeps them on chip.  (Round 4, 20 MC sample lanes per launch, rocprofv3 FETCH/WRITE_SIZE: ResNet18
    // layer3 — 2.36 MB of tiles per lane, 6.4 MB of activations — moves 2.98x its algorithmic bytes weight-major, where the
    // activations are re-fetched once per n-tile, and 2.00x pixel-major; the launch time is the same either way.)
    const double w_b = (prec == BTX_PREC_BF16 ? 2.0 : 4.0) * (double)g->N * pl.K * (kind == BTX_KIND_FLIPOUT ? 2 : 1);
    p.wg_order = (uses_tiles(sel.family) && pl.mtiles > 1 && w_b >= WG_MAJOR_MIB * 1048576.0) ? 1 : 0;
  }
  p.fd_Wo = make_fastdiv((uint32_t)pl.Wo); p.fd_Ho = make_fastdiv((uint32_t)pl.Ho); p.fd_Do = make_fastdiv((uint32_t)pl.Do);
  if (uses_tiles(sel.family)) {
    p.wt = sampled_w ? (void*)sampled_w : (void*)((unsigned char*)ws + sel.wt_off);
    p.wt_ready = sampled_w ? 1 : 0;
    p.wt_bytes = (uint32_t)sel.wt_all;
    p.wt_delta_off = (uint32_t)sel.wt_one;
    p.lane_wt = (long long)sel.wt_one;  // Flipout: lane l's delta tiles at wt_delta_off + l*lane_wt; else its W tiles at l*lane_wt
    p.lane_wt_delta = (kind == BTX_KIND_FLIPOUT) ? 1 : 0;
  }
  hipStream_t st = (hipStream_t)stream;
  // one launcher per (family, precision); the launch of the family select_fwd decided
  typedef int (*LaunchFn)(int, const ContractParams&, int, hipStream_t);
  auto launch = [&](LaunchFn f32, LaunchFn bf16, LaunchFn x3) {
    return (prec == BTX_PREC_BF16 ? bf16 : prec == BTX_PREC_BF16X3 ? x3 : f32)(kind, p, pl.nwg * lanes, st);
  };
  switch (sel.family) {
    case BTX_FAMILY_STEM_POOL: {
      const StemPoolPlan& spp = sel.spp;
      p.pt_R = spp.PB; p.pt_rtiles = spp.bands; p.pt_Rp = spp.Rp; p.pt_astage = spp.astage; p.st_sbytes = spp.sbytes;
      p.pt_lds = spp.lds; p.pt_PP = spp.patch_bytes; p.sp_Hq = spp.Hq; p.sp_Wq = spp.Wq;
      p.fd_rtiles = make_fastdiv((uint32_t)spp.bands);
      rc = launch_stem_pool_bf16(kind, p, pl.nwg * lanes, st);
      break;
    }
    case BTX_FAMILY_STEM: {
      const StemPlan& stp = sel.stp;
      p.pt_R = stp.R; p.pt_Rp = stp.Rp; p.pt_rtiles = stp.rtiles; p.pt_nw = stp.nw; p.pt_astage = stp.astage;
      p.st_sbytes = stp.sbytes; p.pt_lds = stp.lds; p.pt_PP = stp.patch_bytes;
      p.fd_rtiles = make_fastdiv((uint32_t)stp.rtiles);
      rc = launch(launch_contract_stem_f32, launch_contract_stem_bf16, launch_contract_stem_x3);
      break;
    }
    case BTX_FAMILY_PATCH:
    case BTX_FAMILY_TAPS:
    case BTX_FAMILY_TAPS2: {
      const PatchPlan& pt = sel.pt;
      p.pt_G = pt.G; p.pt_R = pt.R; p.pt_Rp = pt.Rp; p.pt_Wp = pt.Wp; p.pt_PP = pt.PP; p.pt_NI = pt.NI;
      p.fd_ptWp = make_fastdiv((uint32_t)pt.Wp); p.fd_ptRp = make_fastdiv((uint32_t)pt.Rp); p.fd_ptR = make_fastdiv((uint32_t)pt.R);
      p.fd_rtiles = make_fastdiv((uint32_t)pt.rtiles);
      p.pt_rtiles = pt.rtiles; p.pt_nw = pt.nw; p.pt_astage = pt.astage; p.pt_lds = pt.lds;
      p.pt_taps = pt.taps; p.pt_kg = pt.kg; p.pt_lds_g = pt.lds_g;
      p.pt_wide = (pt.taps == 33 || pt.taps == 332) ? pt.wide : 0;
      if (p.pt_wide) {  // the grid's n-tiles are pairs of weight tiles (p.ntiles stays the tile count of the weight layout)
        p.fd_ntiles = make_fastdiv((uint32_t)(pl.ntiles / 2));
        p.fd_inner = make_fastdiv((uint32_t)((pl.ntiles / 2) * g->groups * pl.ksplits));
      }
      p.pt_tall = pt.tall; p.pt_P = pt.P; p.pt_Wt = pt.Wt; p.pt_ncs = pt.ncs;
      p.fd_P = make_fastdiv((uint32_t)pt.P); p.fd_Wt = make_fastdiv((uint32_t)pt.Wt); p.fd_ncs = make_fastdiv((uint32_t)pt.ncs);
      rc = launch(launch_contract_patch_f32, launch_contract_patch_bf16, launch_contract_patch_x3);
      break;
    }
    case BTX_FAMILY_GEMM8:
      p.pt_rtiles = sel.g8_pairs;
      p.fd_rtiles = make_fastdiv((uint32_t)sel.g8_pairs); p.fd_inner = make_fastdiv((uint32_t)(sel.g8_pairs * g->groups));
      rc = launch(launch_contract_gemm8_f32, launch_contract_gemm8_bf16, launch_contract_gemm8_x3);
      break;
    case BTX_FAMILY_DMA:
      rc = launch(launch_contract_dma_f32, launch_contract_dma_bf16, launch_contract_dma_x3);
      break;
    default: {  // BTX_FAMILY_REGSTAGE, BTX_FAMILY_GATHER
      // the register-staged fast kernel samples in registers and hashes its own s_in: explicit eps_w / sign_in need either
      // the LDS-DMA family above (pre-pass sampling, packed sign words) or the gather kernel
      // (BTX_PREC_BF16X3 has no register-staged form: such shapes run on the exact-f32 kernel, which is at least as accurate)
      const bool gen2 = sel.family == BTX_FAMILY_GATHER || (noise && (noise->eps_w || noise->sign_in));
      if (var)  // the training variants of local reparameterization (contract_kernel VAR)
        rc = (prec == BTX_PREC_BF16) ? launch_contract_var_bf16(var, act_dtype == BTX_ACT_BF16, gen2, p, pl.nwg * lanes, st)
                                     : launch_contract_var_f32(var, act_dtype == BTX_ACT_BF16, gen2, p, pl.nwg * lanes, st);
      else
        rc = (prec == BTX_PREC_BF16) ? launch_contract_bf16(kind, act_dtype == BTX_ACT_BF16, gen2, p, pl.nwg * lanes, st)
                                     : launch_contract_f32(kind, act_dtype == BTX_ACT_BF16, gen2, p, pl.nwg * lanes, st);
    }
  }
  if (rc) return rc;
  if (pl.ksplits > 1) {
    const long long total = (long long)pl.M * g->N;
    long long blocks = (total / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    {  // one launch for all MC sample lanes (blockIdx.y)
      const float* part = (const float*)ws;
      const unsigned char* r = (const unsigned char*)p.ep_res;
      if (sel.out_bf16)
        hipLaunchKernelGGL(splitk_reduce_kernel<__bf16>, dim3((int)blocks, lanes), dim3(256), 0, st, part, (__bf16*)out, total,
                           pl.ksplits, g->N, p.ep_scale, p.ep_shift, (const __bf16*)r, p.ep_relu, p.lane_partial, p.lane_out,
                           p.lane_res);
      else
        hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3((int)blocks, lanes), dim3(256), 0, st, part, (float*)out, total,
                           pl.ksplits, g->N, p.ep_scale, p.ep_shift, (const float*)r, p.ep_relu, p.lane_partial, p.lane_out,
                           p.lane_res);
      rc = (int)hipGetLastError();
    }
  }
  return rc;
}

int btx::contract_var(int var, const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w, const float* mu_b,
                      const float* rho_b, void* out, float* root, const BtxRng* rng, int act_dtype, int prec, uint32_t flags,
                      void* stream) {
  if (var != 1 && var != 2) return BTX_E_UNSUPPORTED;
  return contract_fwd_impl(var == 1 ? BTX_KIND_LRT : BTX_KIND_REPARAM, g, x, mu_w, rho_w, mu_b, rho_b, out, rng, nullptr, act_dtype,
                           prec, flags & ~BTX_FLAG_LANES_MASK, nullptr, 0, stream, nullptr, nullptr, var, root);
}

extern "C" {

int btx_abi_version(void) { return BTX_ABI_VERSION; }

const char* btx_strerror(int code) {
  switch (code) {
    case 0: return "ok";
    case BTX_E_NULL: return "btx: required pointer is NULL";
    case BTX_E_SHAPE: return "btx: inconsistent or non-positive shape";
    case BTX_E_UNSUPPORTED: return "btx: unsupported configuration";
    case BTX_E_WORKSPACE: return "btx: workspace too small";
    case BTX_E_DTYPE: return "btx: unknown dtype / precision code";
    case BTX_E_ALIGN: return "btx: pointer not 16-byte aligned";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "btx: unknown error";
  }
}

int btx_contract_fwd(int kind, const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w,
                     const float* mu_b, const float* rho_b, void* out, const BtxRng* rng, const BtxNoise* noise,
                     int act_dtype, int prec, uint32_t flags, void* ws, size_t ws_bytes, void* stream) {
  return btx_contract_fwd_ex(kind, g, x, mu_w, rho_w, mu_b, rho_b, out, rng, noise, act_dtype, prec, flags, ws,
                             ws_bytes, stream, nullptr);
}

int btx_contract_fwd_ex(int kind, const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w,
                        const float* mu_b, const float* rho_b, void* out, const BtxRng* rng, const BtxNoise* noise,
                        int act_dtype, int prec, uint32_t flags, void* ws, size_t ws_bytes, void* stream,
                        const BtxEpilogue* ep) {
  return contract_fwd_impl(kind, g, x, mu_w, rho_w, mu_b, rho_b, out, rng, noise, act_dtype, prec,
                           flags & ~BTX_FLAG_LANES_MASK, ws, ws_bytes, stream, ep, nullptr);
}

int btx_contract_fwd_lanes(int kind, const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w,
                           const float* mu_b, const float* rho_b, void* out, const BtxRng* rng, const BtxNoise* noise,
                           int act_dtype, int prec, uint32_t flags, void* ws, size_t ws_bytes, void* stream,
                           const BtxEpilogue* ep, const BtxLanes* lanes) {
  if (!lanes) return BTX_E_NULL;
  if (lanes->n < 1 || lanes->n > 255) return BTX_E_SHAPE;
  if ((lanes->x_stride | lanes->out_stride | lanes->res_stride) & 15) return BTX_E_ALIGN;
  if (noise && lanes->n > 1 && (noise->eps_w || noise->eps_b || noise->sign_in || noise->sign_out)) return BTX_E_UNSUPPORTED;
  return contract_fwd_impl(kind, g, x, mu_w, rho_w, mu_b, rho_b, out, rng, noise, act_dtype, prec,
                           (flags & ~BTX_FLAG_LANES_MASK) | BTX_FLAG_LANES(lanes->n), ws, ws_bytes, stream, ep, lanes);
}

int btx_sample_weights(const BtxSampleItem* items, int n_items, const BtxRng* rng, int prec, void* stream) {
  return btx_sample_weights_lanes(items, n_items, rng, prec, stream, 1, 0);
}

int btx_sample_weights_lanes(const BtxSampleItem* items, int n_items, const BtxRng* rng, int prec, void* stream, int lanes,
                             uint32_t sflags) {
  if (!items || !rng) return BTX_E_NULL;
  if (lanes < 1 || lanes > 255) return BTX_E_SHAPE;
  const uint64_t seed = rng->seed;
  const uint32_t sample_idx = rng->sample_idx;
  if (n_items <= 0) return n_items == 0 ? 0 : BTX_E_SHAPE;
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16 && prec != BTX_PREC_BF16X3) return BTX_E_DTYPE;
  for (int base = 0; base < n_items; base += PRESAMPLE_MAX_ITEMS) {
    PresampleBatch b;
    memset(&b, 0, sizeof(b));
    b.n = n_items - base < PRESAMPLE_MAX_ITEMS ? n_items - base : PRESAMPLE_MAX_ITEMS;
    b.seed_lo = (uint32_t)seed; b.seed_hi = (uint32_t)(seed >> 32); b.sample = sample_idx; b.sample_ptr = rng->sample_idx_dev;
    b.lanes = lanes; b.skip_mu = (sflags & BTX_SAMPLE_SKIP_MU) ? 1 : 0;
    uint32_t blocks = 0;
    for (int i = 0; i < b.n; ++i) {
      const BtxSampleItem& s = items[base + i];
      if (!s.geom || !s.mu_w || !s.rho_w || !s.out) return BTX_E_NULL;
      if (s.kind != BTX_KIND_REPARAM && s.kind != BTX_KIND_FLIPOUT) return BTX_E_UNSUPPORTED;
      const bool remap = s.src_C != 0 || s.src_KW != 0;  // scalar reads: no alignment requirement on mu/rho
      if ((((uintptr_t)s.out) & 15) || (!remap && (((uintptr_t)s.mu_w | (uintptr_t)s.rho_w) & 15))) return BTX_E_ALIGN;
      Plan pl;
      int rc = make_plan(s.geom, prec, 0, DBM, &pl);
      if (rc) return rc;
      if (pl.K % (prec == BTX_PREC_BF16 ? 8 : 4)) return BTX_E_UNSUPPORTED;  // whole 16-byte granules of the tile image
      size_t one = 0;
      if (patch_wt_bytes(pl, s.geom, s.kind, prec, &one, lanes) >= 0xfff00000ULL) return BTX_E_UNSUPPORTED;
      PresampleItem& it = b.it[i];
      it.mu = s.mu_w; it.rho = s.rho_w; it.wt = (unsigned char*)s.out;
      it.delta_off = (uint32_t)one;
      it.nquads = (uint32_t)(s.geom->groups * pl.ntiles * 64) * ((uint32_t)pl.K >> 2);
      it.first_block = blocks;
      it.layer = s.layer_id;
      it.Ng = pl.Ng; it.K = pl.K; it.ntiles = pl.ntiles; it.kind = s.kind;
      if (s.src_C != 0 || s.src_KW != 0) {
        if (s.geom->groups != 1 || s.src_C <= 0 || s.src_KW <= 0 || s.src_C > s.geom->C || s.src_KW > s.geom->KW ||
            s.geom->C % 4)
          return BTX_E_UNSUPPORTED;
        it.Cp = s.geom->C; it.KWp = s.geom->KW; it.src_KW = s.src_KW; it.src_C = s.src_C;
      }
      uint32_t nb = lanes > 1 ? (it.nquads + 255u) / 256u : (it.nquads + 1023u) / 1024u;  // ~4 (quad, lane) pairs per thread
      if (nb < 1) nb = 1;
      if (nb > (lanes > 1 ? 4096u : 1024u)) nb = lanes > 1 ? 4096u : 1024u;
      blocks += nb;
    }
    b.total_blocks = blocks;
    int rc = (prec == BTX_PREC_BF16) ? launch_presample_batch_bf16(b, (hipStream_t)stream)
             : (prec == BTX_PREC_BF16X3) ? launch_presample_batch_x3(b, (hipStream_t)stream)
                                         : launch_presample_batch_f32(b, (hipStream_t)stream);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
