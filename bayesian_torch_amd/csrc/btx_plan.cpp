// btx_plan.cpp — the host-side planner (btx_plan.h) and the pure-host entry points of include/btx.h that answer from it.
// No HIP include: builds with `c++ -std=c++17 -c`.  The promise that an MC sample sums in the same order however many samples
// share its launch (include/btx.h: btx_contract_fwd_lanes) rests on the rules in this file.
#include <string.h>
#include "btx_plan.h"

namespace btx {

// MC sample lanes of the launch being planned (BTX_FLAG_LANES(n) in the flags): the grid is `lanes` copies of the
// single-sample grid, so that many times more workgroups fill the workgroup slots before K has to be split
static inline long long plan_lanes(uint32_t flags) {
  const long long n = (flags >> BTX_FLAG_LANES_SHIFT) & 0xffu;
  return n > 1 ? n : 1;
}

static inline bool throughput_plan(uint32_t flags) { return (flags & BTX_FLAG_CONCURRENT) || plan_lanes(flags) > 1; }

// The ONE split-K cost search: pick the split that minimises (grid rounds on the workgroup slots) x (cost of a split + fixed
// per-block cost).  `base1`: workgroups of ONE lane before the split — the split must not depend on the lane count; `units`
// of `unit_cost` each are dealt over the splits; splits run from 1 to `max_split`; `full_splits`: only splits that divide
// the units (the 8-wave kernel of two K-groups wants every split full).
// `throughput` (throughput_plan): other launches fill the CUs this one leaves idle, so what counts is its CU-time, and that
// only grows with the split (fixed per-block cost, partial sums through HBM, the reduce launch): split just far
// enough that the launch is not a long thin tail of its own stream.  Launches with MC sample lanes take the same
// plan, decided by the grid of ONE lane: the K split — the f32 summation order — of a sample then does not depend
// on how many samples share its launch, nor on how the samples were grouped over launches and ranks.
// `short_exit` (make_plan only): 16 workgroups of at most 16 stages are enough as well: ResNet18's fc (16 n-tiles of 16 stages
// per lane) in ONE piece — 4 splits of 4 stages + the reduce launch measured 77 us per 20 lanes against 39
// (profiles/r06_experiments.txt E18)
static int split_k(long long base1, int units, int unit_cost, int max_split, bool full_splits, bool throughput, bool short_exit) {
  int ks = 1;
  long long best = -1;
  for (int c = 1; c <= max_split; ++c) {
    if (full_splits && units % c) continue;
    const int per = (units + c - 1) / c;
    const long long rounds = (base1 * c + SLOTS - 1) / SLOTS;
    const long long cost = rounds * (per * unit_cost + 4) + (c > 1 ? 1 : 0);  // +1: the reduce pass
    if (best < 0 || cost < best) { best = cost; ks = c; }
    if (throughput && (base1 * c >= 64 || (short_exit && base1 * c >= 16 && per <= 16))) { ks = c; break; }
  }
  return ks;
}

int make_plan(const BtxGeom* g, int prec, uint32_t flags, int bm, Plan* pl) {
  int rc = btx_out_shape(g, flags, &pl->Do, &pl->Ho, &pl->Wo);
  if (rc) return rc;
  if (prec != BTX_PREC_F32 && prec != BTX_PREC_BF16 && prec != BTX_PREC_BF16X3) return BTX_E_DTYPE;
  pl->Cg = g->C / g->groups;
  pl->Ng = g->N / g->groups;
  const long long M = (long long)g->NB * pl->Do * pl->Ho * pl->Wo;
  const long long K = (long long)g->KD * g->KH * g->KW * pl->Cg;
  if (M > 0x7fffffffLL || K > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  pl->M = (int)M;
  pl->K = (int)K;
  const int bk = NG * (prec == BTX_PREC_BF16 ? 8 : 4);
  pl->mtiles = (pl->M + bm - 1) / bm;
  pl->ntiles = (pl->Ng + BN - 1) / BN;
  const long long base1 = (long long)pl->mtiles * pl->ntiles * g->groups;
  const int stages = (pl->K + bk - 1) / bk;
  // split-K over the stages; each split keeps >= 4 stages so the DMA ring fills.  (Not "ceil(stages / c) >= 4": the floor.)
  const int max_ks = stages / 4 > 1 ? (stages / 4 < 32 ? stages / 4 : 32) : 1;
  const int ks = split_k(base1, stages, 1, max_ks, false, throughput_plan(flags), true);
  int per_stages = (stages + ks - 1) / ks;
  pl->kper = per_stages * bk;
  pl->ksplits = (pl->K + pl->kper - 1) / pl->kper;
  const long long nwg = base1 * pl->ksplits;  // per lane
  if (nwg > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  pl->nwg = (int)nwg;
  return 0;
}

// Shape-level eligibility of the LDS-DMA pipeline (btx_contract_dma.h); pointer alignment is checked at launch.
static bool dma_shape_ok(const BtxGeom* g, int act_dtype, int prec, const Plan& pl) {
  if ((prec == BTX_PREC_BF16) != (act_dtype == BTX_ACT_BF16)) return false;  // DMA cannot convert
  const int bk = NG * (prec == BTX_PREC_BF16 ? 8 : 4);
  if (pl.Cg % bk) return false;  // a K-stage must lie inside one filter tap
  const long long in_elems = (long long)g->NB * g->D * g->H * g->W * g->C;
  const long long esz = (act_dtype == BTX_ACT_BF16) ? 2 : 4;
  if (in_elems * esz >= 0xfff00000LL || (long long)pl.M * g->N >= 0x7fffffffLL ||
      (long long)g->N * pl.K * 4 >= 0xfff00000LL)
    return false;  // 32-bit byte offsets inside the buffer descriptors
  return true;
}

// Tall-strip tile of the tap-unrolled kernel: the batch as ONE tall image with P = max(H + ph, Ho) virtual rows per image
// (P - H zero rows between consecutive images: bottom padding of one, top padding of the next; output rows >= Ho of a
// period are dummies), cut into tiles of R virtual rows x Wt columns.  R and Wt need not divide Ho / Wo, so the tile
// can fill the 256 pixel slots of a workgroup whatever the map size (7 | 14 | 28 | 56: 252 pixels) where whole-row /
// whole-image tiles leave an eighth to a quarter of the MFMA tiles empty.  Returns the fraction of pixel slots that hold
// real output pixels (0: no tall tile fits).
static double tall_tile(const BtxGeom* g, const Plan& pl, int tp, int ppcap, PatchPlan* pt) {
  const int halo_r = (g->KH - 1) * g->dh, halo_c = (g->KW - 1) * g->dw;
  if (g->ph > halo_r) return 0.0;
  const int P = (g->H + g->ph > pl.Ho) ? g->H + g->ph : pl.Ho;
  const long long rows_total = (long long)(g->NB - 1) * P + pl.Ho;
  double best = 0.0;
  for (int ncs = 1; ncs <= 8; ++ncs) {
    const int Wt = (pl.Wo + ncs - 1) / ncs;
    if (Wt > tp || Wt < 4 || (ncs > 1 && Wt < 8)) continue;  // Wt >= 4: PixTall::Walk steps 8 pixels with two row wraps
    int R = tp / Wt;
    if (R > rows_total) R = (int)rows_total;
    while (R >= 1 && (R + halo_r) * (Wt + halo_c) > ppcap) --R;
    if (R < 1) continue;
    const long long rtiles = (rows_total + R - 1) / R;
    const double eff = (double)pl.M / ((double)rtiles * ncs * tp);
    if (eff > best * 1.01) {
      best = eff;
      pt->tall = 1; pt->P = P; pt->Wt = Wt; pt->ncs = ncs;
      pt->G = 1; pt->R = R; pt->Rp = R + halo_r; pt->Wp = Wt + halo_c; pt->PP = pt->Rp * pt->Wp;
      pt->rtiles = (int)rtiles;
    }
  }
  return best;
}
// tile of `tp` output pixels whose patch holds at most `ppcap` pixels
static bool patch_tile(const BtxGeom* g, const Plan& pl, int tp, int ppcap, PatchPlan* pt) {
  const int Ho = pl.Ho, Wo = pl.Wo;
  const int Wp = Wo + (g->KW - 1) * g->dw, halo_r = (g->KH - 1) * g->dh;
  if (Wo > tp || Wp * (1 + halo_r) > ppcap) return false;
  int G = 1, R;
  if (Ho * Wo <= tp / 2 || (Ho * Wo <= tp && (Ho + halo_r) * Wp <= ppcap)) {
    R = Ho;
    const int Rp = R + halo_r;
    if (Rp * Wp > ppcap) return false;
    G = tp / (Ho * Wo);
    if (G > ppcap / (Rp * Wp)) G = ppcap / (Rp * Wp);
    if (G > g->NB) G = g->NB;
    if (G < 1) return false;
  } else {
    int rmax = tp / Wo;
    const int rfit = ppcap / Wp - halo_r;
    if (rfit < rmax) rmax = rfit;
    if (rmax > Ho) rmax = Ho;
    if (rmax < 1) return false;
    const int nrt = (Ho + rmax - 1) / rmax;
    R = (Ho + nrt - 1) / nrt;
    // equal row tiles, unless the tallest tile that fits issues fewer 32-pixel MFMA tiles over the image (a tile's tail of < 32
    // pixels still costs a whole MFMA tile per stage): 28 rows of 28 pixels as 7 + 7 + 7 + 7 are 4 x 7 = 28 MFMA tiles, as
    // 8 + 8 + 8 + 4 they are 3 x 7 + 4 = 25 (the stride-2 3x3 layer at 56 -> 28: -10.7 % of its MFMAs)
    auto mfma_tiles = [&](int r) {
      long long n = 0;
      for (int row = 0; row < Ho; row += r) n += ((long long)((Ho - row < r) ? Ho - row : r) * Wo + 31) / 32;
      return n;
    };
    if (rmax > R && (Ho % rmax == 0 || 2 * (Ho % rmax) >= rmax) && mfma_tiles(rmax) < mfma_tiles(R)) R = rmax;  // (no sliver of a last tile)
  }
  pt->G = G; pt->R = R; pt->Rp = R + halo_r; pt->Wp = Wp; pt->PP = G * pt->Rp * Wp;
  pt->rtiles = (Ho + R - 1) / R;
  return pt->PP <= ppcap && G * R * Wo <= tp;
}

// ---- what the two patch plans (make_patch_plan, make_patch2_plan) share ----

// Checks every patch plan starts with; fills the plan of 512-pixel tiles the patch plan is then cut from.
static bool patch_base_ok(const BtxGeom* g, int act_dtype, int prec, uint32_t flags, Plan* pl, PatchPlan* pt) {
  if (flags & (BTX_FLAG_TRANSPOSED | BTX_FLAG_ROWFUSE)) return false;
  pt->wide = 0;
  if (make_plan(g, prec, flags, DBM, pl)) return false;
  if (!dma_shape_ok(g, act_dtype, prec, *pl)) return false;
  return g->D == 1 && g->KD == 1 && pl->Do == 1;
}
// LDS of a workgroup of pt->nw waves whose tile pt->PP is set: `slots` patch slots with their sign slots, `wd` weight tiles and
// the scratch piece of btx_contract_taps.h — or the epilogue staging, whichever is larger; at most `max_ni` 1-KiB DMA
// instructions per wave per patch slot.
static bool patch_lds(PatchPlan* pt, int slots, int wd, int max_ni) {
  const int pieces = (pt->PP + 15) / 16;
  pt->NI = (pieces + pt->nw - 1) / pt->nw;
  if (pt->NI > max_ni) return false;
  pt->astage = pieces * 1024;
  int lds = slots * pt->astage + slots * (pt->astage / 16) + wd * 8192 + 1024;
  const int ep = pt->nw * PT_EP_WAVE + 1024;
  if (lds < ep) lds = ep;
  if (lds > (pt->nw == 4 ? 81920 : 163840)) return false;
  pt->lds = lds;
  pt->lds_g = (lds + 15) & ~15;
  return true;
}
// Reparameterization on a tap-unrolled kernel: one accumulator set per output, so the wave can hold a 64-pixel x 128-channel
// tile (contract_taps_kernel<..., WIDE>, contract_taps2_kernel<..., WIDE>) — taken when whole pairs of n-tiles exist and the
// halved grid still fills the workgroup slots (few-tile launches keep the narrow tile and its K-groups).
static void wide_tile(const BtxGeom* g, int kind, int act_dtype, int prec, uint32_t flags, const Plan& pl, PatchPlan* pt) {
  if (kind == BTX_KIND_REPARAM && prec == BTX_PREC_BF16 && act_dtype == BTX_ACT_BF16 && (pl.Ng % 128) == 0 &&
      (long long)pl.mtiles * (pl.ntiles / 2) * g->groups * plan_lanes(flags) >= SLOTS) {
    pt->wide = 1;
    if (pt->lds < pt->nw * PT_EP_WAVE + 2048) {  // its store side keeps the constants of two channel tiles
      pt->lds = pt->nw * PT_EP_WAVE + 2048;
      pt->lds_g = (pt->lds + 15) & ~15;
    }
  }
}
// workgroups of one lane before the K split, on the grid the plan launches
static long long patch_base1(const BtxGeom* g, const Plan& pl, const PatchPlan& pt) {
  return (long long)pl.mtiles * (pt.wide ? pl.ntiles / 2 : pl.ntiles) * g->groups;
}
// split-K over the channel blocks of a patch plan whose tile, pt->wide and pt->kg are decided; T: taps per channel block
static bool patch_split_k(const BtxGeom* g, int prec, uint32_t flags, int T, Plan* pl, const PatchPlan& pt) {
  const int bk = NG * (prec == BTX_PREC_BF16 ? 8 : 4);
  const int units = pl->Cg / bk / pt.kg;  // channel blocks per K-group over the whole K
  const long long base1 = patch_base1(g, *pl, pt);
  // Throughput plans decide the K split on the grid of the NARROW tile: there the wide tile changes the tile shape, never kper /
  // ksplits.  (A launch with lanes goes wide where the one-lane plan of its samples stays narrow: both must sum in the same
  // order.)  The latency plan of a lone launch promises no such thing and prices the grid it launches.
  const long long base1n = throughput_plan(flags) ? (long long)pl->mtiles * pl->ntiles * g->groups : base1;
  int max_ks = 1;  // the largest split (<= 32) that leaves every split 4 stages: ceil(units / c) * T >= 4
  while (max_ks < units && max_ks < 32 && (units + max_ks) / (max_ks + 1) * T >= 4) ++max_ks;
  const int ks = split_k(base1n, units, T, max_ks, pt.kg == 2, throughput_plan(flags), false);
  const int per = (units + ks - 1) / ks;
  pl->kper = per * pt.kg * bk;
  pl->ksplits = (units + per - 1) / per;
  const long long nwg = base1 * pl->ksplits;
  if (nwg > 0x7fffffffLL) return false;
  pl->nwg = (int)nwg;
  return true;
}

// Tile plan of the patch variant (PatchPlan).  Returns false when the shape is not eligible.
// kind: BTX_KIND_* of the launch being planned, or -1 (the plan every kind can take)
static bool make_patch_plan(const BtxGeom* g, int act_dtype, int prec, uint32_t flags, Plan* pl, PatchPlan* pt, int kind = -1) {
  if (!patch_base_ok(g, act_dtype, prec, flags, pl, pt) || g->sh != 1 || g->sw != 1) return false;
  const int T = g->KH * g->KW;
  if (T < 2 || T > 64) return false;
  // 4-wave blocks, two per CU: 2 patch slots + 2 sign slots + 4 weight tiles within 80 KiB -> 22 pieces = 352 pixels;
  // 8-wave blocks, one per CU: 60 pieces = 960 pixels
  pt->tall = 0; pt->P = 1; pt->Wt = 1; pt->ncs = 1;
  if (patch_tile(g, *pl, 256, 352, pt)) pt->nw = 4;
  else if (patch_tile(g, *pl, 512, 960, pt)) pt->nw = 8;
  else return false;
  // 3x3 on 4-wave blocks (the tap-unrolled kernel): tall-strip tiles when they fill the pixel slots better
  if (pt->nw == 4 && g->KH == 3 && g->KW == 3) {
    const long long mt_old = (long long)((g->NB + pt->G - 1) / pt->G) * pt->rtiles;
    const double eff_old = (double)pl->M / ((double)mt_old * 256.0);
    PatchPlan tp = *pt;
    const double eff_tall = tall_tile(g, *pl, 256, 352, &tp);
    // measured (profiles/r03_tall_tiles_ab.txt, batch 256 / 512 = the tiles of 4 / 8 MC sample lanes): the heavier
    // tile (4 full waves, a store side 50 % longer) pays off only where it removes >= ~15 % of the workgroups (28x28:
    // 19 %, +3 / +8 %; 14x14: 16 %, -5 / +2 %); on 56x56 (9 % fewer workgroups) and 7x7 (6 %) it loses 4-7 %
    if (eff_tall > eff_old * TALL_MIN_GAIN) *pt = tp;
  }
  if (!patch_lds(pt, 2, PT_WD, PT_MAXNI)) return false;
  // grid: m-tiles are (image group, row tile); split-K over the channel blocks
  pl->mtiles = pt->tall ? pt->rtiles * pt->ncs : ((g->NB + pt->G - 1) / pt->G) * pt->rtiles;
  pt->taps = (pt->nw == 4 && pt->NI <= 6 && g->KH == 3 && g->KW == 3) ? 33 : 0;
  if (pt->taps == 33) wide_tile(g, kind, act_dtype, prec, flags, *pl, pt);
  // Few pixel tiles (at most one 4-wave block per CU): 8-wave blocks of two K-groups — split-K inside the workgroup
  // through LDS instead of through HBM, and two waves per SIMD.
  // BTX_FLAG_CONCURRENT: plain 4-wave blocks — an 8-wave block takes the whole LDS of its CU, so two such launches of
  // different MC samples cannot share a CU; 4-wave blocks of two launches pair up and free-run against each other
  // (measured, ResNet18 bs 64, 3 / 4 / 6 samples in flight: 1340 / 1369 / 1346 -> 1382 / 1402 / 1378 MC-samples/s).
  const int ncb = pl->Cg / (NG * (prec == BTX_PREC_BF16 ? 8 : 4));
  pt->kg = (pt->taps && !throughput_plan(flags) && patch_base1(g, *pl, *pt) * plan_lanes(flags) <= 256 && ncb >= 2 && (ncb % 2) == 0 &&
            2 * pt->lds_g <= 163840) ? 2 : 1;
  if (!patch_split_k(g, prec, flags, T, pl, *pt)) return false;
  if (pt->kg == 2) pt->lds = 2 * pt->lds_g;
  return true;
}

// Tile plan of the stride-2 form of the tap-unrolled kernel (btx_contract_taps2.h): 3x3 / stride 2 / pad 1, one phase
// plane of (R+1) x (Wo+1) pixels per image of the tile in each of three LDS slots.
static bool make_patch2_plan(const BtxGeom* g, int act_dtype, int prec, uint32_t flags, Plan* pl, PatchPlan* pt, int kind = -1) {
  if (!patch_base_ok(g, act_dtype, prec, flags, pl, pt)) return false;
  if (g->KH != 3 || g->KW != 3 || g->sh != 2 || g->sw != 2 || g->ph != 1 || g->pw != 1 || g->dh != 1 || g->dw != 1) return false;
  BtxGeom gp = *g;  // the plane of a tile is the halo'd patch of a 2x2 stride-1 window: R+1 rows, Wo+1 columns
  gp.KH = 2; gp.KW = 2;
  if (!patch_tile(&gp, *pl, 256, 272, pt)) return false;
  pt->nw = 4;
  pt->tall = 0; pt->P = 1; pt->Wt = 1; pt->ncs = 1;
  if (!patch_lds(pt, 3, 3, 5)) return false;
  pl->mtiles = ((g->NB + pt->G - 1) / pt->G) * pt->rtiles;
  wide_tile(g, kind, act_dtype, prec, flags, *pl, pt);
  pt->taps = 332;
  pt->kg = 1;
  return patch_split_k(g, prec, flags, 9, pl, *pt);
}

static bool make_stem_plan(const BtxGeom* g, int act_dtype, int prec, const Plan& pl, StemPlan* st) {
  if (g->D != 1 || g->KD != 1 || pl.Do != 1 || g->groups != 1) return false;
  const int esz = (act_dtype == BTX_ACT_BF16) ? 2 : 4;
  const int bk = NG * (prec == BTX_PREC_BF16 ? 8 : 4);
  if ((g->KW * g->C) % bk || pl.K % bk) return false;
  const long long rowB = (long long)g->W * g->C * esz;
  for (int nw = 4; nw <= 8; nw += 4) {
    const int tp = 64 * nw;
    if (pl.Wo > tp) continue;
    int R = tp / pl.Wo;
    if (R > pl.Ho) R = pl.Ho;
    const long long cap = (nw == 4 ? 81920 : 163840) - PT_WD * 8192;
    for (; R >= 1; --R) {
      const long long Rp = (long long)(R - 1) * g->sh + g->KH;
      const long long pb = Rp * rowB;
      const long long astage = (pb + 1023) / 1024 * 1024;
      const long long sbytes = ((pb / esz + 31) / 32 + 3) * 4;
      const long long sb16 = (sbytes + 15) / 16 * 16;
      if (astage + sb16 > cap) continue;
      long long lds = astage + sb16 + PT_WD * 8192;
      const long long ep = (long long)nw * PT_EP_WAVE + 1024;
      if (lds < ep) lds = ep;
      st->R = R; st->Rp = (int)Rp; st->rtiles = (pl.Ho + R - 1) / R; st->nw = nw; st->astage = (int)astage;
      st->sbytes = (int)sb16; st->lds = (int)lds; st->patch_bytes = (int)pb;
      const long long nwg = (long long)g->NB * st->rtiles * pl.ntiles;
      if (nwg > 0x7fffffffLL) return false;
      st->nwg = (int)nwg;
      return true;
    }
  }
  return false;
}

static bool make_stem_pool_plan(const BtxGeom* g, int act_dtype, int prec, const Plan& pl, StemPoolPlan* sp, int lanes = 1) {
  if (prec != BTX_PREC_BF16 || act_dtype != BTX_ACT_BF16) return false;
  if (g->D != 1 || g->KD != 1 || pl.Do != 1 || g->groups != 1) return false;
  const int bk = NG * 8;
  if ((g->KW * g->C) % bk || pl.K % bk || (g->N % 64)) return false;
  const int nstages = pl.K / bk;
  if (nstages < 1 || nstages > 7) return false;
  if (2 * pl.Wo > 256 || pl.Ho < 1) return false;
  const int Hq = (pl.Ho - 1) / 2 + 1, Wq = (pl.Wo - 1) / 2 + 1;
  const long long rowB = (long long)g->W * g->C * 2;
  const long long Rp = (long long)g->sh + g->KH;  // input rows of a half tile (two conv rows)
  const long long pb = Rp * rowB;
  const long long astage = (pb + 1023) / 1024 * 1024;
  const long long sbytes = ((pb / 2 + 31) / 32 + 3) * 4;
  const long long sb16 = (sbytes + 127) / 128 * 128;  // keeps the store-side rows 128-byte aligned (chunk swizzle in address bits)
  // weights | raw patch x2 | signed patch copy | sign words x2 | store-side rows r0, r1, carry (128 B per pixel) | constants
  const long long lds = (long long)nstages * 8192 + 3 * astage + 2 * sb16 + 3LL * pl.Wo * 128 + 1024 + 64;  // (+ the pool's two `ninf` chunks)
  if (lds > 163840) return false;
  // bands: about one workgroup per CU (every band pays two phases of fill / drain, a closing one-row half tile and the
  // fetch of the layer's weight tiles).  With MC sample lanes the launch has `lanes` times the (image, n-tile) units, so the
  // bands get longer — 20 lanes of a ResNet stem at batch 64: one band per image instead of four.  Which workgroup computes a
  // row does not change how it is computed: results are bit-identical whatever the band length.
  const long long units = (long long)g->NB * pl.ntiles;
  long long PB = ((long long)Hq * units * (lanes > 1 ? lanes : 1)) / 256;
  if (PB < 4) PB = 4;
  if (PB > Hq) PB = Hq;
  const int bands = (Hq + (int)PB - 1) / (int)PB;
  const long long nwg = units * bands;
  if (nwg > 0x7fffffffLL) return false;
  sp->PB = (int)PB; sp->bands = bands; sp->Rp = (int)Rp; sp->astage = (int)astage; sp->sbytes = (int)sb16;
  sp->lds = (int)lds; sp->patch_bytes = (int)pb; sp->nwg = (int)nwg; sp->Hq = Hq; sp->Wq = Wq;
  return true;
}

// workspace of the patch variant: split-K partials (256-byte padded), then the pre-sampled weight tiles
// Flipout: [mu tiles | delta tiles of lane 0 | lane 1 | ...] — the mu tiles do not depend on the MC sample, one set serves
// every lane; Reparameterization: [W tiles of lane 0 | lane 1 | ...]
size_t patch_wt_bytes(const Plan& pl, const BtxGeom* g, int kind, int prec, size_t* one, int lanes) {
  const size_t arr = (size_t)g->groups * pl.ntiles * 64 * (size_t)pl.K * (prec == BTX_PREC_BF16 ? 2 : 4);
  if (one) *one = arr;
  return arr * (size_t)(kind == BTX_KIND_FLIPOUT ? 1 + lanes : lanes);
}
static size_t pad256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t plan_ws(const Plan& pl, const BtxGeom* g, int lanes) {
  return pl.ksplits > 1 ? (size_t)lanes * (size_t)pl.ksplits * (size_t)pl.M * (size_t)g->N * sizeof(float) : 0;
}

int select_fwd(int kind, const BtxGeom* g, int act_dtype, int prec, uint32_t flags, bool unaligned, const BtxNoise* noise,
               const BtxEpilogue* ep, FwdSel* s) {
  if (kind != BTX_KIND_REPARAM && kind != BTX_KIND_FLIPOUT && kind != BTX_KIND_LRT) return BTX_E_UNSUPPORTED;
  if (act_dtype != BTX_ACT_F32 && act_dtype != BTX_ACT_BF16) return BTX_E_DTYPE;
  memset(s, 0, sizeof(*s));
  const int lanes = (int)plan_lanes(flags);
  Plan& pl = s->pl;
  int rc = make_plan(g, prec, flags, BM, &pl);
  if (rc) return rc;
  // Local reparameterization (BTX-LRT v1): the register-staged kernel or the gather kernel, nothing else.  The
  // store takes the root of the variance sum, and sqrt is not linear: K is never split (a small-M launch is mtiles * ntiles * groups
  // workgroups per lane, however long K is).  No weight noise exists, so there is nothing to pre-sample, to pass in or to pool.
  if (kind == BTX_KIND_LRT) {
    if (prec == BTX_PREC_BF16X3) return BTX_E_UNSUPPORTED;
    if (flags & (BTX_FLAG_ROWFUSE | BTX_FLAG_OUT_F32 | BTX_FLAG_OUT_BF16)) return BTX_E_UNSUPPORTED;
    if (ep && ep->pool) return BTX_E_UNSUPPORTED;
    if (noise && (noise->sampled_w || noise->eps_w || noise->eps_b || noise->sign_in || noise->sign_out)) return BTX_E_UNSUPPORTED;
    const int G2 = (prec == BTX_PREC_BF16) ? 8 : 4;
    const bool gen2 = (pl.Cg % G2 != 0) || unaligned || (flags & BTX_FLAG_GATHER) != 0;
    pl.ksplits = 1; pl.kper = pl.K;
    const long long nwg = (long long)pl.mtiles * pl.ntiles * g->groups;
    if (nwg * lanes > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
    pl.nwg = (int)nwg;
    s->family = gen2 ? BTX_FAMILY_GATHER : BTX_FAMILY_REGSTAGE;
    s->out_bf16 = (act_dtype == BTX_ACT_BF16) ? 1 : 0;
    s->g8_pairs = 1;
    s->pt.kg = 1;
    s->need = 0;
    return 0;
  }

  // fast (granule) paths need whole 16-byte granules everywhere; otherwise the element-wise gather path
  const int G = (prec == BTX_PREC_BF16) ? 8 : 4;
  // Explicit noise (parity mode) runs on the same kernels as generated noise: eps_w enters the sampling pre-pass, the
  // sign words are packed from sign_in / sign_out.  BTX_FLAG_GATHER forces the element-wise gather kernel (tests).
  const bool explicit_kloop = (flags & BTX_FLAG_GATHER) != 0;
  const bool gen = (pl.Cg % G != 0) || unaligned || explicit_kloop;
  // LDS-DMA pipeline when the activations already have the contraction dtype (no conversion on the way to LDS)
  const bool rowfuse = (flags & BTX_FLAG_ROWFUSE) != 0;
  bool dma = !gen && dma_shape_ok(g, act_dtype, prec, pl);
  // Sample where the weights are used when nothing shares the sampled tile.  A pointwise layer (Linear, 1x1x1 at stride 1) with
  // at most 256 rows per MC sample reads every weight once per sample: the register-staged kernel — (mu, rho) straight into the
  // wave's registers, softplus + Philox + Box-Muller there, the sampled tile never exists in HBM (north_star's kernel design) —
  // does strictly less memory work than a sampling pre-pass plus a tile DMA (measured equal or faster: BASELINE cfg2 10 718 vs
  // 10 592 MC-samples/s, profiles/r05_experiments.txt E6).  Layers whose tiles are shared by many pixel tiles — every convolution
  // of a ResNet — keep pre-sampled tiles: there an in-kernel sampler repeats each draw once per pixel tile.
  // A caller that hands over pre-sampled tiles (BtxNoise.sampled_w) or explicit noise keeps the LDS-DMA family.
  {
    const bool pointwise_geom = !(flags & BTX_FLAG_TRANSPOSED) && g->KD == 1 && g->KH == 1 && g->KW == 1 && g->sd == 1 && g->sh == 1 &&
                                g->sw == 1 && g->pd == 0 && g->ph == 0 && g->pw == 0;
    // (single-sample launches only: with MC sample lanes the pre-sampled form of the ResNet18 classifier — 20 lanes x 64 rows — runs
    // in 72 us against 109 us, the tiles of all lanes coming from the one sampling launch of the replay)
    // BTX_FLAG_CONCURRENT single-sample launches are planned like lanes (a lane is bit-identical to them): same kernel as the lanes.
    if (dma && !rowfuse && pointwise_geom && lanes == 1 && !(flags & BTX_FLAG_CONCURRENT) && pl.M <= 256 && prec != BTX_PREC_BF16X3 &&
        !(noise && (noise->sampled_w || noise->eps_w || noise->sign_in || noise->sign_out)) &&
        !(flags & (BTX_FLAG_OUT_F32 | BTX_FLAG_OUT_BF16)))
      dma = false;
  }
  if (rowfuse) {
    // one K-stage = one kernel row: the K walk sees KW*C "channels" per tap and a single tap per row
    const int esz = (act_dtype == BTX_ACT_BF16) ? 2 : 4;
    const int bk = NG * G;
    const bool ok = !unaligned && !explicit_kloop && !(noise && noise->sign_in) && (prec == BTX_PREC_BF16) == (act_dtype == BTX_ACT_BF16) &&
                    g->groups == 1 && g->dw == 1 && g->pw == 0 && !(flags & BTX_FLAG_TRANSPOSED) &&
                    ((g->KW * g->C) % bk == 0) && ((g->sw * g->C * esz) % 16 == 0) && ((g->W * g->C * esz) % 16 == 0) &&
                    (g->C % G == 0 || G % g->C == 0);
    if (!ok) return BTX_E_UNSUPPORTED;
    dma = true;
  }
  // LDS-DMA variant: 4-wave blocks on 256-pixel tiles (two per CU)
  if (dma) {
    rc = make_plan(g, prec, flags, 256, &pl);
    if (rc) return rc;
  }
  // Parity-major pixel order (ContractParams.par_major) for the data gradient of a stride-2 2-D convolution — a transposed launch
  // whose gather rule leaves 1, 2, 2 or 4 of a 3x3 filter's 9 taps per output-pixel parity class: with the pixels enumerated class by
  // class every 256-pixel tile walks only its class's taps (2.25 of 9 on average) and needs no K split.  Single-sample launches of
  // the generic LDS-DMA kernel with at least 8 pixel tiles and more than one tap.
  // Not under the throughput plan: a lane launch takes raster order, and a BTX_FLAG_CONCURRENT launch must sum as its lanes do.
  bool par_major = false;
  int par_mqp = 0;
  if (dma && !rowfuse && (flags & BTX_FLAG_TRANSPOSED) && !throughput_plan(flags) && g->groups == 1 && g->D == 1 && g->KD == 1 && g->sd == 1 &&
      g->sh == 2 && g->sw == 2 && g->KH * g->KW <= 31 && g->KH * g->KW > 1 && (pl.Ho % 2) == 0 && (pl.Wo % 2) == 0 &&
      pl.mtiles >= 8) {
    const int tp = 256;
    const long long mq = (long long)g->NB * (pl.Ho / 2) * (pl.Wo / 2);
    const long long tiles_per_class = (mq + tp - 1) / tp;  // the last tile of a class is padded: no tile holds two classes
    if (4 * tiles_per_class * pl.ntiles <= 0x7fffffffLL) {
      par_major = true;
      par_mqp = (int)(tiles_per_class * tp);
      pl.mtiles = (int)(4 * tiles_per_class);
      pl.ksplits = 1; pl.kper = pl.K;
      pl.nwg = pl.mtiles * pl.ntiles * g->groups;
    }
  }
  // stem variant: row-fused small-C convolutions with the input rows of the tile resident in LDS
  StemPlan stp = {};
  bool stem = false;
  if (dma && rowfuse) {
    Plan sp;
    if (!make_plan(g, prec, flags, DBM, &sp) && make_stem_plan(g, act_dtype, prec, sp, &stp)) {
      sp.ksplits = 1; sp.kper = sp.K; sp.nwg = stp.nwg;
      pl = sp;
      stem = true;
    }
  }
  // stem + max-pool (BtxEpilogue.pool): the band kernel of btx_contract_stempool.h or nothing
  StemPoolPlan spp = {};
  const bool want_pool = ep && ep->pool;
  if (want_pool) {
    Plan sp;
    // (the pool kernel's store side knows ReLU only: ReLU6 is refused here, the caller clamps a ReLU launch's output)
    if (ep->pool != 1 || !stem || ep->residual || ep->relu == 2 || (noise && (noise->sign_in || noise->sign_out)) ||
        (flags & (BTX_FLAG_OUT_F32 | BTX_FLAG_SWAP_SIGNS)) || make_plan(g, prec, flags, DBM, &sp) ||
        !make_stem_pool_plan(g, act_dtype, prec, sp, &spp, lanes))
      return BTX_E_UNSUPPORTED;
    pl.nwg = spp.nwg;
  }
  // patch variant: stride-1 2-D convolutions keep the halo'd input patch of the tile in LDS
  PatchPlan pt = {};
  bool patch = false;
  if (dma && !rowfuse) {
    Plan pp;
    if (make_patch_plan(g, act_dtype, prec, flags, &pp, &pt, kind)) { pl = pp; patch = true; }
    else if (make_patch2_plan(g, act_dtype, prec, flags, &pp, &pt, kind)) { pl = pp; patch = true; }
  }
  int out_bf16 = (act_dtype == BTX_ACT_BF16) ? 1 : 0;
  if (flags & (BTX_FLAG_OUT_F32 | BTX_FLAG_OUT_BF16)) {
    if (!dma) return BTX_E_UNSUPPORTED;
    out_bf16 = (flags & BTX_FLAG_OUT_BF16) ? 1 : 0;
  }
  // Pointwise Flipout contractions with a long K on the 8-wave GEMM of btx_contract_gemm8.h: one workgroup per CU, a
  // 256-pixel x 128-channel tile, rings of four (conditions in that header).
  bool gemm8 = false;
  int g8_pairs = 1;
  {
    const int bk8 = NG * (prec == BTX_PREC_BF16 ? 8 : 4);  // (dma: the activation dtype is the contraction's)
    if (dma && !rowfuse && !patch && kind == BTX_KIND_FLIPOUT &&
        !(flags & BTX_FLAG_TRANSPOSED) && g->KD == 1 && g->KH == 1 && g->KW == 1 &&
        g->pd == 0 && g->ph == 0 && g->pw == 0 && (pl.K % bk8) == 0 && pl.K >= 4 * bk8 && pl.K >= GEMM8_MIN_K && (pl.Ng % 128) == 0) {
      const long long mt = (pl.M + 255) / 256;
      g8_pairs = pl.Ng / 128;
      const long long nwg = mt * g->groups * g8_pairs;
      if (nwg * lanes <= 0x7fffffffLL) {
        gemm8 = true;
        pl.mtiles = (int)mt; pl.ksplits = 1; pl.kper = pl.K; pl.nwg = (int)nwg;
      }
    }
  }
  size_t need = plan_ws(pl, g, lanes);
  // LDS-DMA and patch variants: the weights are sampled once per launch into the workspace (btx_presample.h),
  // behind the split-K partials
  size_t wt_off = 0, wt_one = 0, wt_all = 0;
  const void* sampled_w = (noise && noise->sampled_w) ? noise->sampled_w : nullptr;
  if (sampled_w && (((uintptr_t)sampled_w) & 15)) return BTX_E_ALIGN;
  if (dma) {
    wt_off = pad256(need);
    wt_all = patch_wt_bytes(pl, g, kind, prec, &wt_one, lanes);
    if (sampled_w && wt_all < 0xfff00000ULL) wt_off = need;  // tiles live in the caller's buffer
    if (wt_off + wt_all >= 0xfff00000ULL) {  // 32-bit offsets inside the descriptor: register-staged kernel instead
      // The tiles of a launch grow with its lanes: the lane count alone would move a sample onto another kernel (another
      // summation order).  A launch with lanes is refused; its caller runs one single-sample launch per lane.
      if (rowfuse || (flags & (BTX_FLAG_OUT_F32 | BTX_FLAG_OUT_BF16)) || lanes > 1) return BTX_E_UNSUPPORTED;
      dma = false;
      rc = make_plan(g, prec, flags, BM, &pl);
      if (rc) return rc;
      need = plan_ws(pl, g, lanes);
    } else if (!sampled_w) {
      need = wt_off + wt_all;
    }
  }
  if ((long long)pl.nwg * lanes > 0x7fffffffLL) return BTX_E_UNSUPPORTED;
  // the family, decided once: everything but the two register-staged kernels belongs to the LDS-DMA pipeline
  if (!dma) s->family = gen ? BTX_FAMILY_GATHER : BTX_FAMILY_REGSTAGE;
  else if (want_pool) s->family = BTX_FAMILY_STEM_POOL;
  else if (stem) s->family = BTX_FAMILY_STEM;
  else if (patch) s->family = pt.taps == 33 ? BTX_FAMILY_TAPS : pt.taps == 332 ? BTX_FAMILY_TAPS2 : BTX_FAMILY_PATCH;
  else s->family = gemm8 ? BTX_FAMILY_GEMM8 : BTX_FAMILY_DMA;
  s->par_major = (par_major && s->family == BTX_FAMILY_DMA) ? 1 : 0;
  s->par_mqp = par_mqp; s->g8_pairs = g8_pairs; s->out_bf16 = out_bf16;
  s->stp = stp; s->spp = spp;
  if (dma && patch) s->pt = pt;
  else s->pt.kg = 1;
  s->need = need; s->wt_off = wt_off; s->wt_one = wt_one; s->wt_all = wt_all;
  return 0;
}

}  // namespace btx

using namespace btx;

extern "C" {

int btx_out_shape(const BtxGeom* g, uint32_t flags, int32_t* Do, int32_t* Ho, int32_t* Wo) {
  if (!g || !Do || !Ho || !Wo) return BTX_E_NULL;
  if (g->NB <= 0 || g->D <= 0 || g->H <= 0 || g->W <= 0 || g->C <= 0 || g->N <= 0 || g->KD <= 0 || g->KH <= 0 ||
      g->KW <= 0 || g->sd <= 0 || g->sh <= 0 || g->sw <= 0 || g->dd <= 0 || g->dh <= 0 || g->dw <= 0 ||
      g->pd < 0 || g->ph < 0 || g->pw < 0 || g->groups <= 0)
    return BTX_E_SHAPE;
  if (g->C % g->groups || g->N % g->groups) return BTX_E_SHAPE;
  if (flags & BTX_FLAG_TRANSPOSED) {
    *Do = (g->D - 1) * g->sd - 2 * g->pd + g->dd * (g->KD - 1) + g->od + 1;
    *Ho = (g->H - 1) * g->sh - 2 * g->ph + g->dh * (g->KH - 1) + g->oh + 1;
    *Wo = (g->W - 1) * g->sw - 2 * g->pw + g->dw * (g->KW - 1) + g->ow + 1;
  } else {
    *Do = (g->D + 2 * g->pd - g->dd * (g->KD - 1) - 1) / g->sd + 1;
    *Ho = (g->H + 2 * g->ph - g->dh * (g->KH - 1) - 1) / g->sh + 1;
    *Wo = (g->W + 2 * g->pw - g->dw * (g->KW - 1) - 1) / g->sw + 1;
  }
  if (*Do <= 0 || *Ho <= 0 || *Wo <= 0) return BTX_E_SHAPE;
  return 0;
}

int btx_contract_pool_shape(const BtxGeom* g, int act_dtype, int prec, uint32_t flags, int32_t* Hq, int32_t* Wq) {
  if (!g || !(flags & BTX_FLAG_ROWFUSE) || (flags & (BTX_FLAG_TRANSPOSED | BTX_FLAG_OUT_F32 | BTX_FLAG_SWAP_SIGNS | BTX_FLAG_GATHER)))
    return 0;
  Plan sp;
  StemPlan stp;
  StemPoolPlan spp;
  if (make_plan(g, prec, flags, DBM, &sp) || !make_stem_plan(g, act_dtype, prec, sp, &stp) ||
      !make_stem_pool_plan(g, act_dtype, prec, sp, &spp))
    return 0;
  if (Hq) *Hq = spp.Hq;
  if (Wq) *Wq = spp.Wq;
  return 1;
}

size_t btx_contract_workspace_bytes(const BtxGeom* g, int kind, int act_dtype, int prec, uint32_t flags) {
  Plan a, b;
  if (!g || make_plan(g, prec, flags, BM, &a) || make_plan(g, prec, flags, DBM, &b)) return 0;
  if (kind == BTX_KIND_LRT) return 0;  // no weight tiles, K never split: no partial sums either
  const int lanes = (int)plan_lanes(flags);
  // which kernel runs also depends on pointer alignment: the largest need of every plan the request can take
  auto with_tiles = [&](const Plan& pl) {
    return pad256(plan_ws(pl, g, lanes)) + patch_wt_bytes(pl, g, BTX_KIND_FLIPOUT, prec, nullptr, lanes);
  };
  auto raise = [](size_t& w, size_t v) { if (v > w) w = v; };
  size_t wa = plan_ws(a, g, lanes);
  raise(wa, with_tiles(b));
  Plan b4;
  if (!make_plan(g, prec, flags, 256, &b4)) raise(wa, with_tiles(b4));
  Plan c;
  PatchPlan pt;
  if (make_patch_plan(g, act_dtype, prec, flags, &c, &pt) || make_patch2_plan(g, act_dtype, prec, flags, &c, &pt)) {
    raise(wa, with_tiles(c));
    // the wide Reparameterization tile halves the grid and may split K differently
    if ((make_patch_plan(g, act_dtype, prec, flags, &c, &pt, BTX_KIND_REPARAM) ||
         make_patch2_plan(g, act_dtype, prec, flags, &c, &pt, BTX_KIND_REPARAM)) && pt.wide)
      raise(wa, with_tiles(c));
  }
  return wa;
}

int btx_contract_plan_info(int kind, const BtxGeom* g, int act_dtype, int prec, uint32_t flags, const BtxEpilogue* ep,
                           BtxPlanInfo* out) {
  if (!g || !out) return BTX_E_NULL;
  memset(out, 0, sizeof(*out));
  FwdSel s;
  const int rc = select_fwd(kind, g, act_dtype, prec, flags, false, nullptr, ep, &s);
  if (rc) return rc;
  out->family = s.family;
  out->ksplits = s.pl.ksplits;
  out->kper = s.pl.kper;
  out->kgroups = s.pt.kg;
  out->wide = s.pt.wide;
  out->tall = s.pt.tall;
  out->par_major = s.par_major;
  out->pool_band = s.spp.PB;
  out->nwg = s.pl.nwg;
  out->lanes = (int32_t)plan_lanes(flags);
  out->ws_bytes = (uint64_t)s.need;
  return 0;
}

size_t btx_sampled_w_bytes(const BtxGeom* g, int kind, int prec) { return btx_sampled_w_bytes_lanes(g, kind, prec, 1); }

size_t btx_sampled_w_bytes_lanes(const BtxGeom* g, int kind, int prec, int lanes) {
  Plan pl;
  if (!g || lanes < 1 || lanes > 255 || make_plan(g, prec, 0, DBM, &pl)) return 0;
  size_t one = 0;
  const size_t tiles = patch_wt_bytes(pl, g, kind, prec, &one, lanes);
  // Flipout: + the sigma cache (f32 per weight, tile order) behind the tiles — what BTX_SAMPLE_SKIP_MU reads instead of rho
  return tiles + (kind == BTX_KIND_FLIPOUT ? one * (prec == BTX_PREC_BF16 ? 2 : 1) : 0);
}

}  // extern "C"
