// btx_plan.h — the host-side planner of the contractions: which kernel family a request runs on, its tile shape and its K split.
// Plain C++ (no HIP include): btx_plan.cpp compiles with the host compiler alone, and the kernels read the tile constants
// they share with the planner from here (btx_contract.h includes this header).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/btx.h"

namespace btx {

constexpr int BM = 256;        // pixels per workgroup tile
constexpr int BN = 64;         // output channels per workgroup tile
constexpr int NG = 4;          // granule rows per K-stage
constexpr int DBM = 512;       // pixels per workgroup tile of the LDS-DMA variant (btx_contract_dma.h), 8-wave blocks (one per CU)

// patch variant (btx_contract_patch.h)
constexpr int PT_WD = 4;  // depth of the weight-tile ring: W(s+3) is fetched while stage s multiplies and s+1 is read
constexpr int PT_EP_ROW = 272;
constexpr int PT_EP_WAVE = 64 * PT_EP_ROW;  // 17408: epilogue staging per wave
constexpr int PT_MAXNI = 8;  // 1-KiB DMA instructions per wave per patch slot (host plan keeps pieces <= NW * 8)

// Workgroup slots the split-K cost models fill, whatever the block size.  For 4-wave blocks, 512 (two per CU) minimises the
// latency of a single launch on an otherwise idle GPU (ResNet18 layer3: 63.5 vs 69.8 us); 256 splits K half as often, which
// wins as soon as several MC samples are in flight (mc.GraphedMC lanes, the bench default: 1.16 -> 1.22 k MC-samples/s)
// because the partial sums cost HBM traffic and a reduce launch while the other samples fill the idle CUs anyway.
constexpr long long SLOTS = 256;
constexpr double TALL_MIN_GAIN = 1.15;  // the gain in pixel-slot efficiency from which tall strips are taken (make_patch_plan)
constexpr int GEMM8_MIN_K = 128;        // the shortest K that goes to the 8-wave pointwise GEMM
constexpr double WG_MAJOR_MIB = 3.0;    // the weight-tile size (MiB) from which the workgroup order turns weight-major

// tiling plan shared by btx_contract_workspace_bytes and btx_contract_fwd
struct Plan {
  int Do, Ho, Wo, Cg, Ng, M, K, mtiles, ntiles, ksplits, kper, nwg;
};

// Tile plan of the patch variant (btx_contract_patch.h): stride-1 2-D convolutions with more than one tap whose
// activations already have the contraction dtype.
struct PatchPlan {
  int G, R, Rp, Wp, PP, NI, rtiles, nw, astage, lds;
  int taps, kg, lds_g;  // tap-unrolled kernel (btx_contract_taps.h): 10*KH+KW or 0; K-groups per workgroup; LDS per group
  int wide;             // tap-unrolled kernel, Reparameterization: 64-pixel x 128-channel wave tiles, ntiles / 2 grid n-tiles
  int tall, P, Wt, ncs;  // tall-strip tiles (ContractParams.pt_tall): virtual rows per image, strip width, strips per row tile
};

// Tile plan of the stem variant (btx_contract_stem.h): row-fused small-C 2-D convolutions; R output rows x full width
// per workgroup, the input rows they need resident in LDS.
struct StemPlan {
  int R, Rp, rtiles, nw, astage, sbytes, lds, patch_bytes, nwg;
};

// Plan of the stem + max-pool variant (btx_contract_stempool.h): 8-wave workgroups, one per CU, each walking a band of
// `PB` pooled rows of one image with all weight tiles resident in LDS.  bf16 only; the pool is 3x3 / stride 2 / pad 1.
struct StemPoolPlan {
  int PB, bands, Rp, astage, sbytes, lds, patch_bytes, nwg, Hq, Wq;
};

// What contract_fwd_impl launches for a request: the kernel family, its tile plan and the workspace it needs.  The ONE copy of
// the routing rules — the launch and btx_contract_plan_info both call select_fwd, and both read the family it decided.
struct FwdSel {
  int family;     // BTX_FAMILY_*; every family from BTX_FAMILY_DMA on reads pre-sampled weight tiles (uses_tiles)
  Plan pl;        // the plan of that family
  int par_major;  // parity-major pixel order (ContractParams.par_major): BTX_FAMILY_DMA only
  int par_mqp, g8_pairs, out_bf16;
  StemPlan stp;      // BTX_FAMILY_STEM, _STEM_POOL
  StemPoolPlan spp;  // BTX_FAMILY_STEM_POOL, else zero
  PatchPlan pt;      // BTX_FAMILY_PATCH, _TAPS, _TAPS2, else zero with kg = 1
  size_t need, wt_off, wt_one, wt_all;
};
static inline bool uses_tiles(int family) { return family >= BTX_FAMILY_DMA; }

// `unaligned`: some pointer of the launch is not 16-byte aligned (granule paths refused); `noise` / `ep` as passed to the
// launch (nullable).  Lanes: BTX_FLAG_LANES(n) in flags.
int select_fwd(int kind, const BtxGeom* g, int act_dtype, int prec, uint32_t flags, bool unaligned, const BtxNoise* noise,
               const BtxEpilogue* ep, FwdSel* s);

int make_plan(const BtxGeom* g, int prec, uint32_t flags, int bm, Plan* pl);
size_t plan_ws(const Plan& pl, const BtxGeom* g, int lanes = 1);  // split-K partials [lane][split][M][N]
size_t patch_wt_bytes(const Plan& pl, const BtxGeom* g, int kind, int prec, size_t* one, int lanes = 1);

}  // namespace btx
