// btx_dw.hip — the depthwise family (btx_contract_dw.h, btx_contract_dw_wgrad.h, BTX-DW v1): its kernels and their launchers.  gfx950 only.
#include <string.h>
#include "btx_contract_dw.h"
#include "btx_contract_dw_wgrad.h"

namespace btx {

int launch_contract_dw(int kind, int act_bf16, const ContractParams& p, int nwg, hipStream_t st) {
  return act_bf16 ? launch_contract_dw_impl<__bf16>(kind, p, nwg, st) : launch_contract_dw_impl<float>(kind, p, nwg, st);
}

int launch_dw_wgrad(int kind, int act_bf16, const BtxGeom* g, const DwWgradPlan& w, const void* x, const void* dy, float* dw_mu,
                    float* dw_delta, float* slab, const BtxRng* rng, int swap, hipStream_t st) {
  DwWgradParams p;
  memset(&p, 0, sizeof(p));
  int32_t Do, Ho, Wo;
  int rc = btx_out_shape(g, 0, &Do, &Ho, &Wo);
  if (rc) return rc;
  p.x = x; p.dy = dy; p.out_m = dw_mu; p.out_d = dw_delta; p.slab = slab;
  p.NB = g->NB; p.H = g->H; p.W = g->W; p.C = g->C; p.Ho = Ho; p.Wo = Wo; p.KH = g->KH; p.KW = g->KW; p.T = g->KH * g->KW;
  p.sh = g->sh; p.sw = g->sw; p.ph = g->ph; p.pw = g->pw; p.dh = g->dh; p.dw = g->dw;
  p.TH = w.TH; p.TW = w.TW; p.PW = w.PW; p.rtiles = w.rtiles; p.ctiles = w.ctiles; p.cblocks = w.cblocks; p.ngrp = w.ngrp;
  p.tiles = w.tiles; p.tps = w.tps; p.direct = w.slabs == 1 ? 1 : 0;
  sign_keys(rng, swap ? BTX_STREAM_SIGN_OUT : BTX_STREAM_SIGN_IN, &p.kin_a, &p.kin_b);
  sign_keys(rng, swap ? BTX_STREAM_SIGN_IN : BTX_STREAM_SIGN_OUT, &p.kout_a, &p.kout_b);
  p.sample_ptr = rng->sample_idx_dev; p.seed_lo = (uint32_t)rng->seed; p.seed_hi = (uint32_t)(rng->seed >> 32); p.layer = rng->layer_id;
  p.swap = swap ? 1 : 0;
  p.fd_cblocks = make_fastdiv((uint32_t)w.cblocks); p.fd_ngrp = make_fastdiv((uint32_t)w.ngrp);
  p.fd_ctiles = make_fastdiv((uint32_t)w.ctiles); p.fd_rtiles = make_fastdiv((uint32_t)w.rtiles);
  p.fd_TW = make_fastdiv((uint32_t)w.TW); p.fd_PW = make_fastdiv((uint32_t)w.PW);
  return act_bf16 ? launch_dw_wgrad_impl<__bf16>(kind, w.form, p, w.nwg, w.lds, st)
                  : launch_dw_wgrad_impl<float>(kind, w.form, p, w.nwg, w.lds, st);
}

}  // namespace btx
