/* btx_attn_train.h — fused multi-head attention training: the forward of btx_attn_fwd that also keeps one scalar per
 * query (csrc/btx_attn.hip), and the flash-attention backward (csrc/btx_attn_bwd.hip).  Part of libbtx.so, declared apart from btx.h
 * and btx_attn.h: the entry points below are an addition to ABI 9, bound by bayesian_torch_amd/_lib.py through its table
 * EXPORTS_ATTN_TRAIN.  Conventions, layouts, masks, D and prec as in btx_attn.h; argument errors return before anything is launched
 * with btx_attn_fwd's checks and codes; no allocation, no memset, no host read: capturable.  No T x T tensor exists in either direction.
 *
 * btx_attn_fwd_train: btx_attn_fwd's arguments plus
 *   lse        [rows][heads][Tq] f32: L_i = log2 sum_j exp2(c s_ij), c = scale * log2 e, s_ij the unscaled score q_i . k_j over the
 *              keys query i sees; +inf for a query whose keys are all masked.  `out` is bit for bit btx_attn_fwd's.
 *
 * btx_attn_bwd is the backward of one btx_attn_fwd_train call with the SAME q, k, v, masks, scale and prec.  With
 * P_ij = exp2(c s_ij - L_i) (a masked entry is exactly 0, by select):
 *   delta_i = dO_i . O_i      dV_j = sum_i P_ij dO_i      dP_ij = dO_i . V_j      dS_ij = P_ij (dP_ij - delta_i)
 *   dQ_i = scale * sum_j dS_ij K_j                        dK_j = scale * sum_i dS_ij Q_i
 * Two launches on `stream`: the dQ pass (one workgroup per (row, head, 128 queries); it also writes delta), then the dK / dV pass
 * (one workgroup per (row, head, 128 keys)).  Every sum runs in a fixed order, no atomics: two calls give the same bits.  Every
 * element of dq, dk and dv is written (zeros for padded keys and for queries whose keys are all masked): the buffers need no clearing.
 *   q, k, v, out, d_out, dq, dk, dv   act_dtype; element (r, t, h, d) of tensor x at X + r*strides[2x] + t*strides[2x+1] + h*D + d,
 *              x = 0 (q), 1 (k), 2 (v), 3 (out), 4 (d_out), 5 (dq), 6 (dk), 7 (dv).  One packed gradient buffer [rows, T, 3E] is
 *              written in place (dq at +0, dk at +E, dv at +2E).  The gradients must not overlap any input.
 *   lse        what btx_attn_fwd_train wrote
 *   delta      [rows][heads][Tq] f32 workspace: written by the first pass, read by the second
 *   prec       BTX_PREC_F32, or BTX_PREC_BF16 (q, k, v, P, dO and dS rounded to bf16 once as MFMA operands, delta taken from that
 *              rounded dO; S, dP, delta and all accumulators f32); BTX_PREC_BF16X3: BTX_E_UNSUPPORTED */
#pragma once
#include "btx_attn.h"

#ifdef __cplusplus
extern "C" {
#endif

int btx_attn_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int rows, int Tq, int Tk, int heads,
                       int D, const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale,
                       int act_dtype, int prec, void* stream);
int btx_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out, const float* lse, float* delta,
                 void* dq, void* dk, void* dv, int rows, int Tq, int Tk, int heads, int D, const int64_t strides[16],
                 const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype, int prec, void* stream);

#ifdef __cplusplus
}
#endif
