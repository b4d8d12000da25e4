/* btx_gru_train.h — fused Bayesian GRU training (GRUReparameterization / GRUFlipout): the forward of btx_gru_fwd
 * that also keeps what the backward needs (csrc/btx_gru.hip), and the backward through time (csrc/btx_gru_bwd.hip).  Part of
 * libbtx.so, declared apart from btx.h and btx_gru.h: the entry points below are an addition to ABI 9, bound by
 * bayesian_torch_amd/_lib.py through its table EXPORTS_GRU_TRAIN.  Conventions as in btx_gru.h: extern "C", 0 on success, > 0 a
 * hipError_t, < 0 a BTX_E_* argument error; argument errors return before anything is launched; no allocation, no memset, no
 * host read; any pointer aligned to its element is accepted.  Both entries serve one lane (lanes are an inference feature).
 *
 * The cell and the noise contract are those of btx_gru.h (gate rows r, z, n; step t of a layer uses sample index s + t, s =
 * sample_idx or the word sample_idx_dev[0], read on the device).
 *   saved      [T][B][4H] f32, planes r_t, z_t, n_t (post-activation) and gh_n,t (the recurrent sum of the n row, bias and
 *              Flipout perturbation included): element ((t*B + b)*4 + q)*H + j.  btx_gru_train_saved_bytes(B, H, T) bytes.
 *   workspace  btx_gru_train_workspace_bytes(B, H, T) bytes for the forward, and again for the backward (the gate gradients dG
 *              [T][B][4H] f32, then 256-byte aligned the f32 carry dh_t * z_t [B][H]); the two need not be the same buffer.
 * btx_gru_fwd_train: hidden_seq and kl_out are bit for bit those of btx_gru_fwd with lanes = 1 and the same arguments.
 * btx_gru_bwd is the backward of one btx_gru_fwd_train call with the SAME arguments (layers, seed, sample indices, x, h0,
 * hidden_seq, saved).  For t = T-1 .. 0, in f32:
 *   dh_t  = d_hidden_seq[:, t] + dh_{t+1} * z_{t+1} + dgh_{t+1} . W_hh(s+t+1)          (no carry for t = T-1)
 *   da_n  = dh_t (1 - z_t)(1 - n_t^2)    da_z = dh_t (h_{t-1} - n_t) z_t (1 - z_t)    da_r = da_n gh_n,t r_t (1 - r_t)
 *   dgi_t = (da_r, da_z, da_n)           dgh_t = (da_r, da_z, da_n r_t)
 * dG holds the planes da_r, da_z, da_n, da_n*r: the input half (dx, the ih gradients) reads planes 0, 1, 2, the recurrent half
 * (the carry, dh0, the hh gradients) planes 0, 1, 3.  Launches: T step launches, one for dh0 when wanted, one input-gradient
 * launch for all steps when dx is wanted, one weight-gradient launch per layer whose grads are given.  The kernels regenerate
 * every noise element with the forward's indices.  Every sum runs in a fixed order (no atomics): two calls give the same bits.
 *   d_hidden_seq [B][T][H] in act_dtype, nullable (zeros)
 *   dx [B][T][I], dh0 [B][H] in act_dtype, each nullable (not computed); dh0 of a call without h0: the gradient at the zero state
 *   g_ih, g_hh  BtxLstmGrads (btx.h), each nullable: dmu_w / drho_w [3H][K] f32, dmu_b / drho_b [3H] f32 (both NULL, or both
 *              given; given for a layer without bias: BTX_E_NULL).  drho = (sum_t dW_t * eps_t) * sigmoid(rho); Flipout:
 *              dDelta_t = (dg_t o s_out)^T (in_t o s_in) in that sum.
 *   prec       BTX_PREC_F32, or BTX_PREC_BF16 (the operands the forward rounds — x, h, the sampled W / mu / Delta — rounded to
 *              bf16, gradients and accumulation in f32); BTX_PREC_BF16X3: BTX_E_UNSUPPORTED */
#pragma once
#include "btx_gru.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t btx_gru_train_saved_bytes(int B, int H, int T);
size_t btx_gru_train_workspace_bytes(int B, int H, int T);
int btx_gru_fwd_train(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, const void* h0,
                      void* hidden_seq, const float* kl_ih, const float* kl_hh, float* kl_out, int B, int I, int H, int T,
                      int act_dtype, int prec, void* workspace, size_t ws_bytes, void* saved, size_t saved_bytes, void* stream);
int btx_gru_bwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, const void* h0,
                const void* hidden_seq, const void* saved, const void* d_hidden_seq, void* dx, void* dh0,
                const BtxLstmGrads* g_ih, const BtxLstmGrads* g_hh, int B, int I, int H, int T, int act_dtype, int prec,
                void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
