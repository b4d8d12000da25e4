/* btx_gru.h — fused Bayesian GRU inference (GRUReparameterization / GRUFlipout).  Part of libbtx.so
 * (csrc/btx_gru.hip), declared apart from btx.h: the entry points below are an addition to ABI 9, bound by
 * bayesian_torch_amd/_lib.py through its table EXPORTS_GRU.  Conventions as in btx.h: extern "C", plain pointers and scalars,
 * 0 on success, > 0 a hipError_t, < 0 a BTX_E_* argument error.
 *
 * The cell, gate rows in torch's order (r, z, n) — row q*H + j of a [3H][K] weight is gate q of hidden unit j:
 *   gi = x_t . W_ih(s+t)^T + b_ih(s+t)          gh = h_{t-1} . W_hh(s+t)^T + b_hh(s+t)
 *   r = sigm(gi_r + gh_r)    z = sigm(gi_z + gh_z)    n = tanh(gi_n + r * gh_n)    h_t = (1 - z) * n + z * h_{t-1}
 * (b_hn is part of gh_n: it sits inside the product with r, as in torch.nn.GRU.)
 *
 * One call is 1 + T launches on `stream`: the input projection gi of every (lane, step) pair at once into the workspace, then one
 * recurrent step launch per time step that samples its rows of W_hh in registers, contracts h_{t-1}, keeps the three recurrent
 * sums apart from gi until the gates are formed, and writes h_t into hidden_seq[:, t].  Step t of a layer draws the noise of a
 * Linear forward of that layer with sample index s + t (s = sample_idx + lane, or the lane's word sample_idx_dev[lane]; the word
 * is read by the kernels, so a captured sequence replays any sample): eps_w element n*Kr + k (Kr = K rounded up to 8 when
 * K % 8 != 0), eps_b element n, s_in element b*Kr + k of the lane's own input, s_out element b*3H + n.  A lane is bit for bit
 * the single-lane call with that lane's index.
 *   ih, hh     BtxLstmLayer (btx.h): mu_w / rho_w [3H][K] f32 (K = I for ih, H for hh), mu_b / rho_b [3H] or both NULL
 *   x          [rows][T][I] in act_dtype; rows = B (x_shared: every lane reads it) or lanes*B (lane l's rows at l*B)
 *   h0         [lanes*B][H] in act_dtype, or NULL (zeros)
 *   hidden_seq [lanes*B][T][H] in act_dtype, fully written; h_T is hidden_seq[:, T-1]
 *   kl_ih, kl_hh, kl_out: optional f32 scalars; kl_out = the per-step KL terms summed over T steps in the eager order
 *   prec       BTX_PREC_F32, or BTX_PREC_BF16 (operands rounded to bf16 once, exact products, f32 accumulation);
 *              BTX_PREC_BF16X3: BTX_E_UNSUPPORTED
 *   workspace  btx_gru_workspace_bytes(lanes, B, H, T) bytes (gi [lanes][T][B][3H] f32), written before it is read
 * Any pointer aligned to its element is accepted (every access is element-wise).  lanes in [1, 255].  No memset, no allocation,
 * no host read.  Argument errors return before anything is launched. */
#pragma once
#include "btx.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t btx_gru_workspace_bytes(int lanes, int B, int H, int T);
int btx_gru_fwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                const void* h0, void* hidden_seq, const float* kl_ih, const float* kl_hh, float* kl_out, int lanes, int B,
                int I, int H, int T, int act_dtype, int prec, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
