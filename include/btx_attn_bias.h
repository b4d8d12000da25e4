/* btx_attn_bias.h — fused multi-head attention with an additive score bias / general mask: the BIAS instantiations
 * of the kernels behind btx_attn.h and btx_attn_train.h (csrc/btx_attn.hip, csrc/btx_attn_bwd.hip).  Part of libbtx.so, declared
 * apart: the entry points below are an addition to ABI 9, bound by bayesian_torch_amd/_lib.py through its table EXPORTS_ATTN_BIAS.
 * Every argument of btx_attn_fwd / btx_attn_fwd_train / btx_attn_bwd keeps its meaning, checks and codes; the score of the pair
 * (row r, head h, query i, key j) becomes
 *
 *   scale * q_i . k_j + bias[(r % bias_rows) * bias_strides[0] + h * bias_strides[1] + i * bias_strides[2] + j]
 *
 * before the softmax, in the forward and in both backward passes (P_ij = exp2(c s_ij + b_ij log2 e - L_i), the rest as in
 * btx_attn_train.h).  The bias has no gradient here.
 *   bias          device pointer, or NULL: the call IS the entry point without a bias (the remaining bias arguments are not read)
 *   bias_dtype    BTX_BIAS_F32; BTX_BIAS_BF16 (widened exactly); BTX_BIAS_U8 (bool / uint8: non-zero = the pair is masked, -inf)
 *   bias_rows     >= 1; row r reads bias row r % bias_rows (MC lanes share the batch's bias: rows = lanes * bias_rows)
 *   bias_strides  (row, head, query) strides in ELEMENTS, each >= 0; 0 broadcasts the axis and nothing is materialised.  The key
 *                 axis is contiguous.  A bias whose base and three strides are multiples of four elements (16 / 8 / 4 bytes) is read
 *                 four keys at a time, every other one element by element, same bits.
 * -inf masks the pair; a query whose every key is masked (by -inf, key_pad or causal) stores zeros and lse = +inf, and gets zero
 * gradients.  Masks stay selects: the bias element of a pair that key_pad, causal or the tensor's end already masks is never added
 * (NaN there cannot leak), and no element with query >= Tq or key >= Tk is read.  +inf and NaN at a visible pair are the caller's.
 * Argument errors return before anything is launched: the codes of the entry point without a bias, and BTX_E_NULL (bias_strides),
 * BTX_E_SHAPE (bias_rows <= 0, a negative stride), BTX_E_DTYPE (bias_dtype), BTX_E_ALIGN (bias below its element's alignment). */
#pragma once
#include "btx_attn_train.h"

#define BTX_BIAS_F32  0
#define BTX_BIAS_BF16 1
#define BTX_BIAS_U8   2

#ifdef __cplusplus
extern "C" {
#endif

int btx_attn_bias_fwd(const void* q, const void* k, const void* v, void* out, int rows, int Tq, int Tk, int heads, int D,
                      const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype, int prec,
                      void* stream, const void* bias, int bias_dtype, int bias_rows, const int64_t bias_strides[3]);
int btx_attn_bias_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int rows, int Tq, int Tk, int heads,
                            int D, const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale,
                            int act_dtype, int prec, void* stream, const void* bias, int bias_dtype, int bias_rows,
                            const int64_t bias_strides[3]);
int btx_attn_bias_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out, const float* lse, float* delta,
                      void* dq, void* dk, void* dv, int rows, int Tq, int Tk, int heads, int D, const int64_t strides[16],
                      const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype, int prec, void* stream,
                      const void* bias, int bias_dtype, int bias_rows, const int64_t bias_strides[3]);

#ifdef __cplusplus
}
#endif
