/* btx_attn.h — fused multi-head attention forward (MultiheadAttentionReparameterization / MultiheadAttentionFlipout, DESIGN.md
 * §30).  Part of libbtx.so (csrc/btx_attn.hip), declared apart from btx.h: the entry point below is an addition to ABI 9, bound by
 * bayesian_torch_amd/_lib.py through its table EXPORTS_ATTN.  Conventions as in btx.h: extern "C", plain pointers and scalars,
 * 0 on success, > 0 a hipError_t, < 0 a BTX_E_* argument error.
 *
 *   out[r, i, h*D + d] = sum_j softmax_j(scale * q[r, i, h*D + :] . k[r, j, h*D + :]) * v[r, j, h*D + d]
 *
 * One launch on `stream`, one workgroup per (row, head, tile of 128 queries): flash attention with an online softmax over key tiles,
 * the score matrix never reaches memory.  No workspace, no allocation, no memset, no host read: capturable.
 *   q, k, v, out   act_dtype (BTX_ACT_F32 | BTX_ACT_BF16); element (r, t, h, d) of tensor X at X + r*strides[2x] + t*strides[2x+1]
 *                  + h*D + d with x = 0 (q), 1 (k), 2 (v), 3 (out): strides in ELEMENTS, the D elements of a head contiguous.  One
 *                  packed in-projection output [rows, T, 3E] is read in place (q at +0, k at +E, v at +2E), and so is a
 *                  [T, rows, E] layout.  Any pointer aligned to its element is accepted: a tensor whose base and strides are
 *                  multiples of 16 bytes is read / written with 16-byte accesses, every other one element by element, same bits.
 *   key_pad        [pad_rows][Tk] bytes, non-zero = the key is masked, or NULL; row r reads mask row r % pad_rows (MC lanes share
 *                  the batch's mask: rows = lanes * pad_rows)
 *   causal         1: key j is masked for query i when j > i
 *   scale          multiplies the scores in f32 (head_dim ** -0.5 for torch's attention)
 *   prec           BTX_PREC_F32 (v_mfma_f32_32x32x2_f32), BTX_PREC_BF16 (q, k, v and the probabilities rounded to bf16 once,
 *                  v_mfma_f32_32x32x16_bf16, f32 accumulation; the maximum, the sum and the output accumulators are f32 in both);
 *                  BTX_PREC_BF16X3: BTX_E_UNSUPPORTED
 * D in {32, 64, 128} (else BTX_E_UNSUPPORTED); rows, Tq, Tk, heads >= 1 (BTX_E_SHAPE).  A masked key contributes exactly 0 whatever
 * bits its k / v rows hold (key_pad and keys >= Tk: their rows are never multiplied; causal: p = 0 exactly).  A query whose keys
 * are all masked stores zeros.  Argument errors return before anything is launched. */
#pragma once
#include "btx.h"

#ifdef __cplusplus
extern "C" {
#endif

int btx_attn_fwd(const void* q, const void* k, const void* v, void* out, int rows, int Tq, int Tk, int heads, int D,
                 const int64_t strides[8], const uint8_t* key_pad, int pad_rows, int causal, float scale, int act_dtype, int prec,
                 void* stream);

#ifdef __cplusplus
}
#endif
