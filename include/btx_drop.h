/* btx_drop.h — BTX-DROP v1: Monte-Carlo dropout on BTX-RNG v1.  Part of libbtx.so (csrc/btx_drop.hip), declared apart
 * from btx.h: the entry points below are an addition to ABI 9, bound by bayesian_torch_amd/_lib.py through its table EXPORTS_DROP.
 * Conventions as in btx.h: extern "C", plain pointers and scalars, 0 on success, > 0 a hipError_t, < 0 a BTX_E_* argument error.
 *
 * The keep decision of element index i (64-bit) of a layer with BTX-RNG key (seed, sample_idx, layer_id):
 *   g = i >> 3 (must fit 32 bits)         P = Philox4x32-10(counter (g, sample_idx, layer_id, BTX_STREAM_DROP), key (seed_lo, seed_hi))
 *   h = (P.x[(i >> 1) & 3] >> (16 * (i & 1))) & 0xffff          sixteen bits per element, eight elements per Philox call
 *   kept iff h < T, T in [0, 65536]:  out = round_to_act_dtype(f32(x) * scale)  (one f32 multiply, one rounding; RNE for bf16)
 *   dropped:                          out = +0.0 BY SELECTION (a dropped inf / NaN gives 0)
 * T and scale come from the caller (T = clamp(floor((1 - p) * 65536 + 0.5), 0, 65536), scale = f32(65536.0 / T), 0 when T = 0).
 *
 * The tensor of one lane is logically [N][S][C] (examples, spatial positions, channels; a 2-D [B, F] tensor is N = B, S = 1, C = F).
 *   mode   BTX_DROP_ELEMENT  i = (n * S + s) * C + c, the element's position in channels-last order whatever the memory layout
 *          BTX_DROP_CHANNEL  i = n * C + c: one decision for every spatial position of channel c of example n
 *   layout BTX_DROP_CL       memory order [N][S][C]  (offset = (n * S + s) * C + c)
 *          BTX_DROP_NCS      memory order [N][C][S]  (offset = (n * C + c) * S + s): every element derives its index, no speed promised
 * lanes = L >= 1 MC samples: `out` holds L tensors of N * S * C elements back to back; lane l draws at the sample index
 *   rng->sample_idx + l, or rng->sample_idx_dev[l] when given (L consecutive words, read by the kernel: capturable).
 *   in_rows = L * N: x holds L tensors back to back as well.  in_rows = N: x is ONE tensor every lane reads (broadcast).
 *   Anything else: BTX_E_SHAPE.  out may alias x unless x is broadcast to more than one lane.
 * Launches one kernel and nothing else: no memset, no allocation, no host read.  Any pointer aligned to its element is accepted:
 *   lanes on the 16-byte grid take 16-byte accesses, the others (and the last N * S * C % 8 elements of a lane) element-wise
 *   ones with the same bits; BTX_E_ALIGN is returned only for a pointer off its element's own alignment.
 * Errors, all before anything is launched: BTX_E_NULL (x, out, rng), BTX_E_DTYPE (act_dtype), BTX_E_UNSUPPORTED (unknown mode or
 *   layout, N * S * C > 2^35, lanes > 65535), BTX_E_SHAPE (N, C, S, lanes < 1, T > 65536, in_rows). */
#pragma once
#include "btx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BTX_DROP_ELEMENT 0
#define BTX_DROP_CHANNEL 1
#define BTX_DROP_CL  0
#define BTX_DROP_NCS 1
#define BTX_DROP_CHUNK 8192            /* elements of one lane a workgroup owns */
#define BTX_DROP_MAX_ELEMENTS (1ull << 35)

int btx_dropout_fwd(const void* x, void* out, int act_dtype, int64_t N, int64_t C, int64_t S, int mode, int layout,
                    uint32_t T, float scale, int lanes, int64_t in_rows, const BtxRng* rng, void* stream);

/* dx = drop(dy) with the mask of the forward, regenerated from the key (nothing is saved): btx_dropout_fwd of one lane on dy.
 * dx may alias dy. */
int btx_dropout_bwd(const void* dy, void* dx, int act_dtype, int64_t N, int64_t C, int64_t S, int mode, int layout,
                    uint32_t T, float scale, const BtxRng* rng, void* stream);

#ifdef __cplusplus
}
#endif
