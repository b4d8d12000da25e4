/*
 * btx.h — C-ABI of libbtx.so: the MI355X (gfx950) variational-layer forward hot path.
 *
 * This is the drop-in boundary ("C-ABI face").  The reference
 * (IntelLabs/bayesian-torch) has no FFI of its own: its boundary is the Python nn.Module surface,
 * and every entry point below replaces a *chain of ATen ops* inside one reference method.  Each
 * declaration cites the reference lines it subsumes (paths relative to /root/reference/bayesian_torch).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers / sizes / scalars, no torch types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - returns 0 on success; >0 = hipError_t from the runtime; <0 = BTX_E_* argument error.
 *   - never throws, never allocates device memory, never synchronises: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream).  The caller owns every
 *     buffer and keeps it alive until the stream has passed the call.
 *   - stateless => thread-safe for distinct streams/buffers.
 *   - workspaces (`ws`, `workspace`) and outputs may hold ANYTHING on entry: every workspace byte a call reads was written or
 *     cleared by that same call, and every output element is written — except where a declaration below says that an argument
 *     is accumulated or updated in place (BTX_FLAG_KL_ACCUM, the packed MC sums, evaluator and optimizer state, the BatchNorm
 *     running estimates); DESIGN.md §24 lists them, tests/test_gpu_poison.py holds the rule.
 *
 * Data layout:
 *   activations  channels-last: x[nb][d][h][w][c]   (f32 or bf16, `act_dtype`)
 *   weights      GEMM-major  : mu/rho[n][tap][c] f32, tap = (kd*KH + kh)*KW + kw, c within the group
 *                (== torch channels_last physical layout of the logical [Cout,Cin/g,k...] tensor;
 *                 for Linear it is the native [out][in]).
 *   output       channels-last: out[nb][do][ho][wo][n], same dtype as the activations.
 *
 * Noise definition (BTX-RNG v1): eps and the Flipout signs are pure functions of
 * (seed, sample_idx, layer_id, stream, logical element index) — Philox4x32-10 + Box–Muller for eps,
 * a keyed 32-bit mixer for the 1-bit signs — so a regenerated tile is identical in every workgroup
 * and on every rank.  Passing explicit noise tensors (eps_w, eps_b, sign_in, sign_out) overrides it;
 * that is the parity mode used against torch-drawn noise.
 */
#ifndef BTX_H_
#define BTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BTX_ABI_VERSION 9

/* argument-error codes (negative) */
#define BTX_E_NULL        (-1)   /* required pointer is NULL */
#define BTX_E_SHAPE       (-2)   /* inconsistent / non-positive shape */
#define BTX_E_UNSUPPORTED (-3)   /* valid request this build does not implement */
#define BTX_E_WORKSPACE   (-4)   /* workspace too small (see btx_*_workspace_bytes) */
#define BTX_E_DTYPE       (-5)   /* unknown dtype / precision code */
#define BTX_E_ALIGN       (-6)   /* pointer not 16-byte aligned (per pointer: DESIGN.md "Alignment contract") */

/* kind */
#define BTX_KIND_REPARAM 0
#define BTX_KIND_FLIPOUT 1
#define BTX_KIND_LRT     2 /* local reparameterization (BTX-LRT v1): y = m + sqrt(v) * zeta with m = x (*) mu_w + mu_b,
                              v = x^2 (*) sigma_w^2 + sigma_b^2 and one standard normal zeta per OUTPUT element, stream
                              BTX_STREAM_OUT_NOISE at the element's linear index in the (lane's own) channels-last output tensor:
                              btx_fill_eps(out_numel, rng, BTX_STREAM_OUT_NOISE) returns the zeta of a launch bit for bit.  Forward
                              entry points only (btx_contract_fwd, _ex, _lanes), on BTX_FAMILY_REGSTAGE / _GATHER with K never split.
                              BTX_E_UNSUPPORTED: BTX_PREC_BF16X3, BTX_FLAG_ROWFUSE, BTX_FLAG_OUT_*, BtxEpilogue.pool and every
                              BtxNoise field (no weight noise exists; there is no explicit-noise mode). */
/* activation dtype */
#define BTX_ACT_F32  0
#define BTX_ACT_BF16 1
/* contraction precision */
#define BTX_PREC_F32  0   /* v_mfma_f32_32x32x2_f32: exact f32 fma chain (parity mode) */
#define BTX_PREC_BF16 1   /* v_mfma_f32_32x32x16_bf16, f32 accumulate (throughput mode) */
#define BTX_PREC_BF16X3 2 /* split-bf16: f32 activations, every operand as hi + lo bf16 (hi = rn(v), lo = rn(v - hi)), three
                             v_mfma_f32_32x32x16_bf16 per product (hi*hi + hi*lo + lo*hi), f32 accumulate: the f32 result of
                             the reference's F.conv*d / F.linear to ~1e-6 rel-L2 per layer (the tolerance north_star states is
                             1e-4) at a third of the bf16 matrix rate instead of a sixteenth.  Kernel family and workspace
                             sizes are those of BTX_PREC_F32; sampled-weight tiles (btx_sample_weights) are specific to it.
                             RANGE: operands must be finite and below the bf16 maximum (|v| < 3.39e38): for +-inf, or a
                             value whose hi rounds to inf, lo = rn(v - hi) = inf - inf = NaN and the product is NaN where the
                             reference's f32 convolution gives inf or a finite value (the split is not guarded: it sits in
                             the fragment-read path of the hot loop).  BTX_PREC_F32 has no such limit. */
/* flags */
#define BTX_FLAG_TRANSPOSED   1u  /* ConvTranspose gather rule */
#define BTX_FLAG_KL_ACCUM     2u  /* btx_kl_gauss: add to *kl_out instead of overwriting */
#define BTX_FLAG_ROWFUSE      4u  /* small-C stems: the KW taps of a kernel row are contiguous with the channels in
                                     memory (C*KW elements per row), so one K-stage = one kernel row.  Needs
                                     groups=1, dil_w=1, pad_w=0 (padding materialised by the caller), C*KW a multiple
                                     of the stage (32 bf16 / 16 f32 elements), activation dtype == precision dtype;
                                     returns BTX_E_UNSUPPORTED otherwise. */
#define BTX_FLAG_OUT_F32      8u  /* store the output as f32 / bf16 regardless of act_dtype (LDS-DMA kernels only: lets */
#define BTX_FLAG_OUT_BF16    16u  /* a caller that had to copy the input anyway keep "f32 in/out, bf16 MFMA" semantics) */
#define BTX_FLAG_SWAP_SIGNS  64u  /* Flipout: hash the INPUT signs from stream SIGN_OUT and the OUTPUT signs from stream
                                     SIGN_IN.  The data gradient of a Flipout layer is itself a Flipout-shaped contraction,
                                     dx = convT(dy, mu) + s_in * convT(dy * s_out, sigma*eps): the same entry point computes
                                     it on the transposed (or flipped) geometry with the two sign streams exchanged. */
#define BTX_FLAG_CONCURRENT 128u  /* hint: other launches run beside this one (several MC samples in flight on their own
                                     streams): plan for device throughput — CU-time — rather than for the latency of this
                                     launch, i.e. do not split K through HBM just to fill idle CUs */
#define BTX_FLAG_REVERSE    256u  /* walk the launch's workgroup tiles in DESCENDING order.  Results are identical (no launch
                                     depends on its block order); a caller that chains layers alternates the flag so that each
                                     launch starts on the activations its producer wrote LAST — the ones most likely still in
                                     the 256-MB Infinity Cache when the tensors of a launch (MC sample lanes: hundreds of MB)
                                     exceed it. */
#define BTX_FLAG_GATHER      32u  /* force the element-wise gather kernel (any shape / alignment; samples in registers).
                                     The library picks it by itself whenever a fast kernel does not apply; the flag
                                     exists so tests can exercise it on shapes the fast kernels would take. */

/* MC sample lanes (btx_contract_fwd_lanes): n independent Monte-Carlo samples of the SAME layer in one launch.  Whoever
 * asks for a workspace size or a pool shape for such a launch ORs BTX_FLAG_LANES(n) into the flags (the entry point sets
 * it from BtxLanes.n itself). */
#define BTX_FLAG_LANES_SHIFT 16
#define BTX_FLAG_LANES_MASK  (0xffu << BTX_FLAG_LANES_SHIFT)
#define BTX_FLAG_LANES(n)    (((uint32_t)(n) & 0xffu) << BTX_FLAG_LANES_SHIFT)

/* RNG streams of BTX-RNG v1 */
#define BTX_STREAM_EPS_W    0u
#define BTX_STREAM_EPS_B    1u
#define BTX_STREAM_SIGN_IN  2u
#define BTX_STREAM_SIGN_OUT 3u
#define BTX_STREAM_OUT_NOISE 4u /* BTX_KIND_LRT: the per-output-element normal zeta */
#define BTX_STREAM_DROP 7u      /* BTX-DROP v1: the keep bits of the dropout layers (include/btx_drop.h) */

/* Geometry of one variational contraction.  Linear is the 1x1x1 case: NB=batch, D=H=W=1, C=in_features,
 * KD=KH=KW=1, N=out_features.  Conv1d uses H only... by convention lower-rank convs put their axes last
 * (Conv1d: D=H=1, W=L;  Conv2d: D=1). */
typedef struct BtxGeom {
  int32_t NB, D, H, W, C;        /* input  [NB][D][H][W][C]  (C = total input channels) */
  int32_t N;                     /* total output channels */
  int32_t KD, KH, KW;            /* kernel taps */
  int32_t sd, sh, sw;            /* stride */
  int32_t pd, ph, pw;            /* padding */
  int32_t dd, dh, dw;            /* dilation */
  int32_t od, oh, ow;            /* output_padding (transposed only; else 0) */
  int32_t groups;
} BtxGeom;

typedef struct BtxRng {
  uint64_t seed;
  uint32_t sample_idx;           /* global Monte-Carlo sample index */
  uint32_t layer_id;
  const uint32_t* sample_idx_dev; /* optional DEVICE pointer: when non-NULL the kernels read the sample index from it
                                     when they run and sample_idx is ignored.  This is what lets one captured hipGraph
                                     of a whole MC forward be replayed for successive samples (update the word, replay):
                                     no per-launch host work in the Monte-Carlo loop.  Honoured by every entry point that
                                     takes a BtxRng except btx_fill_sign (ABI 7: also btx_contract_wgrad, btx_rho_grad,
                                     btx_fill_eps, btx_dgrad_weights — a whole TRAINING step can be captured). */
} BtxRng;

/* Optional explicit noise (parity mode).  Any member may be NULL => generated by BTX-RNG v1.
 *   eps_w   f32, same layout as mu_w ([N][tap][c])
 *   eps_b   f32 [N]
 *   sign_in  int8 (+1/-1), same layout as x      (Flipout only)
 *   sign_out int8 (+1/-1), same layout as out    (Flipout only) */
typedef struct BtxNoise {
  const float*  eps_w;
  const float*  eps_b;
  const int8_t* sign_in;
  const int8_t* sign_out;
  const void*   sampled_w;   /* weight tiles filled by btx_sample_weights for the same (seed, sample_idx, layer_id,
                                kind, prec, geometry): the launch skips its own sampling pre-pass.  Not explicit noise:
                                the values are BTX-RNG v1's.  Ignored by the kernels that sample in-register. */
} BtxNoise;

int         btx_abi_version(void);
const char* btx_strerror(int code);

/* K1. Mean Gaussian KL(q||p) of one parameter tensor, sigma_q = log1p(exp(rho)).
 * Replaces: BaseVariationalLayer_.kl_div  layers/base_variational_layer.py:53-68  and the softplus in
 * *.kl_loss()  (layers/variational_layers/linear_variational.py:144-155, layers/flipout_layers/conv_flipout.py:362-368).
 * prior_mu_t / prior_sigma_t: optional full-shape prior tensors (utils/util.py:102-117 MOPED overwrites
 * them); when NULL the scalars are used.  kl_out: 1 float, overwritten (or += with BTX_FLAG_KL_ACCUM).
 * Deterministic two-pass reduction; ws must hold btx_kl_workspace_bytes(n). */
size_t btx_kl_workspace_bytes(size_t n);
int btx_kl_gauss(const float* mu, const float* rho, size_t n,
                 const float* prior_mu_t, const float* prior_sigma_t,
                 float prior_mu, float prior_sigma,
                 float* kl_out, uint32_t flags, void* ws, size_t ws_bytes, void* stream);

/* K1b. KL of a whole model in one launch (+ one final reduce), and its gradient.
 * Replaces get_kl_loss  models/dnn_to_bnn.py:157-165  (sum over modules of the per-tensor MEANS) and, for training
 * (README.md:114-125: loss = ce + kl / batch_size), the autograd graph torch builds through base_variational_layer.py:53-68:
 *   d kl / d mu  = (mu - mu_p) / (sigma_p^2 n)        d kl / d rho = (sigma / sigma_p^2 - 1 / sigma) * sigmoid(rho) / n
 * items_host is a HOST array read before the call returns; mu/rho (and dmu/drho of the backward) are device pointers of
 * n floats in any element order (the terms are elementwise), prior tensors optional as in btx_kl_gauss.
 * grad_out: DEVICE pointer to the upstream gradient scalar (no host sync). */
typedef struct BtxKlItem {
  const float* mu;
  const float* rho;
  const float* prior_mu_t;     /* nullable */
  const float* prior_sigma_t;  /* nullable */
  float*       dmu;            /* backward only */
  float*       drho;           /* backward only */
  float        prior_mu, prior_sigma;
  size_t       n;
} BtxKlItem;
size_t btx_kl_model_workspace_bytes(int n_items);
int btx_kl_gauss_model(const BtxKlItem* items_host, int n_items, float* kl_out, void* ws, size_t ws_bytes, void* stream);
int btx_kl_gauss_model_bwd(const BtxKlItem* items_host, int n_items, const float* grad_out, void* stream);

/* K1c. Sampled KL against a non-Gaussian weight prior (BTX-KLMC v1; csrc/btx_klmc.hip).
 * Per tensor of n elements, sigma = log1p(exp(rho)), `draws` = S >= 1:
 *   eps_j[i] = BTX-RNG v1 normal at element index i, stream rng_stream | (j << 8)   (BTX_STREAM_KL_W weights, _KL_B biases)
 *   w_j[i]   = mu[i] + sigma[i] eps_j[i]
 *   kl       = (1 / n) sum_i [ -log sigma[i] - (1 + log 2 pi) / 2 - (1 / S) sum_j log p(w_j[i]) ]     summed over the items
 * The entropy of q is closed-form, only E_q[-log p] is sampled; btx_fill_eps(n, rng, rng_stream | (j << 8)) returns eps_j bit
 * for bit.  i is the index in the order of mu / rho as handed over (the Python face hands over the unpadded GEMM-major order).
 * Backward, with s = d log p / dw and g = *grad_out:
 *   dmu[i]  = -(g / n) (1 / S) sum_j s(w_j[i])        drho[i] = (g / n) [ -1 / sigma[i] - (1 / S) sum_j s(w_j[i]) eps_j[i] ] sigmoid(rho[i])
 * Priors, d = w - loc (loc_t[i] when loc_t is given, else prior.loc):
 *   BTX_PRIOR_GAUSS_MIX2  p0 = pi in (0, 1), p1 = sigma1 > 0, p2 = sigma2 > 0:  pi N(loc, sigma1^2) + (1 - pi) N(loc, sigma2^2)
 *   BTX_PRIOR_LAPLACE     p0 = b > 0:                                           exp(-|d| / b) / (2 b)
 *   BTX_PRIOR_STUDENT_T   p0 = nu > 0, p1 = scale t > 0:                        Student-t density of d / t, over t
 * The host derives every constant in double.  One launch per 48 items plus one fixed-order final reduce (kl_out overwritten, or
 * += with BTX_FLAG_KL_ACCUM); the backward is one element-wise launch per 48 items that writes every element of dmu / drho, no
 * atomics, nothing saved.  sample_idx_dev (nullable) wins over sample_idx and is read by the kernels (captured steps).
 * Parameter and gradient pointers on any 4-byte boundary are accepted (off the 16-byte grid: scalar accesses); ws: 8-byte aligned
 * (BTX_E_ALIGN), btx_kl_mc_workspace_bytes(n_items) bytes.  Before any launch: BTX_E_NULL (a required pointer), BTX_E_SHAPE
 * (n == 0, n_items < 1, draws < 1 or >= 2^24, rng_stream >= 256, a prior parameter out of range), BTX_E_UNSUPPORTED (unknown
 * prior type, n > 0xfffffffc), BTX_E_WORKSPACE. */
#define BTX_STREAM_KL_W 5u
#define BTX_STREAM_KL_B 6u
#define BTX_PRIOR_GAUSS_MIX2 1
#define BTX_PRIOR_LAPLACE    2
#define BTX_PRIOR_STUDENT_T  3
typedef struct BtxPrior {
  int32_t type;
  float   loc, p0, p1, p2;
} BtxPrior;
typedef struct BtxKlMcItem {
  const float* mu;
  const float* rho;
  const float* loc_t;          /* nullable */
  float*       dmu;            /* backward only */
  float*       drho;           /* backward only */
  size_t       n;
  BtxPrior     prior;
  uint32_t     layer_id, rng_stream;
  uint32_t     sample_idx;
  const uint32_t* sample_idx_dev;  /* nullable; wins */
} BtxKlMcItem;
size_t btx_kl_mc_workspace_bytes(int n_items);
int btx_kl_mc_model(const BtxKlMcItem* items_host, int n_items, uint64_t seed, int draws, float* kl_out, uint32_t flags,
                    void* ws, size_t ws_bytes, void* stream);
int btx_kl_mc_model_bwd(const BtxKlMcItem* items_host, int n_items, uint64_t seed, int draws, const float* grad_out,
                        void* stream);

/* K1d. Sparse variational dropout (BTX-SVD v1; csrc/btx_svd.hip): the KL of a variational Gaussian against
 * the log-uniform prior p(|w|) ~ 1 / |w| in the approximation of Molchanov, Ashukha & Vetrov (2017, eq. 14), the log-alpha
 * statistics of a model and pruning in place.  Per tensor of n elements, sigma = log1p(exp(rho)), every step in f32:
 *   la_raw = 2 log(sigma) - log(mu^2 + 1e-8)          la = min(max(la_raw, -20), 20)          (log alpha, BTX_LOGALPHA_MAX)
 *   kl_i   = k1 - k1 sigmoid(k2 + k3 la) + 0.5 log1p(exp(-la))        k1 = 0.63576, k2 = 1.87320, k3 = 1.48695
 *   kl     = c sum_i kl_i,  c = 1 / n (BTX_REDUCE_MEAN) or 1 (BTX_REDUCE_SUM), summed over the items
 * Backward, g = *grad_out, s = sigmoid(k2 + k3 la):
 *   d      = -(k1 k3 s (1 - s) + 0.5 sigmoid(-la)), 0 where la_raw lies strictly outside [-20, 20] (NaN included)
 *   dmu[i] = g c d (-2 mu / (mu^2 + 1e-8))             drho[i] = g c d (2 sigmoid(rho) / sigma)
 * Nothing is sampled.  The terms are element-wise: mu / rho are the tensor's dense storage in any element order.  One launch per 48
 * items (the f64 partial of each block, at most 256 blocks per item), then a one-wave fold per launch: each item's partials in a
 * fixed order that depends on n alone, the items in index order, in f64; kl_out overwritten, or += with BTX_FLAG_KL_ACCUM.
 * terms_out (nullable): n_items doubles, the per-item term c sum_i kl_i — the same bits whichever call the item sits in.
 * The backward is one element-wise launch per 48 items that writes every element of dmu / drho: no atomics, nothing saved.
 * Parameter and gradient pointers on any 4-byte boundary are accepted (off the 16-byte grid: scalar accesses, same bits); ws and
 * terms_out: 8-byte aligned (BTX_E_ALIGN), btx_kl_logu_workspace_bytes(n_items) bytes.  Before any launch: BTX_E_NULL (a required
 * pointer), BTX_E_SHAPE (n == 0, n_items < 1, an unknown reduction code), BTX_E_UNSUPPORTED (n > 0xfffffffc), BTX_E_WORKSPACE.
 *
 * btx_logalpha_stats: per item BTX_LOGALPHA_STATS_WORDS uint64 words — [k] = count(la > thresholds[k]) for k < n_thresholds <=
 * BTX_LOGALPHA_MAX_THRESHOLDS (strict; the other words of [0, 8) are 0), [8] = count(mu == 0), the rest 0 — and, when bins > 0
 * (<= BTX_LOGALPHA_MAX_BINS), hist_out[item][b], b = min(bins - 1, floor((la + 20) * bins / 40)).  Integer counters: exact.
 * btx_logalpha_prune: mu = 0 and rho = BTX_RHO_PRUNED (-40: sigma = 4.2e-18, sigma^2 still a normal f32) wherever la > threshold;
 * word [0] of the item = the number of elements pruned, the other words 0.  Both clear their outputs themselves (memset nodes), are
 * capturable and accept any 4-byte boundary for mu / rho; stats_out / hist_out: 8-byte aligned (BTX_E_ALIGN).  Before any launch:
 * BTX_E_NULL, BTX_E_SHAPE (n == 0, n_items < 1, n_thresholds outside [0, 8], bins outside [0, 4096], a NaN threshold),
 * BTX_E_UNSUPPORTED (n > 0xfffffffc). */
#define BTX_REDUCE_MEAN 0
#define BTX_REDUCE_SUM  1
#define BTX_LOGALPHA_MAX 20.0f
#define BTX_RHO_PRUNED (-40.0f)
#define BTX_LOGALPHA_MAX_THRESHOLDS 8
#define BTX_LOGALPHA_MAX_BINS 4096
#define BTX_LOGALPHA_STATS_WORDS 16
typedef struct BtxKlLogUItem {
  const float* mu;
  const float* rho;
  float*       dmu;            /* backward only */
  float*       drho;           /* backward only */
  size_t       n;
  int32_t      reduction;      /* BTX_REDUCE_* */
} BtxKlLogUItem;
typedef struct BtxLogAlphaItem {
  float* mu;                   /* written by btx_logalpha_prune only */
  float* rho;
  size_t n;
} BtxLogAlphaItem;
size_t btx_kl_logu_workspace_bytes(int n_items);
int btx_kl_logu_model(const BtxKlLogUItem* items_host, int n_items, float* kl_out, double* terms_out, uint32_t flags, void* ws,
                      size_t ws_bytes, void* stream);
int btx_kl_logu_model_bwd(const BtxKlLogUItem* items_host, int n_items, const float* grad_out, void* stream);
int btx_logalpha_stats(const BtxLogAlphaItem* items_host, int n_items, const float* thresholds, int n_thresholds, int bins,
                       uint64_t* stats_out, uint64_t* hist_out, void* stream);
int btx_logalpha_prune(const BtxLogAlphaItem* items_host, int n_items, float threshold, uint64_t* stats_out, void* stream);

/* K2-K5. Fused sample-and-contract forward of one variational layer.
 * Replaces the whole body of
 *   LinearReparameterization.forward   layers/variational_layers/linear_variational.py:157-178
 *   LinearFlipout.forward              layers/flipout_layers/linear_flipout.py:145-174
 *   Conv{1,2,3}dReparameterization.forward  layers/variational_layers/conv_variational.py:183-227, 357-380, 530-574
 *   Conv{1,2,3}dFlipout.forward        layers/flipout_layers/conv_flipout.py:175-244, 370-417, 568-637
 *   ConvTranspose{1,2,3}d{Reparameterization,Flipout}.forward  conv_variational.py:577-1094, conv_flipout.py:640-1228
 * (sigma=log1p(exp(rho)); eps~N(0,1); W=mu+sigma*eps | y0=conv(x,mu)+conv(x*s_in, sigma*eps)*s_out; + bias).
 * mu_b/rho_b NULL => no bias.  The KL term of these methods is btx_kl_gauss (RNG-free).
 * ws: split-K partial sums; must hold btx_contract_workspace_bytes(...) bytes (may be 0). */
size_t btx_contract_workspace_bytes(const BtxGeom* g, int kind, int act_dtype, int prec, uint32_t flags);
int btx_contract_fwd(int kind, const BtxGeom* g,
                     const void* x, const float* mu_w, const float* rho_w,
                     const float* mu_b, const float* rho_b,
                     void* out,
                     const BtxRng* rng, const BtxNoise* noise /* nullable */,
                     int act_dtype, int prec, uint32_t flags,
                     void* ws, size_t ws_bytes, void* stream);

/* §8(f)-3, the step either side of the path: eval-mode BatchNorm (+ residual add, + ReLU) folded into the store of the
 * contraction (reference models/deterministic/resnet_large.py:49-60: out = relu(bn(conv(x)) [+ identity])).
 *   y = conv_out * scale[n] + shift[n]  (+ residual[same index as out])  ;  then the activation `relu`:
 *   relu = 0: none;  1: y = max(y, 0) (ReLU);  2: y = min(max(y, 0), 6) (ReLU6, MobileNetV2's ConvBNReLU).
 * The activation acts on the f32 value, in front of the one rounding to the output dtype; both bounds of ReLU6 are exact in
 * bf16, so relu = 2 gives exactly clamp(output of relu = 0, 0, 6).  relu = 2 with pool = 1 returns BTX_E_UNSUPPORTED.
 * scale/shift: f32 [N] (NULL => 1 / 0), read element by element; residual: same layout and dtype as `out` (NULL => none) — like
 * x, mu_w, rho_w, out and eps_w it is moved in 16-byte granules by the fast kernels: with any of them off the 16-byte grid the
 * launch takes the element-wise gather kernel (BTX_E_UNSUPPORTED where none exists: BTX_FLAG_ROWFUSE, BTX_FLAG_OUT_*).
 * pool = 1: the ResNet stem's nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (resnet_large.py:118,145) is applied to y
 * inside the same launch and `out` is the POOLED tensor [NB][Hq][Wq][N] (btx_contract_pool_shape); the conv output never
 * reaches HBM.  Row-fused bf16 stems only (BTX_FLAG_ROWFUSE, generated noise, no residual): everything else returns
 * BTX_E_UNSUPPORTED and the caller pools with btx_maxpool2d_cl.  Values are bit-identical to the two-launch chain. */
typedef struct BtxEpilogue {
  const float* scale;
  const float* shift;
  const void*  residual;
  int32_t      relu;      /* 0 none, 1 ReLU, 2 ReLU6 */
  int32_t      pool;
} BtxEpilogue;
/* 1 (and the pooled extent) when btx_contract_fwd_ex would take epilogue.pool = 1 for this geometry, else 0 */
int btx_contract_pool_shape(const BtxGeom* g, int act_dtype, int prec, uint32_t flags, int32_t* Hq, int32_t* Wq);
int btx_contract_fwd_ex(int kind, const BtxGeom* g,
                        const void* x, const float* mu_w, const float* rho_w,
                        const float* mu_b, const float* rho_b,
                        void* out,
                        const BtxRng* rng, const BtxNoise* noise /* nullable */,
                        int act_dtype, int prec, uint32_t flags,
                        void* ws, size_t ws_bytes, void* stream,
                        const BtxEpilogue* epilogue /* nullable */);

/* MC sample lanes.  The Monte-Carlo loop of the reference (examples/main_bayesian_imagenet_dnn2bnn.py:480-499:
 * `for mc_run in range(num_monte_carlo): output = model(images)`) evaluates the same layer once per sample with fresh
 * noise; on a 256-CU GPU one sample of a 7x7 or 14x14 layer is a few hundred workgroups — too few to fill the chip and
 * to overlap one workgroup's prologue / store with another's MFMA loop.  btx_contract_fwd_lanes runs `n` samples of one
 * layer in ONE launch: lane l reads x + l*x_stride (x_stride 0: the lanes share the input, e.g. the network's first
 * layer), uses the MC sample index rng->sample_idx + l (rng->sample_idx_dev[l] when given: n consecutive words) and
 * writes out + l*out_stride (residual + l*res_stride).  Strides in bytes, multiples of 16.  Every lane computes bit for
 * bit what btx_contract_fwd_ex with BTX_FLAG_CONCURRENT would for its sample (the noise indices are relative to the lane's
 * own tensors; a launch with lanes is always planned for throughput, and the K split — the f32 summation order — of that
 * plan is decided by the grid of ONE lane, so it does not depend on n).
 * noise->sampled_w: the buffer btx_sample_weights_lanes filled for the same n.  Explicit noise tensors: n == 1 only.
 * ws: btx_contract_workspace_bytes(..., flags | BTX_FLAG_LANES(n)). */
typedef struct BtxLanes {
  int32_t n;
  int64_t x_stride, out_stride, res_stride;
} BtxLanes;
int btx_contract_fwd_lanes(int kind, const BtxGeom* g,
                           const void* x, const float* mu_w, const float* rho_w,
                           const float* mu_b, const float* rho_b,
                           void* out,
                           const BtxRng* rng, const BtxNoise* noise /* nullable */,
                           int act_dtype, int prec, uint32_t flags,
                           void* ws, size_t ws_bytes, void* stream,
                           const BtxEpilogue* epilogue /* nullable */, const BtxLanes* lanes);

/* Plan introspection (ABI 9, host only: no GPU, no launch).  What btx_contract_fwd_ex (flags without BTX_FLAG_LANES) or
 * btx_contract_fwd_lanes (flags | BTX_FLAG_LANES(n)) would launch for this request — computed by the same routine the launch
 * runs, so it cannot drift from it.  Assumes every pointer of the launch 16-byte aligned, no explicit noise and no pre-sampled
 * tiles (BtxNoise NULL) and a workspace of at least ws_bytes; `ep` only matters through its pool / residual members (nullable).
 * Returns what the launch would return for an argument error or an unsupported request (BTX_E_UNSUPPORTED: the caller runs the
 * request another way — a launch with lanes, one single-sample launch per lane), else 0 and fills *out.
 * The f32 summation order of an output element is fixed by (family, ksplits, kper, kgroups, par_major); wide, tall and
 * pool_band change which workgroup computes an element, not how. */
#define BTX_FAMILY_GATHER    0  /* element-wise gather kernel (unaligned / channel-padded shapes, BTX_FLAG_GATHER) */
#define BTX_FAMILY_REGSTAGE  1  /* register-staged kernel (samples in registers) */
#define BTX_FAMILY_DMA       2  /* generic LDS-DMA kernel (btx_contract_dma.h) */
#define BTX_FAMILY_GEMM8     3  /* 8-wave pointwise GEMM (btx_contract_gemm8.h) */
#define BTX_FAMILY_PATCH     4  /* run-time-tap patch kernel (btx_contract_patch.h) */
#define BTX_FAMILY_TAPS      5  /* tap-unrolled 3x3 stride-1 kernel (btx_contract_taps.h) */
#define BTX_FAMILY_TAPS2     6  /* tap-unrolled 3x3 stride-2 kernel (btx_contract_taps2.h) */
#define BTX_FAMILY_STEM      7  /* row-fused stem (btx_contract_stem.h) */
#define BTX_FAMILY_STEM_POOL 8  /* row-fused stem + max-pool (btx_contract_stempool.h) */
typedef struct BtxPlanInfo {
  int32_t  family;     /* BTX_FAMILY_* */
  int32_t  ksplits;    /* K splits (> 1: partial sums in the workspace + one reduce launch) */
  int32_t  kper;       /* K elements per split */
  int32_t  kgroups;    /* K-groups inside one workgroup (tap-unrolled 8-wave form: 2), else 1 */
  int32_t  wide;       /* tap-unrolled Reparameterization: 64-pixel x 128-channel wave tiles */
  int32_t  tall;       /* tap-unrolled: tall-strip tiles */
  int32_t  par_major;  /* LDS-DMA transposed stride-2: parity-major pixel order */
  int32_t  pool_band;  /* stem + max-pool: pooled rows per band (PB), else 0 */
  int32_t  nwg;        /* workgroups per lane */
  int32_t  lanes;      /* MC sample lanes of the launch */
  uint64_t ws_bytes;   /* workspace the launch needs */
} BtxPlanInfo;
int btx_contract_plan_info(int kind, const BtxGeom* g, int act_dtype, int prec, uint32_t flags,
                           const BtxEpilogue* ep /* nullable */, BtxPlanInfo* out);

/* Weight gradient of one variational contraction (training; what autograd derives for the F.conv*d / F.linear calls of
 * conv_flipout.py:376-417, conv_variational.py:379-380, linear_flipout.py:168-174):
 *   dw_mu   [n][tap][c] = sum_p dy[p][n] * x[p @ tap][c]
 *   dw_delta[n][tap][c] = sum_p (dy * s_out)[p][n] * (x * s_in)[p @ tap][c]                      (Flipout only)
 *   db_mu[n] = sum_p dy[p][n],  db_delta[n] = sum_p (dy * s_out)[p][n]                            (optional, NULL = skip)
 * in the GEMM-major layout of mu_w, f32 whatever the activation dtype (exact-f32 MFMA, f32 atomics: the summation order
 * over pixel chunks is not fixed).  The outputs are cleared by the call.  x / dy: channels-last as in btx_contract_fwd,
 * dy = gradient of its output.  The Flipout signs are those of the forward with the same BtxRng (or noise->sign_in /
 * sign_out).  dmu = dw_mu and drho = dw_delta * eps * sigmoid(rho) (Reparameterization: dw_mu * eps * sigmoid(rho)) are
 * elementwise follow-ups on the caller's side.  ConvTranspose layers: call it on the plain-convolution geometry with x and
 * dy exchanged and BTX_FLAG_SWAP_SIGNS.  The data gradient needs no entry point of its own: see BTX_FLAG_SWAP_SIGNS. */
int btx_contract_wgrad(int kind, const BtxGeom* g, const void* x, const void* dy, float* dw_mu, float* dw_delta,
                       float* db_mu, float* db_delta, const BtxRng* rng, const BtxNoise* noise /* nullable */,
                       int act_dtype, uint32_t flags, void* stream);
/* The same with a workspace (ABI 8): the partial sums of the pixel chunks leave as plain stores into per-chunk slabs in `ws`
 * and a second launch adds them in chunk order — the result no longer depends on the order in which workgroups retire, and
 * no f32 atomic crosses the fabric (db_* still uses them: N values).  With a workspace the weight gradient of a stride-1
 * 3x3 "same" convolution on bf16 activations (C % 64 == 0, N % 64 == 0, W <= 63, hashed signs, no bias: the body of a
 * ResNet) takes a kernel that holds all nine taps of a 64 x 64 tile in one workgroup (csrc/btx_wgrad_taps.h): x is staged
 * once per pixel instead of once per tap.  ws: 16-byte aligned, btx_wgrad_workspace_bytes(kind, g, act_dtype, flags) bytes
 * (BTX_E_WORKSPACE if smaller); the outputs need not be cleared and are fully overwritten.  A launch whose pixels fit one
 * chunk stores straight into dw_* (no second launch).
 * rho_w / drho (both or neither): the reduction launch also writes what btx_rho_grad would compute from the finished
 * gradient, drho[i] = dw[i] * eps(i) * sigmoid(rho_w[i]) with dw = dw_delta (Flipout) or dw_mu (Reparameterization), eps of
 * stream BTX_STREAM_EPS_W of rng; rho_w in the order of mu_w.  drho may alias dw_delta (which then holds drho only); for a
 * Reparameterization layer it must be a buffer of its own (dw_mu is dmu). */
size_t btx_wgrad_workspace_bytes(int kind, const BtxGeom* g, int act_dtype, uint32_t flags);
int btx_contract_wgrad_ws(int kind, const BtxGeom* g, const void* x, const void* dy, float* dw_mu, float* dw_delta,
                          float* db_mu, float* db_delta, const BtxRng* rng, const BtxNoise* noise /* nullable */,
                          int act_dtype, uint32_t flags, void* ws, size_t ws_bytes, const float* rho_w /* nullable */,
                          float* drho /* nullable */, void* stream);

/* Sampling pre-pass, hoisted.  The LDS-DMA / patch kernels of btx_contract_fwd* first sample the layer's weights ONCE
 * into MFMA-ready tiles (W = mu + sigma*eps for Reparameterization; mu and sigma*eps for Flipout; reference:
 * conv_flipout.py:380-394, conv_variational.py:357-366 materialise the same tensors with ATen ops) and then contract.
 * btx_sample_weights does that pre-pass for a whole model in one launch (per-layer launches cost more than the
 * sampling itself); the buffers are handed to btx_contract_fwd* through BtxNoise.sampled_w.  `out` of each item must
 * hold btx_sampled_w_bytes(geom, kind, prec) bytes (depends on N, K, groups only), 16-byte aligned; the tile layout is
 * private to the library.  items_host is a HOST array, read before the call returns. */
typedef struct BtxSampleItem {
  const BtxGeom* geom;       /* host pointer */
  const float*   mu_w;       /* device, GEMM-major, as passed to btx_contract_fwd */
  const float*   rho_w;
  void*          out;        /* device */
  int32_t        kind;
  uint32_t       layer_id;
  int32_t        src_KW, src_C;  /* both 0: mu_w/rho_w have geom's layout.  Otherwise geom describes a PADDED layout
                                    [N][KD*KH][KW][C] (row-fused stems: KW and C padded; channel-padded layers: C padded)
                                    and mu_w/rho_w are the caller's unpadded [N][KD*KH][src_KW][src_C] weights: padded
                                    positions are sampled as exact zeros, noise indices are those of the padded layout
                                    (what the contraction launched on the padded geometry expects).  groups == 1. */
} BtxSampleItem;
size_t btx_sampled_w_bytes(const BtxGeom* g, int kind, int prec);
int btx_sample_weights(const BtxSampleItem* items_host, int n_items, const BtxRng* rng /* layer_id unused */,
                       int prec, void* stream);
/* The same for `lanes` MC samples at once (sample indices rng->sample_idx + l, or rng->sample_idx_dev[l]); `out` of each
 * item holds btx_sampled_w_bytes_lanes(...) bytes.  The mean tiles of a Flipout layer do not depend on the sample: the
 * buffer keeps ONE set for all lanes, and with BTX_SAMPLE_SKIP_MU in `sflags` the call leaves them untouched — for
 * callers that know mu AND rho have not changed since the call that last wrote them into this buffer (an MC loop over
 * frozen parameters): the buffer also keeps sigma = softplus(rho) (f32, tile order) from that call, and per MC step the
 * pre-pass reads it once and writes sigma*eps for every lane, nothing else. */
#define BTX_SAMPLE_SKIP_MU 1u
size_t btx_sampled_w_bytes_lanes(const BtxGeom* g, int kind, int prec, int lanes);
int btx_sample_weights_lanes(const BtxSampleItem* items_host, int n_items, const BtxRng* rng /* layer_id unused */,
                             int prec, void* stream, int lanes, uint32_t sflags);

/* Training, the step in front of the data gradient (ABI 7).  dx of a stride-1 convolution is the forward's own contraction on the
 * spatially flipped, channel-transposed kernel, of a Linear layer on W^T (what autograd derives for F.conv*d / F.linear inside
 * conv_flipout.py:376-417, linear_flipout.py:168-174).  One launch writes its three weight operands in the GEMM-major order of
 * that geometry — out[c][tp][n] = src[n][flip ? T-1-tp : tp][c] for mu, rho and for the eps the forward drew (regenerated at the
 * source index: stream BTX_STREAM_EPS_W of rng) — from the layer's own GEMM-major parameters mu_w / rho_w [N][T][C] (groups == 1).
 * The results go to btx_contract_fwd as (mu_w, rho_w, BtxNoise.eps_w) of the transposed geometry. */
int btx_dgrad_weights(const float* mu_w, const float* rho_w, float* out_mu, float* out_rho, float* out_eps, int N, int T, int C,
                      int flip, const BtxRng* rng, void* stream);

/* Training, the step behind btx_contract_wgrad: drho[i] = dw[i] * eps(i) * sigmoid(rho[i]) over the n elements of a weight
 * tensor in the order of mu_w (what autograd derives for `sigma = log1p(exp(rho)); delta = sigma * eps` of
 * conv_flipout.py:372-375 / conv_variational.py:358-366 / linear_flipout.py:150-153).  dw = dw_delta of a Flipout layer,
 * dw_mu of a Reparameterization layer (dmu is dw_mu itself).  eps is regenerated from rng (stream BTX_STREAM_EPS_W, or
 * _EPS_B for the bias vectors): the values btx_fill_eps would write, never materialised.  drho may alias dw. */
int btx_rho_grad(const float* dw, const float* rho, float* drho, size_t n, const BtxRng* rng, uint32_t rng_stream,
                 void* stream);

/* Training of the local reparameterization layers (BTX-LRT v1, DESIGN.md section 21 "Backward"; additive, the ABI number stays 9).
 *
 * btx_lrt_fwd_train: the BTX_KIND_LRT launch of btx_contract_fwd_ex without an epilogue — `out` is bit-identical to what that call
 * writes for the same arguments — plus root[i] = sqrtf(v_i + sigma_b^2), f32, in the layout of `out` (4 bytes of saved state per output
 * element).  flags: BTX_FLAG_GATHER, _REVERSE, _CONCURRENT; anything else BTX_E_UNSUPPORTED (as is BTX_PREC_BF16X3).
 *
 * btx_lrt_bwd: the whole backward of one layer on `stream`, from g = dy (the gradient of `out`, activation dtype, layout of `out`),
 * the saved root and the forward's BtxRng (zeta is regenerated: stream BTX_STREAM_OUT_NOISE at the element's index in `out`;
 * sample_idx_dev is honoured):
 *   c = root > 0 ? zeta / (2 root) : 0,  gv = act(g * c)            (gradient DEFINED as 0 where the variance sum is 0)
 *   dmu_w = corr(x, g)        drho_w = corr(act(x * x), gv) * 2 sigma sigmoid(rho_w)       GEMM-major f32, as btx_contract_wgrad_ws
 *   dmu_b = sum_p g           drho_b = (sum_p gv) * 2 sigma_b sigmoid(rho_b)               f32 [N], fixed summation order
 *   dx    = act(A + 2 x (.) B),  A = act(op^T(g, mu_w)),  B = act(op^T(gv, sigma^2))       activation dtype, layout of x; the two
 *           contractions run noise-free in precision `prec` on the geometry of the data gradient
 * Every member of BtxLrtGrads is nullable and skipped when NULL (drho_b needs rho_b).  Covered: Linear, and 2-D convolutions (D == KD
 * == 1) with groups == 1 whose stride-1 padding does not exceed the dilated kernel extent; everything else, and BTX_PREC_BF16X3,
 * returns BTX_E_UNSUPPORTED from both calls before anything is launched, as every argument error does (BTX_E_NULL, _SHAPE, _DTYPE,
 * _WORKSPACE).  No host read, no allocation, no memset: all scratch comes from `ws` (btx_lrt_bwd_workspace_bytes; any alignment).
 * Pointers off the 16-byte grid take element-wise paths; BTX_E_ALIGN is never returned. */
typedef struct BtxLrtGrads {
  float* dmu_w;
  float* drho_w;
  float* dmu_b;
  float* drho_b;
  void*  dx;
} BtxLrtGrads;
int btx_lrt_fwd_train(const BtxGeom* g, const void* x, const float* mu_w, const float* rho_w, const float* mu_b /* nullable */,
                      const float* rho_b /* nullable */, void* out, float* root, const BtxRng* rng, int act_dtype, int prec,
                      uint32_t flags, void* stream);
int btx_lrt_bwd_workspace_bytes(const BtxGeom* g, int act_dtype, int prec, size_t* bytes);
int btx_lrt_bwd(const BtxGeom* g, const void* x, const void* dy, const float* root, const float* mu_w, const float* rho_w,
                const float* rho_b /* nullable */, const BtxLrtGrads* out, const BtxRng* rng, int act_dtype, int prec, void* ws,
                size_t ws_bytes, void* stream);

/* §8(f): the data format in front of the path.  Small-C stems (BTX_FLAG_ROWFUSE) take channels-last [NB][Hp][Wp][cp]
 * activations with the conv padding materialised and the channels zero-padded to cp (4 or 8), in the MFMA dtype.
 * btx_rowfuse_pack writes that tensor in ONE pass from the caller's logical [N,C,H,W] activations of any layout:
 * strides_ncHW = element strides of (n, c, h, w), host array of 4; element (n,c,h,w) lands at
 * out[n][h+ph][w+pw][c]; everything else is zero.  x is read element by element; out: 16-byte aligned (BTX_E_ALIGN), one
 * store per padded pixel.  (The reference hands F.conv2d the NCHW tensor and a padding argument:
 * layers/flipout_layers/conv_flipout.py:376-383.) */
int btx_rowfuse_pack(const void* x, int in_dtype, const int64_t* strides_ncHW_host, int NB, int C, int H, int W,
                     void* out, int out_dtype, int Hp, int Wp, int cp, int ph, int pw, void* stream);

/* §8(f): the op right behind the stem of the reference's ResNets (models/deterministic/resnet_large.py: maxpool after
 * conv1-bn1-relu, torch.nn.MaxPool2d(kernel, stride, padding), dilation 1, floor mode).  Channels-last [NB][H][W][C]
 * -> [NB][Ho][Wo][C], C % 8 == 0, 2*pad <= k; identical results to torch (max is exact). */
int btx_maxpool2d_cl(const void* x, void* out, int dtype, int NB, int H, int W, int C, int k, int stride, int pad,
                     void* stream);
/* The same under autograd (ABI 8; the reference's training loop runs self.maxpool with gradients enabled).  _train: also idx[NB][Ho][Wo][C]
 * (uint8, 8-byte aligned) = kh * k + kw of each output element's maximum inside its window, the first maximum in scan order as
 * torch.nn.functional.max_pool2d_with_indices picks it (k <= 15).  _bwd: dx[NB][H][W][C] from dy[NB][Ho][Wo][C] and idx — every
 * input element sums dy over the windows whose recorded maximum it is (f32 accumulation, one rounding; no atomics, every element
 * of dx is written).  Results equal torch's max_pool2d forward / backward bit for bit. */
int btx_maxpool2d_cl_train(const void* x, void* out, uint8_t* idx, int dtype, int NB, int H, int W, int C, int k, int stride,
                           int pad, void* stream);
int btx_maxpool2d_cl_bwd(const void* dy, const uint8_t* idx, void* dx, int dtype, int NB, int H, int W, int C, int k, int stride,
                         int pad, void* stream);

/* §8(f)-4, the step either side of the path in the reference's TRAINING loop (README.md:114-125 on
 * models/deterministic/resnet_large.py:46-62: conv -> bn -> relu under model.train()): torch.nn.BatchNorm2d in training mode on
 * channels-last activations x[M][C] (M = N*H*W), ABI 7.  Forward: batch mean / biased variance per channel (f64 fold of per-block
 * f32 sums, fixed order), y = (x - mean) * invstd * gamma + beta, running_mean / running_var updated as torch does
 * (running = (1 - momentum) * running + momentum * batch, unbiased variance), save_mean / save_invstd (f32 [C]) for the backward.
 * Backward: dgamma = sum(dy * xhat), dbeta = sum(dy) ([C] in param_dtype since ABI 8, f32 before; each nullable), dx = gamma * invstd * (dy - dbeta / M - xhat * dgamma / M).
 * x / y / dy / dx: act_dtype (BTX_ACT_F32 | BTX_ACT_BF16), 16-byte aligned; gamma, beta, running_*: param_dtype (same codes),
 * each nullable (affine=False / track_running_stats=False); C % 8 == 0, C <= 2048 (else BTX_E_UNSUPPORTED: the caller keeps
 * torch's own kernels).  Three launches per call on `stream`, workspace btx_bn_workspace_bytes(M, C). */
size_t btx_bn_workspace_bytes(long long M, int C);
/* ABI 8: what the reference's blocks do right behind the normalisation (models/deterministic/resnet_large.py:46-62: `relu(bn1(..))`,
 * `relu(bn2(..) + identity)`), inside the same launches.  Forward: y = [relu](bn(x) [+ residual]) in ONE rounding; with relu the
 * apply pass also writes one bit per element (y > 0; byte t = the 8 channels of 16-byte group t, M*C/8 bytes) into `mask`.
 * Backward: the incoming gradient is first masked with those bits (torch's threshold_backward), g = dy where y > 0 else 0; all
 * sums and dx are formed from g, and `dres` (nullable) receives g itself — the gradient of the residual branch. */
typedef struct BtxBnFuse {
  const void* residual;  /* forward: act_dtype, shape and layout of x, 16-byte aligned; nullable */
  int32_t     relu;
  void*       mask;      /* forward: written; backward: read.  Required when relu. */
  void*       dres;      /* backward: act_dtype [M][C], 16-byte aligned; nullable; needs relu */
} BtxBnFuse;
int btx_bn_train_fwd(const void* x, void* y, int act_dtype, long long M, int C, const void* gamma, const void* beta,
                     void* running_mean, void* running_var, int param_dtype, float momentum, float eps, float* save_mean,
                     float* save_invstd, long long* num_batches_tracked /* nullable, int64 device word: += 1 (ABI 8) */,
                     const BtxBnFuse* fuse /* nullable */, void* ws, size_t ws_bytes, void* stream);
int btx_bn_train_bwd(const void* x, const void* dy, void* dx, int act_dtype, long long M, int C, const void* gamma,
                     int param_dtype, const float* save_mean, const float* save_invstd, void* dgamma, void* dbeta,
                     const BtxBnFuse* fuse /* nullable */, void* ws, size_t ws_bytes, void* stream);

/* Global average pooling in front of the classifier (resnet_large.py: AdaptiveAvgPool2d((1,1))): channels-last
 * [NB][HW][C] -> [NB][C], f32 accumulation in a fixed order, C % 8 == 0. */
int btx_avgpool_global_cl(const void* x, void* out, int dtype, int NB, int HW, int C, void* stream);

/* Output spatial extent for a geometry (same arithmetic as torch's conv / conv_transpose). */
int btx_out_shape(const BtxGeom* g, uint32_t flags, int32_t* Do, int32_t* Ho, int32_t* Wo);

/* Materialise the noise BTX-RNG v1 defines (tests, and the reference's observable side effect that
 * layer.eps_kernel holds the eps of the last forward: conv_variational.py:362, linear_variational.py:161).
 * btx_fill_eps: out[i] = eps(stream, index i), i in [0,n)   (stream = BTX_STREAM_EPS_W / _EPS_B)
 * btx_fill_sign: out[i] = +1/-1 (int8) for element index i  (stream = BTX_STREAM_SIGN_IN / _SIGN_OUT) */
int btx_fill_eps(float* out, size_t n, const BtxRng* rng, uint32_t rng_stream, void* stream);
int btx_fill_sign(int8_t* out, size_t n, const BtxRng* rng, uint32_t rng_stream, void* stream);

/* K6. Monte-Carlo predictive accumulation (what examples/main_bayesian_imagenet_dnn2bnn.py:483-499 and
 * utils/util.py:41-60 do on the host with torch.stack -> softmax -> mean / entropy).
 * packed layout (f32): [bs*C sum p | bs*C sum p^2 | bs sum H(p) | 1 sum kl | 1 sample count]
 * The buffer is accumulated in place (zero it first); one RCCL all-reduce(sum) of it merges ranks.
 * Limit: a row of probabilities stays in LDS, C <= 24575 classes (16383 on a device that refuses the 96-KiB dynamic-LDS
 * opt-in); wider rows return BTX_E_UNSUPPORTED (the Python face then uses torch ops on the device: mc.MC_MAX_CLASSES). */
size_t btx_mc_packed_floats(int bs, int C);
int btx_mc_accumulate(const void* logits, int bs, int C, int act_dtype, float kl,
                      float* packed, void* stream);
/* the same for the logits of `lanes` MC samples back to back ([lanes][bs][C], what a btx_contract_fwd_lanes forward leaves):
 * ONE launch; a workgroup owns a batch row and folds its lanes in order, so the result is bit for bit that of `lanes`
 * btx_mc_accumulate calls. */
int btx_mc_accumulate_lanes(const void* logits, int lanes, int bs, int C, int act_dtype, float kl,
                            float* packed, void* stream);

/* Fused Bayesian LSTM inference (reference layers/variational_layers/rnn_variational.py:104-153, layers/flipout_layers/
 * rnn_flipout.py:104-153): the whole sequence of an LSTMReparameterization / LSTMFlipout as 1 + T launches on `stream` —
 * the input projection of every (lane, step) pair at once into the workspace, then one recurrent step launch per time step
 * that samples its rows of W_hh in registers, contracts h_{t-1}, applies the gates and the cell and writes h_t / c_t into
 * hidden_seq[:, t] / c_seq[:, t].  Step t of a layer draws the noise of a Linear forward of that layer with sample index
 * s + t (s = sample_idx + lane, or the lane's word sample_idx_dev[lane]; the device word is read by the kernels, so a captured
 * sequence replays any sample).  Layer parameters: mu_w / rho_w [4H][K] f32 (K = I for ih, H for hh), mu_b / rho_b [4H] or
 * both NULL.
 *   x          [rows][T][I] in act_dtype; rows = B (x_shared: every lane reads it) or lanes*B (lane l's rows at l*B)
 *   h0, c0     [lanes*B][H] in act_dtype, or both NULL (zeros)
 *   hidden_seq, c_seq [lanes*B][T][H] in act_dtype (c is carried in f32 between the steps)
 *   kl_ih, kl_hh, kl_out: optional f32 scalars; kl_out = the per-step KL terms summed over T steps in the eager order
 *   prec       BTX_PREC_F32 or BTX_PREC_BF16 (BTX_PREC_BF16X3: BTX_E_UNSUPPORTED)
 * lanes in [1, 255].  Argument errors return before anything is launched. */
typedef struct BtxLstmLayer {
  const float* mu_w;
  const float* rho_w;
  const float* mu_b;
  const float* rho_b;
  uint32_t layer_id;
  uint32_t sample_idx;           /* index of step 0 of lane 0 (host form) */
  const void* sample_idx_dev;    /* uint32 per lane, or NULL */
} BtxLstmLayer;

size_t btx_lstm_workspace_bytes(int lanes, int B, int H, int T);
int btx_lstm_fwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, int x_shared,
                 const void* h0, const void* c0, void* hidden_seq, void* c_seq, const float* kl_ih, const float* kl_hh,
                 float* kl_out, int lanes, int B, int I, int H, int T, int act_dtype, int prec, void* workspace,
                 size_t ws_bytes, void* stream);

/* Fused Bayesian LSTM training (one lane, lanes are an inference feature): the forward of btx_lstm_fwd that also keeps, in the
 * caller's `saved` buffer, what the backward needs, and the backward through time.
 *   saved      [T][B][4H] f32 gate pre-activations, then (256-byte aligned) [T][B][H] f32 cell states c_t;
 *              btx_lstm_train_saved_bytes(B, H, T) bytes.  hidden_seq / c_seq / kl_out are bit for bit those of btx_lstm_fwd.
 *   workspace  btx_lstm_train_workspace_bytes(B, H, T) bytes for the forward, and again for the backward (dgates [T][B][4H] f32
 *              + the f32 dc carry [B][H]); the two need not be the same buffer.
 * btx_lstm_bwd is the backward of one btx_lstm_fwd_train call with the SAME arguments (layers, seed, sample indices, x, h0 / c0,
 * hidden_seq, saved).  Noise contract: that of btx_lstm_fwd — step t of a layer uses sample index s + t (s = sample_idx, or the
 * word sample_idx_dev[0], read on the device), eps_w element n*Kr + k (Kr = K rounded up to 8 when K % 8 != 0), eps_b element
 * n, s_in element b*Kr + k, s_out element b*4H + n; the backward regenerates every one of them in its kernels.  Launches:
 * T step launches (t = T-1 .. 0: dgates_t = gate / cell backward of d hidden_seq[:, t] (+ d c_seq[:, t]) + dgates_{t+1} . W_hh(s+t+1),
 * W_hh columns sampled in registers), one launch for dh0 / dc0 when either is wanted, one input-gradient launch for all steps
 * (dx_t = dgates_t . W_ih(s+t)), and one weight-gradient launch per layer whose grads are given.  Every sum runs in a fixed order
 * (no atomics): two calls give the same bits.
 *   d_hidden_seq, d_c_seq  [B][T][H] in act_dtype, either nullable (zeros)
 *   dx [B][T][I], dh0 / dc0 [B][H] in act_dtype, each nullable (not computed); dh0 / dc0 of a call without h0 / c0: the
 *              gradients at the zero initial state
 *   BtxLstmGrads (per layer, nullable): dmu_w / drho_w [4H][K] f32, dmu_b / drho_b [4H] f32 (NULL when the layer has no bias)
 *              drho = (sum_t dW_t * eps_t) * sigmoid(rho) (Flipout: dDelta_t = (dg_t o s_out)^T (in_t o s_in) in that sum)
 * bf16 precision: the operands the forward rounds (x, h, the sampled W / mu / Delta) are rounded to bf16, f32 accumulation.
 * prec BTX_PREC_BF16X3: BTX_E_UNSUPPORTED.  Argument errors return before anything is launched. */
typedef struct BtxLstmGrads {
  float* dmu_w;
  float* drho_w;
  float* dmu_b;
  float* drho_b;
} BtxLstmGrads;

size_t btx_lstm_train_saved_bytes(int B, int H, int T);
size_t btx_lstm_train_workspace_bytes(int B, int H, int T);
int btx_lstm_fwd_train(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x,
                       const void* h0, const void* c0, void* hidden_seq, void* c_seq, const float* kl_ih, const float* kl_hh,
                       float* kl_out, int B, int I, int H, int T, int act_dtype, int prec, void* workspace, size_t ws_bytes,
                       void* saved, size_t saved_bytes, void* stream);
int btx_lstm_bwd(int kind, const BtxLstmLayer* ih, const BtxLstmLayer* hh, uint64_t seed, const void* x, const void* h0,
                 const void* c0, const void* hidden_seq, const void* saved, const void* d_hidden_seq, const void* d_c_seq,
                 void* dx, void* dh0, void* dc0, const BtxLstmGrads* g_ih, const BtxLstmGrads* g_hh, int B, int I, int H, int T,
                 int act_dtype, int prec, void* workspace, size_t ws_bytes, void* stream);

/* K9. Uncertainty-calibration losses (reference utils/avuc_loss.py AvULoss / AUAvULoss, utils/uncertainty_calibration_loss.py
 * EaULoss / EaCLoss / AvULoss), forward and backward, without a host read: capturable into a hipGraph.
 *   loss = -beta * log(r + 1e-10),  r = (n_1 + n_4) / (n_1 + n_2 + n_3 + n_4 + 1e-10);  n_q = sum over the examples of a
 *   quadrant (good / bad x certain / uncertain) of a product of two soft weights.  Gradients flow through the weights only.
 * btx_avu_fwd: logits [B][C] in act_dtype, labels int64 [B].  area = 0: one threshold on the entropy H (certain = H <= th);
 *   area = 1: the trapezoid over np.linspace(0, 1, 21) of r at th_k = umin + t_k * (umax - umin), evaluated in double from the
 *   f32 umin / umax, th_20 = umax exactly (`th` is ignored).  out[0] = loss, out[1] = r (the AvU, or its area).
 * btx_avu_bwd: the backward of the btx_avu_fwd call that filled `ws`, same logits.  g_loss / g_r: DEVICE scalars, the upstream
 *   gradients of out[0] / out[1], either nullable (zero).  dlogits [B][C] in act_dtype, fully overwritten.
 * btx_eau_fwd / btx_eau_bwd: error, other f32 [B].  conf_form = 0 (EaU): other = uncertainty, certain = other <= other_th,
 *   weights (1 - tanh e | tanh e) x (1 - tanh u | tanh u);  conf_form = 1 (EaC): other = confidence, certain = other > other_th,
 *   weights (1 - tanh e | tanh e) x (conf | 1 - conf).  good = error <= error_th.  derror / dother: either nullable.
 * A threshold is the float argument, or — when its *_dev pointer is non-NULL — one f32 word in device memory that the kernel
 * reads when it runs (a captured graph follows an updated threshold).
 * ws: btx_calib_workspace_bytes(B) bytes, 8-byte aligned, written by the forward and read by the backward.  Every sum has a fixed shape and
 * no atomics: two runs give the same bits.  Three launches for forward + backward (AvU forms), two for EaU / EaC.
 * Errors: BTX_E_NULL, BTX_E_SHAPE (B, C <= 0, area / conf_form not 0 or 1), BTX_E_DTYPE, BTX_E_WORKSPACE, BTX_E_ALIGN (ws). */
size_t btx_calib_workspace_bytes(int B);
int btx_avu_fwd(const void* logits, const int64_t* labels, int B, int C, int act_dtype, int area, float th, const float* th_dev,
                float beta, float* out, void* ws, size_t ws_bytes, void* stream);
int btx_avu_bwd(const void* logits, int B, int C, int act_dtype, const float* g_loss, const float* g_r, const void* ws,
                size_t ws_bytes, void* dlogits, void* stream);
int btx_eau_fwd(const float* error, const float* other, int B, int conf_form, float error_th, const float* error_th_dev,
                float other_th, const float* other_th_dev, float beta, float* out, void* ws, size_t ws_bytes, void* stream);
int btx_eau_bwd(const float* error, const float* other, int B, int conf_form, const float* g_loss, const void* ws,
                size_t ws_bytes, float* derror, float* dother, void* stream);

/* K10. INT8 inference, arithmetic BTX-Q8 v1, for Linear and Conv2d Reparameterization layers with groups = 1
 * (reference layers/variational_layers/quantize_linear_variational.py:134-224, quantize_conv_variational.py:457-552: quantize eps,
 * quantized.mul, quantized.add, quantized linear / conv2d on the CPU engines).  Every floating step is one f32 operation, round to
 * nearest even, never contracted;  q(v, s, z, lo, hi) = clamp(rint(v * (1 / s)) + z, lo, hi).
 * BtxQ8Chain (HOST struct): the scales of the weight chain, each with the f32 reciprocal the quantize steps multiply by, and
 *   bias_div = (double)s_x * (double)s_w, the divisor of the int32 bias.
 * Weight image W: int8 [N][Kp], k = tap * Cp + c, tap = kh * KW + kw, Cp = C rounded up to 16, Kp = the row size
 *   btx_q8_weight_row_bytes(taps, C) = taps * Cp rounded up to 64; padding bytes are zero.  0 = invalid or too large.
 * btx_q8_quantize_act: x [NB][C][H][W] LOGICAL, element strides strides_host[4] (any memory format), f32 or bf16 ->
 *   out uint8 channels-last [NB][H][W][C] = q(x, scale, zero_point, 0, 255).  One launch.
 * btx_q8_sample_weights: one launch per layer.  mu_i / sigma_i: int8 GEMM-major [N][taps][C].  eps = BTX-RNG v1 stream EPS_W at
 *   index (n * taps + tap) * eps_C + c — the float layer's index space, eps_C = its channel count rounded up to 8 — or, when eps_w
 *   is non-NULL, eps_w[N][taps][C] f32 (then eps_C may equal C).  eps_i = q(eps, s_eps, 0, -128, 127);
 *   d_i = q((sigma_i * s_sigma) * (eps_i * s_eps), s_d, ..);  W_i = q((d_i * s_d) + (mu_i * s_mu), s_w, ..).
 *   S[n] = sum_k W_i[n][k] (int32).  b_i[n] = (int32) rint((double)(mu_b + sigma_b * eps_b) / bias_div), eps_b = stream EPS_B at
 *   index n or eps_b[n]; sigma_b NULL: the bias is mu_b; mu_b NULL: b_i = 0.  rng may be NULL when all the noise is explicit;
 *   rng->sample_idx_dev is honoured.
 * btx_q8_contract: implicit GEMM on v_mfma_i32_16x16x64_i8.  g: Linear (D = H = W = 1, taps = 1) or Conv2d (D = KD = 1), groups 1.
 *   acc = sum_k (x - x_zero_point) * W_i, padded taps contribute 0;  o = clamp(rint(f32(acc + b_i) * multiplier) + out_zero_point,
 *   relu ? out_zero_point : 0, 255).  out: uint8 channels-last [NB][OH][OW][N], or with out_f32 the dequantized
 *   f32 (o - out_zero_point) * out_scale.
 * Errors: BTX_E_NULL, BTX_E_SHAPE (extents, scales <= 0, zero points outside [0, 255]), BTX_E_UNSUPPORTED (groups != 1, D or KD != 1,
 *   index spaces beyond 32 bits), BTX_E_DTYPE, BTX_E_ALIGN (W 16 bytes; S, b_i, the quantize output 4 bytes).
 *
 * Between the layers (ABI 9, additive; the ops of the reference's models/bayesian/quantized_resnet_variational_large.py on quint8:
 * torch.ops.quantized.add, nn.MaxPool2d, nn.AvgPool2d).  All are one launch, capturable: no allocation, no sync, no host read.
 * BtxQ8Add (HOST struct): the add of a (uint8, s_a, z_a) and b (uint8, s_b, z_b) into (s, zero_point):
 *   da = fma(s_a, a, pre_a), pre_a = f32(s_a * f32(-z_a)), ONE rounding (what torch's vector kernel computes, not (a - z_a) * s_a);
 *   db alike;  o = clamp(rint((da + db) * inv_s) + zero_point, relu ? zero_point : 0, 255), inv_s = f32(1) / f32(s).  The caller
 *   computes pre_a, pre_b, inv_s once in f32.
 * btx_q8_add: out[i] = add(a[i], b[i]) over n bytes; 16 bytes per thread when the three bases are 16-byte aligned, bytewise else.
 * btx_q8_contract_res: btx_q8_contract with a residual operand in its store: the lane's four uint8 outputs o (formed exactly as
 *   btx_q8_contract forms them, the conv's own ReLU clamp included) become add(o, residual[m][n]) with add_host->s_a / pre_a
 *   describing the conv's (out scale, out_zero_point).  residual: uint8 channels-last [NB][OH][OW][N].  Bit-identical to
 *   btx_q8_contract followed by btx_q8_add.  out_f32 != 0 -> BTX_E_UNSUPPORTED.
 * btx_q8_maxpool2d_cl / btx_q8_avgpool2d_cl: uint8 channels-last [NB][H][W][C] -> [NB][Ho][Wo][C], floor mode, Ho = (H + 2 pad - k)
 *   / stride + 1; scale and zero point pass through.  16 channels per thread when C % 16 == 0 and both bases are 16-byte aligned,
 *   bytewise otherwise.  max: the maximum over the in-image window elements, 2 * pad <= k.  avg: o = clamp(rint(f32(sum - k*k *
 *   zero_point) * f32(1.0 / (k*k))) + zero_point, 0, 255), int32 sum, the reciprocal computed in double and rounded once;
 *   pad != 0 or ceil_mode != 0 -> BTX_E_UNSUPPORTED.
 * Errors as above: BTX_E_NULL, BTX_E_SHAPE (extents, n == 0, s_a / s_b / inv_s <= 0, zero points outside [0, 255]). */
typedef struct BtxQ8Chain {
  float s_sigma, s_mu, s_eps, inv_s_eps, s_d, inv_s_d, inv_s_w;
  double bias_div;
} BtxQ8Chain;
size_t btx_q8_weight_row_bytes(int taps, int C);
int btx_q8_quantize_act(const void* x, int act_dtype, const int64_t* strides_host, uint8_t* out, int NB, int C, int H, int W,
                        float scale, int zero_point, void* stream);
int btx_q8_sample_weights(const int8_t* mu_i, const int8_t* sigma_i, const float* mu_b, const float* sigma_b, int N, int taps, int C,
                          int eps_C, const BtxQ8Chain* chain_host, const BtxRng* rng, const float* eps_w, const float* eps_b,
                          int8_t* W, int32_t* S, int32_t* b_i, void* stream);
int btx_q8_contract(const BtxGeom* g, const uint8_t* x, int x_zero_point, const int8_t* W, const int32_t* S, const int32_t* b_i,
                    float multiplier, int out_zero_point, int relu, int out_f32, float out_scale, void* out, void* stream);
typedef struct BtxQ8Add {
  float s_a, pre_a, s_b, pre_b, inv_s;
  int zero_point, relu;
} BtxQ8Add;
int btx_q8_add(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, const BtxQ8Add* add_host, void* stream);
int btx_q8_contract_res(const BtxGeom* g, const uint8_t* x, int x_zero_point, const int8_t* W, const int32_t* S, const int32_t* b_i,
                        float multiplier, int out_zero_point, int relu, int out_f32, const uint8_t* residual, const BtxQ8Add* add_host,
                        void* out, void* stream);
int btx_q8_maxpool2d_cl(const uint8_t* x, uint8_t* out, int NB, int H, int W, int C, int k, int stride, int pad, void* stream);
int btx_q8_avgpool2d_cl(const uint8_t* x, uint8_t* out, int NB, int H, int W, int C, int k, int stride, int pad, int ceil_mode,
                        int zero_point, void* stream);

/* K10, Flipout (ABI 9, additive; DESIGN.md §13 "Flipout"): the INT8 forward of LinearFlipout / Conv2dFlipout, groups = 1 (reference
 * layers/flipout_layers/quantized_linear_flipout.py:138-261, quantized_conv_flipout.py:398-514: two quantized convs, three
 * quantized.mul and one quantized.add, entries e0 .. e9 of quant_dict).  One pre-pass launch and ONE contraction launch.
 * quantized.mul(a, b -> (s_o, z_o)) = clamp(rint(f32((a - z_a) * (b - z_b)) * m) + z_o, lo, hi) with the int32 product exact and
 *   m = f32(f32(s_a) * f32(s_b)) * (f32(1) / f32(s_o)), computed by the caller once.
 * BtxQ8Delta (HOST struct): inv_s_eps = 1 / s_e0; mult = m of (s_sigma, s_e0 -> s_e1); mean_bias / pert_bias = BTX_Q8_BIAS_*: which
 *   f32 vector becomes the int32 bias of the mean / the perturbed GEMM (none, mu_b, sigma_b * eps_b); div_mean = (double)s_x *
 *   s_mu, div_pert = (double)s_e6 * s_e1.
 * btx_q8_sample_delta: sigma_i int8 GEMM-major [N][taps][C]; eps as in btx_q8_sample_weights (stream EPS_W in the float layer's
 *   index space, eps_C, or explicit eps_w).  eps_i = q(eps, s_e0, 0, -128, 127); D[n][k] = mul(sigma_i, eps_i) in [-128, 127], int8
 *   [N][Kp] in the weight image layout, padding zero; S_d[n] = its row sum; b_mean_i / b_pert_i[n] = (int32) rint((double)b /
 *   div), b = mu_b[n] or f32(sigma_b[n] * eps_b) (eps_b: stream EPS_B at index n, or eps_b[n]) or 0.
 * BtxQ8Flipout (HOST struct): z_x, z_xp (e6), z_mean (e3), z_pert (e7), z_p2 (e8); sin_pos / sin_neg = the bytes q(+1, e4), q(-1, e4)
 *   minus z_e4, sout_* alike with e5; mult_xp = m of (s_x, s_e4 -> s_e6), mult_mean = f32(f32(s_x) * f32(s_mu)) / f32(s_e3),
 *   mult_pert = f32(f32(s_e6) * f32(s_e1)) / f32(s_e7), mult_p2 = m of (s_e7, s_e5 -> s_e8); out_scale = s_e9 (f32 output).
 * btx_q8_contract_flipout: g as in btx_q8_contract.  W_mu / S_mu: the mean image and its row sums (btx_q8_sample_weights with a zero
 *   sigma_i).  x' = mul(x, sign byte) is formed on the way into LDS; o1 = requantize(sum (x - z_x) W_mu + b_mean_i), p =
 *   requantize(sum (x' - z_xp) D + b_pert_i), padded taps contribute 0 to both; p2 = mul(p, sign byte); out = add(o1, p2) with
 *   add_host (a = (s_e3, z_mean), b = (s_e8, z_p2), its relu flag the ReLU clamp).  out: uint8 channels-last [NB][OH][OW][N], or
 *   with out_f32 the dequantized f32 (o - z_e9) * out_scale.  Signs: BTX-RNG v1 stream SIGN_IN at index pixel * sign_C + c (pixel
 *   = (img * H + ih) * W + iw; sign_C = the float layer's row length, >= C and a multiple of 8) and SIGN_OUT at m * N + n; sign_in / sign_out (int8
 *   +1 / -1, channels-last like x / out), when non-NULL, override the hash.  rng may be NULL when both are given;
 *   rng->sample_idx_dev is honoured.  Errors as above; capturable. */
#define BTX_Q8_BIAS_NONE      0
#define BTX_Q8_BIAS_MU        1
#define BTX_Q8_BIAS_SIGMA_EPS 2
typedef struct BtxQ8Delta {
  float inv_s_eps, mult;
  int mean_bias, pert_bias;
  double div_mean, div_pert;
} BtxQ8Delta;
typedef struct BtxQ8Flipout {
  int z_x, z_xp, z_mean, z_pert, z_p2;
  int sin_pos, sin_neg, sout_pos, sout_neg;
  float mult_xp, mult_mean, mult_pert, mult_p2, out_scale;
} BtxQ8Flipout;
int btx_q8_sample_delta(const int8_t* sigma_i, const float* mu_b, const float* sigma_b, int N, int taps, int C, int eps_C,
                        const BtxQ8Delta* delta_host, const BtxRng* rng, const float* eps_w, const float* eps_b, int8_t* D, int32_t* S_d,
                        int32_t* b_mean_i, int32_t* b_pert_i, void* stream);
int btx_q8_contract_flipout(const BtxGeom* g, const uint8_t* x, const int8_t* W_mu, const int32_t* S_mu, const int32_t* b_mean_i,
                            const int8_t* D, const int32_t* S_d, const int32_t* b_pert_i, const BtxQ8Flipout* flip_host,
                            const BtxQ8Add* add_host, const BtxRng* rng, int sign_C, const int8_t* sign_in, const int8_t* sign_out,
                            int out_f32, void* out, void* stream);

/* K11 (ABI 9, additive; DESIGN.md §14 "BTX-OPT v1"): the parameter update of SGD / Adam / AdamW as ONE pass over every tensor of a
 * param group (torch/optim/sgd.py, adam.py: _single_tensor_sgd / _single_tensor_adam), and the global gradient norm with its clip
 * coefficient.  f32 only.  The unit is built with -ffp-contract=off: every operation of BTX-OPT v1 is rounded once.
 * BtxOptimItem (HOST array): p, g and the state tensors of one parameter in the SAME storage order, n elements each, walked flat.
 *   SGD: state0 = momentum_buffer (NULL when momentum == 0), state1 unused.  Adam: state0 = exp_avg, state1 = exp_avg_sq.
 *   Items with n == 0 are skipped.  The library folds the items into by-value kernel-argument tables of at most 48 per launch; a
 *   workgroup owns one chunk of BTX_OPTIM_CHUNK elements of one item.  16-byte accesses when all pointers of an item are 16-byte
 *   aligned, scalar ones otherwise.
 * BtxOptimHyper (DEVICE block, 16 words, 16-byte aligned): read by the kernel when it RUNS, never written by it; the host rewrites
 *   it before each launch or replay, so a captured launch follows a changed lr and the advancing step count.  All floats are the
 *   f32 roundings of values the host computes in double:
 *   neg_lr = -lr (SGD); wd = weight_decay (coupled); decay_mul = 1 - lr * wd (BTX_OPT_DECOUPLED); one_m_b1 = 1 - beta1; b2 = beta2;
 *   one_m_b2 = 1 - beta2; eps; neg_step_size = -lr / (1 - beta1^t); bc2s = sqrt(1 - beta2^t); momentum; one_m_damp = 1 - dampening.
 * coef: optional DEVICE word (btx_optim_grad_norm's out[1]): g is multiplied by it first (after the negation of BTX_OPT_MAXIMIZE).
 * btx_optim_grad_norm: out[0] = total_norm = f32(sqrt(sum g^2)) over all items, out[1] = coef = min(1, max_norm / (total_norm +
 *   1e-6f)) in f32.  Per-chunk f32 lane sums, f64 partials in ws (btx_optim_grad_norm_workspace_bytes(n_items, total elements)), one
 *   final block folds them in a fixed order: no atomics, two runs give the same bits.  state pointers of the items are ignored.
 * Every launch is capturable (no allocation, no sync, no host read).  Errors, all before anything is launched: BTX_E_NULL (items,
 *   hyper, out, ws, p, g, a required state pointer), BTX_E_SHAPE (n_items < 0, n < 0, max_norm not > 0), BTX_E_UNSUPPORTED (more than
 *   BTX_OPTIM_MAX_ITEMS items), BTX_E_ALIGN (a tensor pointer not 4-byte, hyper not 16-byte, ws not 8-byte aligned),
 *   BTX_E_WORKSPACE.  n_items == 0 (or only empty items) launches nothing and returns 0 (grad_norm still writes out). */
#define BTX_OPTIM_CHUNK     4096
#define BTX_OPTIM_MAX_ITEMS 65536
#define BTX_OPT_MAXIMIZE   1u
#define BTX_OPT_NESTEROV   2u
#define BTX_OPT_DECOUPLED  4u   /* AdamW: p *= decay_mul */
#define BTX_OPT_FIRST_STEP 8u   /* SGD: buf = g */
#define BTX_OPT_COUPLED_WD 16u  /* g += wd * p */
typedef struct BtxOptimItem {
  float* p;
  const float* g;
  float* state0;
  float* state1;
  int64_t n;
} BtxOptimItem;
typedef struct BtxOptimHyper {
  float neg_lr, wd, decay_mul, one_m_b1, b2, one_m_b2, eps, neg_step_size, bc2s, momentum, one_m_damp;
  uint32_t flags;
  uint32_t reserved[4];
} BtxOptimHyper;
int btx_optim_sgd(const BtxOptimItem* items, int n_items, const BtxOptimHyper* hyper_dev, int has_momentum, const float* coef_dev,
                  void* stream);
int btx_optim_adam(const BtxOptimItem* items, int n_items, const BtxOptimHyper* hyper_dev, const float* coef_dev, void* stream);
size_t btx_optim_grad_norm_workspace_bytes(int n_items, int64_t total_elements);
int btx_optim_grad_norm(const BtxOptimItem* items, int n_items, float max_norm, float* out_dev, void* ws, size_t ws_bytes,
                        void* stream);

/* K12 (ABI 9, additive): loss heads on a stack of Monte-Carlo logits [S][B][C] (contiguous, act_dtype f32 or bf16),
 * labels int64 [B].  f32 arithmetic, max-subtracted softmax / log-sum-exp; one workgroup per batch row for all S samples; every sum
 * has a fixed shape and no atomics: two runs give the same bits.  No host read, no allocation: capturable into a hipGraph.
 * 1 <= S <= BTX_MCLOSS_MAX_S, B >= 1 (else BTX_E_SHAPE), 1 <= C <= BTX_MCLOSS_MAX_CLASSES (C < 1: BTX_E_SHAPE, wider:
 * BTX_E_UNSUPPORTED).  Rows off the 16-byte grid (any pointer, any C) take the element-wise path: same bits, never BTX_E_ALIGN.
 * ws: btx_mcloss_workspace_bytes(S, B) bytes (enough for either head), 8-byte aligned, written by a forward and read by ITS backward.
 * btx_mc_ce_fwd: out[0] = ce + (kl ? kl[0] * inv_b : 0);  reduce 0: ce = inv_b * sum_b CE(mean_s z_s[b], y_b), reduce 1:
 *   ce = inv_b * sum_b mean_s CE(z_s[b], y_b);  CE with label smoothing ls in [0, 1): lse(z) - (1 - ls) z[y] - ls / C * sum_c z[c].
 *   kl: DEVICE pointer to one f32, nullable.  inv_b: the caller's 1 / B.
 * btx_mc_ce_bwd: dlogits [S][B][C] in act_dtype = g_loss[0] * d ce / d logits, fully overwritten; g_loss: DEVICE scalar.  (The gradient
 *   of the kl input is g_loss[0] * inv_b: the caller's.)
 * btx_avu_mc_fwd / btx_avu_mc_bwd: btx_avu_fwd / btx_avu_bwd with p_s = softmax(z_s), pbar = mean_s p_s, confidence and prediction
 *   from pbar (lowest index on ties) and the uncertainty u = H(pbar) - mean_s H(p_s), epsilon 1e-10 inside every log, in place of the
 *   entropy; area, th, th_dev, beta, out[0..1], g_loss, g_r as there.  Gradients flow through the soft weights into all S samples.
 *   The backward keeps a row of C floats in LDS: C <= BTX_AVU_MC_MAX_CLASSES (wider: BTX_E_UNSUPPORTED, from forward and backward alike).
 * Errors: BTX_E_NULL, BTX_E_SHAPE (also reduce / area not 0 or 1, label_smoothing outside [0, 1)), BTX_E_UNSUPPORTED, BTX_E_DTYPE,
 *   BTX_E_WORKSPACE, BTX_E_ALIGN (ws only), all before anything is launched. */
#define BTX_MCLOSS_MAX_S 32
#define BTX_MCLOSS_MAX_CLASSES 24575
#define BTX_AVU_MC_MAX_CLASSES 16128   /* btx_avu_mc_*: the backward's LDS row of C floats stays below the 64 KiB every kernel may use */
size_t btx_mcloss_workspace_bytes(int S, int B);
int btx_mc_ce_fwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int reduce, float label_smoothing,
                  const float* kl, float inv_b, float* out, void* ws, size_t ws_bytes, void* stream);
int btx_mc_ce_bwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int reduce, float label_smoothing,
                  float inv_b, const float* g_loss, const void* ws, size_t ws_bytes, void* dlogits, void* stream);
int btx_avu_mc_fwd(const void* logits, const int64_t* labels, int S, int B, int C, int act_dtype, int area, float th,
                   const float* th_dev, float beta, float* out, void* ws, size_t ws_bytes, void* stream);
int btx_avu_mc_bwd(const void* logits, int S, int B, int C, int act_dtype, const float* g_loss, const float* g_r, const void* ws,
                   size_t ws_bytes, void* dlogits, void* stream);

/* K13 (ABI 9, additive): the bias gradient of a variational layer with a fixed summation order,
 *   db_mu[n] = sum_m dy[m][n],   Flipout also  db_delta[n] = sum_m dy[m][n] * s_out[m][n];   dy [M][N] pixel-major in act_dtype.
 * s_out: `sign_out` (int8 +/-1, dy's layout) when non-NULL, else the hashed BTX-RNG v1 sign of element m * N + n under `rng` — the
 * signs btx_contract_wgrad applies to dy (BTX_FLAG_SWAP_SIGNS in `flags` selects the SIGN_IN stream; rng->sample_idx_dev is honoured).
 * btx_contract_wgrad[_ws] can return the same sums (db_mu / db_delta non-NULL), accumulated with f32 atomics over its pixel chunks:
 * equal up to the order of the additions, not bit-reproducible.  Here a thread adds its pixels in order, rows and parts are added in
 * index order: two runs give the same bits.  ws: btx_bias_grad_workspace_bytes(M, N) bytes, 4-byte aligned (may be NULL when M <= 1024).
 * Errors: BTX_E_NULL, BTX_E_UNSUPPORTED (kind), BTX_E_SHAPE (M, N < 1), BTX_E_DTYPE, BTX_E_WORKSPACE, BTX_E_ALIGN (ws). */
size_t btx_bias_grad_workspace_bytes(int64_t M, int N);
int btx_bias_grad(int kind, const void* dy, int64_t M, int N, int act_dtype, float* db_mu, float* db_delta, const BtxRng* rng,
                  const int8_t* sign_out, uint32_t flags, void* ws, size_t ws_bytes, void* stream);

/* K14 (ABI 9, additive): the gradient bucket of data-parallel training.  Every gradient of a step (and the loss
 * word) is scaled into ONE flat f32 buffer, the operand of the step's single all-reduce, and copied back out of it.  f32 only.
 * BtxBucketItem (HOST array): n elements at src, walked flat, and their place in the bucket, bucket + offset (in elements).  The
 *   caller lays the bucket out (parallel.GradReducer rounds every offset up to a multiple of 4 so that 16-byte aligned tensors
 *   keep 16-byte accesses); the slices must not overlap.  Items with n == 0 are skipped.
 * btx_bucket_pack:   bucket[offset + i] = src[i] * scale, ONE f32 multiply rounded once (the unit is built with -ffp-contract=off).
 * btx_bucket_unpack: src[i] = bucket[offset + i], a plain copy.  It WRITES the memory src points to: the field is const because pack,
 *   the common direction, only reads it, and unpack casts the qualifier away.
 * The library folds the items into by-value kernel-argument tables of at most 48 per launch; a workgroup owns one chunk of
 *   BTX_OPTIM_CHUNK elements of one item.  16-byte accesses when src and bucket + offset are both 16-byte aligned, scalar ones
 *   otherwise: any 4-byte aligned tensor is valid.  Words of the bucket outside the items' slices are never written.
 * Every launch is capturable (no allocation, no sync, no host read).  Errors, all before anything is launched: BTX_E_NULL (bucket,
 *   items, the src of a non-empty item), BTX_E_SHAPE (n_items < 0, n < 0, offset < 0), BTX_E_UNSUPPORTED (more than
 *   BTX_OPTIM_MAX_ITEMS items, an item of more than (2^31 - 1) * BTX_OPTIM_CHUNK elements), BTX_E_ALIGN (src or bucket not 4-byte
 *   aligned).  n_items == 0 (or only empty items) launches nothing and returns 0. */
typedef struct BtxBucketItem {
  const float* src;
  int64_t offset;
  int64_t n;
} BtxBucketItem;
int btx_bucket_pack(const BtxBucketItem* items, int n_items, float scale, float* bucket, void* stream);
int btx_bucket_unpack(const BtxBucketItem* items, int n_items, const float* bucket, void* stream);

/* K15 (ABI 9, additive; DESIGN.md §18, BTX-EVAL v1): evaluation of a batch from its packed MC statistics (K6) and its labels, on
 * the device and without a host read — what examples/main_bayesian_imagenet.py:549-595 (validate: top-1 / top-5) and :598-642
 * (evaluate: mean probabilities, argmax, accuracy) do on the host, with the entropy / mutual information of utils/util.py:41-60
 * and the quadrant counts of utils/avuc_loss.py:392-443 (eval_avu / accuracy_vs_uncertainty, a Python loop per example).
 * Per row (f32, every operation rounded once, sums of a shape fixed by C): p = sum_p / n, pred = lowest index of the largest p,
 *   conf = p[pred]; a row is valid iff 0 <= label < C (every other label is ignored and adds nothing);
 *   rank = #{c : p_c > p_y} + #{c < y : p_c == p_y}; nll = -logf(p_y + 1e-15f); brier = sum_c (p_c - [c == y])^2;
 *   H = -sum_c p_c logf(p_c + 1e-15f); MI = H - sum_H / n.
 * The row's record [pred, rank, conf, p_y, nll, brier, H, MI] (rank = -1, p_y = nll = brier = 0 when ignored) goes to the workspace
 *   and, when records != NULL, to records[cursor + row] for cursor + row < capacity (cursor: the state word below).
 * state (float64, accumulated in place: zero it to reset; add two states to merge them):
 *   [0] valid rows  [1] ignored rows  [2] top-1 hits  [3] top-k hits (rank < topk)  [4] sum nll  [5] sum brier  [6] sum H
 *   [7] sum MI  [8] sum conf  [9] sum u over correct rows  [10] sum u over incorrect rows  (u = H, or MI when use_mi)
 *   [BTX_MC_EVAL_CURSOR] rows seen (advanced by bs per call)  [BTX_MC_EVAL_DROPPED] rows whose record did not fit  [13..15] spare
 *   [BTX_MC_EVAL_HEADER + 3 b ..] ECE bin b of nbins, b = clamp((int)ceilf(conf * nbins) - 1, 0, nbins - 1): rows, sum conf, top-1 hits
 *   [BTX_MC_EVAL_HEADER + 3 nbins + 4 t ..] threshold t of T: n_ac, n_au, n_ic, n_iu with certain <=> u <= th[t]
 *   th is DEVICE memory, read by the launch.  Sums are taken in double in an order fixed by bs alone: no atomics.
 * Nothing varies per batch but the tensors' contents, so a captured call can be replayed.  Any 4-byte aligned packed / th /
 *   records / ws and 8-byte aligned labels / state are valid (element-wise accesses).
 * Errors, all before anything is launched: BTX_E_NULL (packed, labels, state, ws; th with T > 0; records with capacity > 0),
 *   BTX_E_SHAPE (bs, C, topk < 1, nbins outside 1..BTX_MC_EVAL_MAX_BINS, T outside 0..BTX_MC_EVAL_MAX_THRESHOLDS, capacity < 0,
 *   use_mi not 0 or 1), BTX_E_UNSUPPORTED (C > BTX_MC_EVAL_MAX_CLASSES: the Python face uses torch ops on the device),
 *   BTX_E_WORKSPACE (ws_bytes, state_doubles below the two helpers), BTX_E_ALIGN (below the element type's alignment). */
#define BTX_MC_EVAL_MAX_CLASSES 24575   /* the K6 limit: what the accumulate kernels pack, this head evaluates */
#define BTX_MC_EVAL_MAX_BINS 64
#define BTX_MC_EVAL_MAX_THRESHOLDS 32
#define BTX_MC_EVAL_HEADER 16
#define BTX_MC_EVAL_CURSOR 11
#define BTX_MC_EVAL_DROPPED 12
size_t btx_mc_eval_state_doubles(int nbins, int T);   /* 0 for nbins / T out of range */
size_t btx_mc_eval_workspace_bytes(int bs);
int btx_mc_eval(const float* packed, const int64_t* labels, int bs, int C, int topk, int nbins, const float* th, int T, int use_mi,
                double* state, size_t state_doubles, float* records, int64_t capacity, void* ws, size_t ws_bytes, void* stream);

/* K16 (ABI 9, additive; DESIGN.md §19, BTX-REG v1): the two ends of a model that predicts real values.  A model output is
 * out [rows][W] in act_dtype (f32 or bf16): has_var = 1: W = 2 D, columns [0, D) the mean m and [D, 2 D) the log-variance s;
 * has_var = 0: W = D, the mean alone.  Elements e = b * D + d, N = rows * D <= 2^31 - 3 (more: BTX_E_UNSUPPORTED).
 * Every launch goes to the caller's stream, allocates nothing, reads nothing on the host and uses no atomics: capturable, and two
 * runs give the same bits.  Sums over the elements ("chunk / fold"): terms widen to double; a workgroup of 256 threads owns a chunk
 * of 4096 elements, thread t adds e = t, t + 256, ... in order from zero, a xor butterfly per wave (32, 16, ..., 1), then
 * (w0 + w1) + (w2 + w3); ONE workgroup folds the chunks' partials, lane l adding l, l + 64, ..., with the same butterfly.
 *
 * btx_mc_moments_lanes: packed (float64, 3 N + 2 words) += the statistics of `lanes` samples, out [lanes * bs][W] back to back:
 *   [N sum m | N sum m^2 | N sum v | sum kl | samples], v = (double)expf(s), m^2 the exact double product of the widened value; the
 *   third block is left untouched when has_var = 0.  One element-wise launch; a thread folds the lanes of its elements in order, so
 *   one call equals `lanes` calls with lanes = 1 bit for bit.  16-byte accesses when out and packed are 16-byte aligned and D is a
 *   multiple of 16 / sizeof(element), element-wise ones otherwise: same bits, and no valid tensor ends in BTX_E_ALIGN.
 * btx_mc_gnll_fwd: out[0] = the Gaussian negative log-likelihood of the stack [S][B][W] against target [B][D] (f32), 1 <= S <=
 *   BTX_MCLOSS_MAX_S.  Per element f32, every operation rounded once.  has_var = 0: s = logf(noise_var) for every sample, noise_var > 0.
 *   reduce 1 ("loss"):    l = 0.5 (s + (y - m)^2 expf(-s));  out = sum_{s,b,d} l / (S B) + [full] 0.5 log(2 pi) D + kl[0] / B
 *   reduce 0 ("moments"): mbar = (sum_s m_s) / S, vbar = (sum_s expf(s_s)) / S + (sum_s (m_s - mbar)^2) / S,
 *                         l = 0.5 (logf(vbar) + (y - mbar)^2 / vbar);  out = sum_{b,d} l / B + [full] ... + kl[0] / B
 *   The sum is the chunk / fold sum; the division, the constant and the kl term are taken in double and rounded to f32 once.
 *   kl: DEVICE pointer to one f32, nullable.  ws: btx_mc_gnll_workspace_bytes(B, D) bytes, 8-byte aligned.  Two launches.
 * btx_mc_gnll_bwd: dstack [S][B][W] in act_dtype (bf16: round to nearest even) = g_loss[0] * d out / d stack, fully overwritten, one
 *   element-wise launch; g_loss: DEVICE scalar, multiplied last.  With k = 1 / (S B), r = y - m (reduce 1) or y - mbar (reduce 0):
 *   reduce 1: d m_s = -(r expf(-s)) k, d s_s = 0.5 (1 - r^2 expf(-s)) k;  reduce 0: a = 1 / vbar - r^2 / vbar^2,
 *   d m_s = (-(r / vbar) + (m_s - mbar) a) k, d s_s = 0.5 expf(s_s) a k.  (The gradient of kl is g_loss[0] / B: the caller's.)
 * btx_reg_eval_update: folds a batch — packed as above and target [bs][D] f32 — into state (float64).  Per element, in double with
 *   every operation rounded once: n = packed[3 N + 1], mean = sum_m / n, ep = max(sum_m2 / n - mean^2, 0), al = sum_v / n + noise_var,
 *   var = max(ep + al, min_var), err = y - mean, nll = 0.5 ((double)logf((float)(2 pi var)) + err^2 / var),
 *   cover_k = [err^2 <= z2[k] var], k < K <= BTX_REG_EVAL_MAX_LEVELS; z2: DEVICE doubles (the squared normal quantiles).  A NaN target
 *   marks an ignored element, which adds nothing.  state, accumulated in place (zero it to reset, add two states to merge them):
 *   [0] valid  [1] ignored  [2] sum err^2  [3] sum |err|  [4] sum nll  [5] sum ep  [6] sum al  [7] sum y  [8] sum y^2
 *   [BTX_REG_EVAL_CURSOR] elements seen  [BTX_REG_EVAL_DROPPED] elements whose record did not fit  [11..15] spare
 *   [BTX_REG_EVAL_HEADER + k] elements covered at level k.  records != NULL: records[cursor + e] = (mean, ep, al, err) as f32 for
 *   cursor + e < capacity (err is NaN on an ignored element).  Two launches; ws: btx_reg_eval_workspace_bytes(bs, D) bytes.
 * Errors, all before anything is launched: BTX_E_NULL, BTX_E_SHAPE (lanes, S, rows, D < 1, S > BTX_MCLOSS_MAX_S, a flag that is not
 *   0 or 1, has_var = 0 with noise_var <= 0, K outside 0..BTX_REG_EVAL_MAX_LEVELS, capacity < 0, noise_var < 0, min_var <= 0),
 *   BTX_E_UNSUPPORTED (N), BTX_E_DTYPE, BTX_E_WORKSPACE (ws_bytes, state_doubles < BTX_REG_EVAL_HEADER + K), BTX_E_ALIGN (a pointer
 *   below the alignment of its own element type). */
#define BTX_REG_EVAL_MAX_LEVELS 8
#define BTX_REG_EVAL_HEADER 16
#define BTX_REG_EVAL_CURSOR 9
#define BTX_REG_EVAL_DROPPED 10
int btx_mc_moments_lanes(const void* out, int lanes, int bs, int D, int has_var, int act_dtype, double kl, double* packed,
                         void* stream);
size_t btx_mc_gnll_workspace_bytes(int B, int D);
int btx_mc_gnll_fwd(const void* stack, const float* target, int S, int B, int D, int has_var, int act_dtype, int reduce, float noise_var,
                    int full, const float* kl, float* out, void* ws, size_t ws_bytes, void* stream);
int btx_mc_gnll_bwd(const void* stack, const float* target, int S, int B, int D, int has_var, int act_dtype, int reduce, float noise_var,
                    const float* g_loss, void* dstack, void* stream);
size_t btx_reg_eval_workspace_bytes(int bs, int D);
int btx_reg_eval_update(const double* packed, const float* target, int bs, int D, double noise_var, double min_var, const double* z2,
                        int K, double* state, size_t state_doubles, float* records, int64_t capacity, void* ws, size_t ws_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTX_H_ */
