"""ctypes binding of libbtx.so (include/btx.h).  The HIP library is THE product path: there is no fallback —
`lib()` raises if it is missing, and every non-zero return code raises `BtxError`."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

KIND_REPARAM, KIND_FLIPOUT, KIND_LRT = 0, 1, 2
ACT_F32, ACT_BF16 = 0, 1
PREC_F32, PREC_BF16, PREC_BF16X3 = 0, 1, 2
PREC_CODE = {"f32": 0, "bf16": 1, "bf16x3": 2}
FLAG_TRANSPOSED, FLAG_KL_ACCUM, FLAG_ROWFUSE, FLAG_OUT_F32, FLAG_OUT_BF16, FLAG_GATHER, FLAG_SWAP_SIGNS, FLAG_CONCURRENT = 1, 2, 4, 8, 16, 32, 64, 128
FLAG_REVERSE = 256
E_UNSUPPORTED = -3
STREAM_EPS_W, STREAM_EPS_B, STREAM_SIGN_IN, STREAM_SIGN_OUT, STREAM_OUT_NOISE = 0, 1, 2, 3, 4
STREAM_KL_W, STREAM_KL_B = 5, 6   # BTX-KLMC v1: the sampled KL's own draws (draw j: stream | j << 8)
STREAM_DROP = 7                   # BTX-DROP v1 (include/btx_drop.h): the keep bits of the dropout layers
DROP_ELEMENT, DROP_CHANNEL = 0, 1
DROP_CL, DROP_NCS = 0, 1
DROP_CHUNK, DROP_MAX_ELEMENTS = 8192, 1 << 35
PRIOR_GAUSS_MIX2, PRIOR_LAPLACE, PRIOR_STUDENT_T = 1, 2, 3
# BTX-SVD v1: reduction codes, the log-alpha clamp, the rho of a pruned weight, the layout of the statistics words
REDUCE_MEAN, REDUCE_SUM = 0, 1
LOGALPHA_MAX, RHO_PRUNED = 20.0, -40.0
LOGALPHA_MAX_THRESHOLDS, LOGALPHA_MAX_BINS, LOGALPHA_STATS_WORDS, LOGALPHA_ZERO_MU = 8, 4096, 16, 8
ABI_VERSION = 9
FLAG_LANES_SHIFT = 16
FLAG_LANES_MASK = 0xff << FLAG_LANES_SHIFT
SAMPLE_SKIP_MU = 1


class BtxError(RuntimeError):
    pass


class Geom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "NB", "D", "H", "W", "C", "N", "KD", "KH", "KW", "sd", "sh", "sw", "pd", "ph", "pw",
        "dd", "dh", "dw", "od", "oh", "ow", "groups")]


class Rng(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("sample_idx", ctypes.c_uint32), ("layer_id", ctypes.c_uint32),
                ("sample_idx_dev", ctypes.c_void_p)]


class BnFuse(ctypes.Structure):
    _fields_ = [("residual", ctypes.c_void_p), ("relu", ctypes.c_int32), ("mask", ctypes.c_void_p), ("dres", ctypes.c_void_p)]


class Epilogue(ctypes.Structure):
    _fields_ = [("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("residual", ctypes.c_void_p),
                ("relu", ctypes.c_int32), ("pool", ctypes.c_int32)]


class Lanes(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("x_stride", ctypes.c_int64), ("out_stride", ctypes.c_int64),
                ("res_stride", ctypes.c_int64)]


class PlanInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("family", "ksplits", "kper", "kgroups", "wide", "tall", "par_major", "pool_band",
                                              "nwg", "lanes")] + [("ws_bytes", ctypes.c_uint64)]


FAMILIES = ("gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem", "stem_pool")  # BTX_FAMILY_* order


class Noise(ctypes.Structure):
    _fields_ = [("eps_w", ctypes.c_void_p), ("eps_b", ctypes.c_void_p),
                ("sign_in", ctypes.c_void_p), ("sign_out", ctypes.c_void_p), ("sampled_w", ctypes.c_void_p)]


class SampleItem(ctypes.Structure):
    _fields_ = [("geom", ctypes.POINTER(Geom)), ("mu_w", ctypes.c_void_p), ("rho_w", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("kind", ctypes.c_int32), ("layer_id", ctypes.c_uint32),
                ("src_KW", ctypes.c_int32), ("src_C", ctypes.c_int32)]


class LstmLayer(ctypes.Structure):
    _fields_ = [("mu_w", ctypes.c_void_p), ("rho_w", ctypes.c_void_p), ("mu_b", ctypes.c_void_p), ("rho_b", ctypes.c_void_p),
                ("layer_id", ctypes.c_uint32), ("sample_idx", ctypes.c_uint32), ("sample_idx_dev", ctypes.c_void_p)]


class LstmGrads(ctypes.Structure):
    _fields_ = [("dmu_w", ctypes.c_void_p), ("drho_w", ctypes.c_void_p), ("dmu_b", ctypes.c_void_p), ("drho_b", ctypes.c_void_p)]


class LrtGrads(ctypes.Structure):  # BtxLrtGrads: every member nullable
    _fields_ = [("dmu_w", ctypes.c_void_p), ("drho_w", ctypes.c_void_p), ("dmu_b", ctypes.c_void_p), ("drho_b", ctypes.c_void_p),
                ("dx", ctypes.c_void_p)]


class KlItem(ctypes.Structure):
    _fields_ = [("mu", ctypes.c_void_p), ("rho", ctypes.c_void_p), ("prior_mu_t", ctypes.c_void_p),
                ("prior_sigma_t", ctypes.c_void_p), ("dmu", ctypes.c_void_p), ("drho", ctypes.c_void_p),
                ("prior_mu", ctypes.c_float), ("prior_sigma", ctypes.c_float), ("n", ctypes.c_size_t)]


class Prior(ctypes.Structure):  # BtxPrior
    _fields_ = [("type", ctypes.c_int32), ("loc", ctypes.c_float), ("p0", ctypes.c_float), ("p1", ctypes.c_float),
                ("p2", ctypes.c_float)]


class KlMcItem(ctypes.Structure):  # BtxKlMcItem
    _fields_ = [("mu", ctypes.c_void_p), ("rho", ctypes.c_void_p), ("loc_t", ctypes.c_void_p), ("dmu", ctypes.c_void_p),
                ("drho", ctypes.c_void_p), ("n", ctypes.c_size_t), ("prior", Prior), ("layer_id", ctypes.c_uint32),
                ("rng_stream", ctypes.c_uint32), ("sample_idx", ctypes.c_uint32), ("sample_idx_dev", ctypes.c_void_p)]


class KlLogUItem(ctypes.Structure):  # BtxKlLogUItem
    _fields_ = [("mu", ctypes.c_void_p), ("rho", ctypes.c_void_p), ("dmu", ctypes.c_void_p), ("drho", ctypes.c_void_p),
                ("n", ctypes.c_size_t), ("reduction", ctypes.c_int32)]


class LogAlphaItem(ctypes.Structure):  # BtxLogAlphaItem
    _fields_ = [("mu", ctypes.c_void_p), ("rho", ctypes.c_void_p), ("n", ctypes.c_size_t)]


class Q8Chain(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("s_sigma", "s_mu", "s_eps", "inv_s_eps", "s_d", "inv_s_d", "inv_s_w")] + \
               [("bias_div", ctypes.c_double)]


class Q8Add(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("s_a", "pre_a", "s_b", "pre_b", "inv_s")] + \
               [("zero_point", ctypes.c_int32), ("relu", ctypes.c_int32)]


class Q8Delta(ctypes.Structure):
    _fields_ = [("inv_s_eps", ctypes.c_float), ("mult", ctypes.c_float), ("mean_bias", ctypes.c_int32), ("pert_bias", ctypes.c_int32),
                ("div_mean", ctypes.c_double), ("div_pert", ctypes.c_double)]


class Q8Flipout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("z_x", "z_xp", "z_mean", "z_pert", "z_p2", "sin_pos", "sin_neg", "sout_pos", "sout_neg")] + \
               [(n, ctypes.c_float) for n in ("mult_xp", "mult_mean", "mult_pert", "mult_p2", "out_scale")]


class OptimItem(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("state0", ctypes.c_void_p), ("state1", ctypes.c_void_p),
                ("n", ctypes.c_int64)]


class BucketItem(ctypes.Structure):  # K14: n elements at src <-> bucket + offset
    _fields_ = [("src", ctypes.c_void_p), ("offset", ctypes.c_int64), ("n", ctypes.c_int64)]


class OptimHyper(ctypes.Structure):  # the DEVICE block of BTX-OPT v1: 16 words, filled on the host and copied
    _fields_ = [(n, ctypes.c_float) for n in ("neg_lr", "wd", "decay_mul", "one_m_b1", "b2", "one_m_b2", "eps", "neg_step_size",
                                              "bc2s", "momentum", "one_m_damp")] + \
               [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


OPT_MAXIMIZE, OPT_NESTEROV, OPT_DECOUPLED, OPT_FIRST_STEP, OPT_COUPLED_WD = 1, 2, 4, 8, 16
OPTIM_CHUNK, OPTIM_MAX_ITEMS = 4096, 65536
Q8_BIAS_NONE, Q8_BIAS_MU, Q8_BIAS_SIGMA_EPS = 0, 1, 2

EXPORTS = ("btx_abi_version", "btx_strerror", "btx_kl_workspace_bytes", "btx_kl_gauss", "btx_kl_model_workspace_bytes",
           "btx_kl_gauss_model", "btx_kl_gauss_model_bwd", "btx_contract_wgrad",
           "btx_contract_workspace_bytes", "btx_contract_fwd", "btx_contract_fwd_ex", "btx_contract_fwd_lanes", "btx_contract_pool_shape", "btx_contract_plan_info", "btx_out_shape", "btx_fill_eps", "btx_fill_sign", "btx_rho_grad",
           "btx_mc_packed_floats", "btx_mc_accumulate", "btx_mc_accumulate_lanes", "btx_sampled_w_bytes", "btx_sample_weights", "btx_sampled_w_bytes_lanes", "btx_sample_weights_lanes", "btx_rowfuse_pack", "btx_maxpool2d_cl", "btx_avgpool_global_cl",
           "btx_bn_workspace_bytes", "btx_bn_train_fwd", "btx_bn_train_bwd", "btx_dgrad_weights",
           "btx_wgrad_workspace_bytes", "btx_contract_wgrad_ws", "btx_maxpool2d_cl_train", "btx_maxpool2d_cl_bwd",
           "btx_lstm_workspace_bytes", "btx_lstm_fwd", "btx_lstm_train_saved_bytes", "btx_lstm_train_workspace_bytes",
           "btx_lstm_fwd_train", "btx_lstm_bwd",
           "btx_calib_workspace_bytes", "btx_avu_fwd", "btx_avu_bwd", "btx_eau_fwd", "btx_eau_bwd",
           "btx_q8_weight_row_bytes", "btx_q8_quantize_act", "btx_q8_sample_weights", "btx_q8_contract",
           "btx_q8_add", "btx_q8_contract_res", "btx_q8_maxpool2d_cl", "btx_q8_avgpool2d_cl",
           "btx_q8_sample_delta", "btx_q8_contract_flipout",
           "btx_optim_sgd", "btx_optim_adam", "btx_optim_grad_norm_workspace_bytes", "btx_optim_grad_norm",
           "btx_mcloss_workspace_bytes", "btx_mc_ce_fwd", "btx_mc_ce_bwd", "btx_avu_mc_fwd", "btx_avu_mc_bwd",
           "btx_bias_grad_workspace_bytes", "btx_bias_grad",
           "btx_bucket_pack", "btx_bucket_unpack",
           "btx_mc_eval_state_doubles", "btx_mc_eval_workspace_bytes", "btx_mc_eval",
           "btx_mc_moments_lanes", "btx_mc_gnll_workspace_bytes", "btx_mc_gnll_fwd", "btx_mc_gnll_bwd",
           "btx_reg_eval_workspace_bytes", "btx_reg_eval_update",
           "btx_lrt_fwd_train", "btx_lrt_bwd_workspace_bytes", "btx_lrt_bwd",
           "btx_kl_mc_workspace_bytes", "btx_kl_mc_model", "btx_kl_mc_model_bwd",
           "btx_kl_logu_workspace_bytes", "btx_kl_logu_model", "btx_kl_logu_model_bwd", "btx_logalpha_stats", "btx_logalpha_prune")
# include/btx_drop.h: entry points added to ABI 9 in a header of their own (EXPORTS stays what include/btx.h declares)
EXPORTS_DROP = ("btx_dropout_fwd", "btx_dropout_bwd")
MC_EVAL_MAX_CLASSES, MC_EVAL_MAX_BINS, MC_EVAL_MAX_THRESHOLDS = 24575, 64, 32
MC_EVAL_HEADER, MC_EVAL_CURSOR, MC_EVAL_DROPPED = 16, 11, 12
REG_EVAL_MAX_LEVELS, REG_EVAL_HEADER, REG_EVAL_CURSOR, REG_EVAL_DROPPED = 8, 16, 9, 10
REG_CHUNK = 4096


def lib_path():
    # BTX_LIB: alternative build of the same ABI (A/B measurements of kernel variants)
    return os.environ.get("BTX_LIB") or os.path.join(_HERE, "libbtx.so")


def lib():
    """Load libbtx.so once.  Raises BtxError (loudly) when the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise BtxError("libbtx.so not found at %s — build it with `python __graft_entry__.py build` "
                       "(hipcc --offload-arch=gfx950); there is no fallback path." % path)
    L = ctypes.CDLL(path)
    vp, sz, u32, i32, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
    L.btx_abi_version.restype = i32
    L.btx_abi_version.argtypes = []
    L.btx_strerror.restype = ctypes.c_char_p
    L.btx_strerror.argtypes = [i32]
    L.btx_kl_workspace_bytes.restype = sz
    L.btx_kl_workspace_bytes.argtypes = [sz]
    L.btx_kl_gauss.restype = i32
    L.btx_kl_gauss.argtypes = [vp, vp, sz, vp, vp, f32, f32, vp, u32, vp, sz, vp]
    L.btx_kl_model_workspace_bytes.restype = sz
    L.btx_kl_model_workspace_bytes.argtypes = [i32]
    L.btx_kl_gauss_model.restype = i32
    L.btx_kl_gauss_model.argtypes = [ctypes.POINTER(KlItem), i32, vp, vp, sz, vp]
    L.btx_kl_gauss_model_bwd.restype = i32
    L.btx_kl_gauss_model_bwd.argtypes = [ctypes.POINTER(KlItem), i32, vp, vp]
    L.btx_contract_wgrad.restype = i32
    L.btx_contract_wgrad.argtypes = [i32, ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, ctypes.POINTER(Rng),
                                     ctypes.POINTER(Noise), i32, u32, vp]
    L.btx_contract_wgrad_ws.restype = i32
    L.btx_contract_wgrad_ws.argtypes = [i32, ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, ctypes.POINTER(Rng),
                                        ctypes.POINTER(Noise), i32, u32, vp, sz, vp, vp, vp]
    L.btx_wgrad_workspace_bytes.restype = sz
    L.btx_wgrad_workspace_bytes.argtypes = [i32, ctypes.POINTER(Geom), i32, u32]
    L.btx_contract_workspace_bytes.restype = sz
    L.btx_contract_workspace_bytes.argtypes = [ctypes.POINTER(Geom), i32, i32, i32, u32]
    L.btx_contract_fwd.restype = i32
    L.btx_contract_fwd.argtypes = [i32, ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, ctypes.POINTER(Rng),
                                   ctypes.POINTER(Noise), i32, i32, u32, vp, sz, vp]
    L.btx_contract_fwd_ex.restype = i32
    L.btx_contract_fwd_ex.argtypes = L.btx_contract_fwd.argtypes + [ctypes.POINTER(Epilogue)]
    L.btx_contract_fwd_lanes.restype = i32
    L.btx_contract_fwd_lanes.argtypes = L.btx_contract_fwd_ex.argtypes + [ctypes.POINTER(Lanes)]
    L.btx_contract_plan_info.restype = i32
    L.btx_contract_plan_info.argtypes = [i32, ctypes.POINTER(Geom), i32, i32, u32, ctypes.POINTER(Epilogue), ctypes.POINTER(PlanInfo)]
    L.btx_contract_pool_shape.restype = i32
    L.btx_contract_pool_shape.argtypes = [ctypes.POINTER(Geom), i32, i32, u32] + [ctypes.POINTER(ctypes.c_int32)] * 2
    L.btx_out_shape.restype = i32
    L.btx_out_shape.argtypes = [ctypes.POINTER(Geom), u32] + [ctypes.POINTER(ctypes.c_int32)] * 3
    L.btx_fill_eps.restype = i32
    L.btx_fill_eps.argtypes = [vp, sz, ctypes.POINTER(Rng), u32, vp]
    L.btx_rho_grad.restype = i32
    L.btx_rho_grad.argtypes = [vp, vp, vp, sz, ctypes.POINTER(Rng), u32, vp]
    L.btx_fill_sign.restype = i32
    L.btx_fill_sign.argtypes = [vp, sz, ctypes.POINTER(Rng), u32, vp]
    L.btx_mc_packed_floats.restype = sz
    L.btx_mc_packed_floats.argtypes = [i32, i32]
    L.btx_sampled_w_bytes.restype = sz
    L.btx_sampled_w_bytes.argtypes = [ctypes.POINTER(Geom), i32, i32]
    L.btx_sample_weights.restype = i32
    L.btx_sample_weights.argtypes = [ctypes.POINTER(SampleItem), i32, ctypes.POINTER(Rng), i32, vp]
    L.btx_sampled_w_bytes_lanes.restype = sz
    L.btx_sampled_w_bytes_lanes.argtypes = [ctypes.POINTER(Geom), i32, i32, i32]
    L.btx_sample_weights_lanes.restype = i32
    L.btx_sample_weights_lanes.argtypes = [ctypes.POINTER(SampleItem), i32, ctypes.POINTER(Rng), i32, vp, i32, u32]
    L.btx_rowfuse_pack.restype = i32
    L.btx_rowfuse_pack.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int64), i32, i32, i32, i32, vp, i32, i32, i32, i32, i32,
                                   i32, vp]
    L.btx_maxpool2d_cl.restype = i32
    L.btx_maxpool2d_cl.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.btx_maxpool2d_cl_train.restype = i32
    L.btx_maxpool2d_cl_train.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.btx_maxpool2d_cl_bwd.restype = i32
    L.btx_maxpool2d_cl_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.btx_avgpool_global_cl.restype = i32
    L.btx_avgpool_global_cl.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.btx_mc_accumulate.restype = i32
    L.btx_mc_accumulate.argtypes = [vp, i32, i32, i32, f32, vp, vp]
    L.btx_mc_accumulate_lanes.restype = i32
    L.btx_mc_accumulate_lanes.argtypes = [vp, i32, i32, i32, i32, f32, vp, vp]
    i64 = ctypes.c_longlong
    L.btx_bn_workspace_bytes.restype = sz
    L.btx_bn_workspace_bytes.argtypes = [i64, i32]
    L.btx_bn_train_fwd.restype = i32
    L.btx_bn_train_fwd.argtypes = [vp, vp, i32, i64, i32, vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, ctypes.POINTER(BnFuse), vp, sz, vp]
    L.btx_bn_train_bwd.restype = i32
    L.btx_bn_train_bwd.argtypes = [vp, vp, vp, i32, i64, i32, vp, i32, vp, vp, vp, vp, ctypes.POINTER(BnFuse), vp, sz, vp]
    L.btx_dgrad_weights.restype = i32
    L.btx_dgrad_weights.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(Rng), vp]
    L.btx_lstm_workspace_bytes.restype = sz
    L.btx_lstm_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.btx_lstm_fwd.restype = i32
    L.btx_lstm_fwd.argtypes = [i32, ctypes.POINTER(LstmLayer), ctypes.POINTER(LstmLayer), ctypes.c_uint64, vp, i32, vp, vp, vp, vp,
                               vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]
    L.btx_lstm_train_saved_bytes.restype = sz
    L.btx_lstm_train_saved_bytes.argtypes = [i32, i32, i32]
    L.btx_lstm_train_workspace_bytes.restype = sz
    L.btx_lstm_train_workspace_bytes.argtypes = [i32, i32, i32]
    L.btx_lstm_fwd_train.restype = i32
    L.btx_lstm_fwd_train.argtypes = [i32, ctypes.POINTER(LstmLayer), ctypes.POINTER(LstmLayer), ctypes.c_uint64, vp, vp, vp, vp,
                                     vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, sz, vp]
    L.btx_lstm_bwd.restype = i32
    L.btx_lstm_bwd.argtypes = [i32, ctypes.POINTER(LstmLayer), ctypes.POINTER(LstmLayer), ctypes.c_uint64, vp, vp, vp, vp, vp, vp,
                               vp, vp, vp, vp, ctypes.POINTER(LstmGrads), ctypes.POINTER(LstmGrads), i32, i32, i32, i32, i32,
                               i32, vp, sz, vp]
    L.btx_calib_workspace_bytes.restype = sz
    L.btx_calib_workspace_bytes.argtypes = [i32]
    L.btx_avu_fwd.restype = i32
    L.btx_avu_fwd.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, f32, vp, vp, sz, vp]
    L.btx_avu_bwd.restype = i32
    L.btx_avu_bwd.argtypes = [vp, i32, i32, i32, vp, vp, vp, sz, vp, vp]
    L.btx_eau_fwd.restype = i32
    L.btx_eau_fwd.argtypes = [vp, vp, i32, i32, f32, vp, f32, vp, f32, vp, vp, sz, vp]
    L.btx_eau_bwd.restype = i32
    L.btx_eau_bwd.argtypes = [vp, vp, i32, i32, vp, vp, sz, vp, vp, vp]
    L.btx_q8_weight_row_bytes.restype = sz
    L.btx_q8_weight_row_bytes.argtypes = [i32, i32]
    L.btx_q8_quantize_act.restype = i32
    L.btx_q8_quantize_act.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int64), vp, i32, i32, i32, i32, f32, i32, vp]
    L.btx_q8_sample_weights.restype = i32
    L.btx_q8_sample_weights.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(Q8Chain), ctypes.POINTER(Rng), vp, vp,
                                        vp, vp, vp, vp]
    L.btx_q8_contract.restype = i32
    L.btx_q8_contract.argtypes = [ctypes.POINTER(Geom), vp, i32, vp, vp, vp, f32, i32, i32, i32, f32, vp, vp]
    L.btx_q8_add.restype = i32
    L.btx_q8_add.argtypes = [vp, vp, vp, sz, ctypes.POINTER(Q8Add), vp]
    L.btx_q8_contract_res.restype = i32
    L.btx_q8_contract_res.argtypes = [ctypes.POINTER(Geom), vp, i32, vp, vp, vp, f32, i32, i32, i32, vp, ctypes.POINTER(Q8Add), vp, vp]
    L.btx_q8_maxpool2d_cl.restype = i32
    L.btx_q8_maxpool2d_cl.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.btx_q8_avgpool2d_cl.restype = i32
    L.btx_q8_avgpool2d_cl.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.btx_q8_sample_delta.restype = i32
    L.btx_q8_sample_delta.argtypes = [vp, vp, vp, i32, i32, i32, i32, ctypes.POINTER(Q8Delta), ctypes.POINTER(Rng), vp, vp, vp, vp, vp,
                                      vp, vp]
    L.btx_q8_contract_flipout.restype = i32
    L.btx_q8_contract_flipout.argtypes = [ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Q8Flipout),
                                          ctypes.POINTER(Q8Add), ctypes.POINTER(Rng), i32, vp, vp, i32, vp, vp]
    L.btx_optim_sgd.restype = i32
    L.btx_optim_sgd.argtypes = [ctypes.POINTER(OptimItem), i32, vp, i32, vp, vp]
    L.btx_optim_adam.restype = i32
    L.btx_optim_adam.argtypes = [ctypes.POINTER(OptimItem), i32, vp, vp, vp]
    L.btx_optim_grad_norm_workspace_bytes.restype = sz
    L.btx_optim_grad_norm_workspace_bytes.argtypes = [i32, ctypes.c_int64]
    L.btx_optim_grad_norm.restype = i32
    L.btx_optim_grad_norm.argtypes = [ctypes.POINTER(OptimItem), i32, f32, vp, vp, sz, vp]
    L.btx_mcloss_workspace_bytes.restype = sz
    L.btx_mcloss_workspace_bytes.argtypes = [i32, i32]
    L.btx_mc_ce_fwd.restype = i32
    L.btx_mc_ce_fwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, f32, vp, vp, sz, vp]
    L.btx_mc_ce_bwd.restype = i32
    L.btx_mc_ce_bwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, sz, vp, vp]
    L.btx_avu_mc_fwd.restype = i32
    L.btx_avu_mc_fwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, f32, vp, vp, sz, vp]
    L.btx_avu_mc_bwd.restype = i32
    L.btx_avu_mc_bwd.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp, vp]
    L.btx_bias_grad_workspace_bytes.restype = sz
    L.btx_bias_grad_workspace_bytes.argtypes = [ctypes.c_int64, i32]
    L.btx_bias_grad.restype = i32
    L.btx_bias_grad.argtypes = [i32, vp, ctypes.c_int64, i32, i32, vp, vp, ctypes.POINTER(Rng), vp, ctypes.c_uint32, vp, sz, vp]
    L.btx_bucket_pack.restype = i32
    L.btx_bucket_pack.argtypes = [ctypes.POINTER(BucketItem), i32, f32, vp, vp]
    L.btx_bucket_unpack.restype = i32
    L.btx_bucket_unpack.argtypes = [ctypes.POINTER(BucketItem), i32, vp, vp]
    L.btx_mc_eval_state_doubles.restype = sz
    L.btx_mc_eval_state_doubles.argtypes = [i32, i32]
    L.btx_mc_eval_workspace_bytes.restype = sz
    L.btx_mc_eval_workspace_bytes.argtypes = [i32]
    L.btx_mc_eval.restype = i32
    L.btx_mc_eval.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, sz, vp, ctypes.c_int64, vp, sz, vp]
    f64 = ctypes.c_double
    L.btx_mc_moments_lanes.restype = i32
    L.btx_mc_moments_lanes.argtypes = [vp, i32, i32, i32, i32, i32, f64, vp, vp]
    L.btx_mc_gnll_workspace_bytes.restype = sz
    L.btx_mc_gnll_workspace_bytes.argtypes = [i32, i32]
    L.btx_mc_gnll_fwd.restype = i32
    L.btx_mc_gnll_fwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, sz, vp]
    L.btx_mc_gnll_bwd.restype = i32
    L.btx_mc_gnll_bwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp]
    L.btx_reg_eval_workspace_bytes.restype = sz
    L.btx_reg_eval_workspace_bytes.argtypes = [i32, i32]
    L.btx_reg_eval_update.restype = i32
    L.btx_reg_eval_update.argtypes = [vp, vp, i32, i32, f64, f64, vp, i32, vp, sz, vp, ctypes.c_int64, vp, sz, vp]
    L.btx_lrt_fwd_train.restype = i32
    L.btx_lrt_fwd_train.argtypes = [ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Rng), i32, i32, u32, vp]
    L.btx_lrt_bwd_workspace_bytes.restype = i32
    L.btx_lrt_bwd_workspace_bytes.argtypes = [ctypes.POINTER(Geom), i32, i32, ctypes.POINTER(sz)]
    L.btx_lrt_bwd.restype = i32
    L.btx_lrt_bwd.argtypes = [ctypes.POINTER(Geom), vp, vp, vp, vp, vp, vp, ctypes.POINTER(LrtGrads), ctypes.POINTER(Rng), i32, i32,
                              vp, sz, vp]
    L.btx_kl_mc_workspace_bytes.restype = sz
    L.btx_kl_mc_workspace_bytes.argtypes = [i32]
    L.btx_kl_mc_model.restype = i32
    L.btx_kl_mc_model.argtypes = [ctypes.POINTER(KlMcItem), i32, ctypes.c_uint64, i32, vp, u32, vp, sz, vp]
    L.btx_kl_mc_model_bwd.restype = i32
    L.btx_kl_mc_model_bwd.argtypes = [ctypes.POINTER(KlMcItem), i32, ctypes.c_uint64, i32, vp, vp]
    L.btx_kl_logu_workspace_bytes.restype = sz
    L.btx_kl_logu_workspace_bytes.argtypes = [i32]
    L.btx_kl_logu_model.restype = i32
    L.btx_kl_logu_model.argtypes = [ctypes.POINTER(KlLogUItem), i32, vp, vp, u32, vp, sz, vp]
    L.btx_kl_logu_model_bwd.restype = i32
    L.btx_kl_logu_model_bwd.argtypes = [ctypes.POINTER(KlLogUItem), i32, vp, vp]
    L.btx_logalpha_stats.restype = i32
    L.btx_logalpha_stats.argtypes = [ctypes.POINTER(LogAlphaItem), i32, ctypes.POINTER(ctypes.c_float), i32, i32, vp, vp, vp]
    L.btx_logalpha_prune.restype = i32
    L.btx_logalpha_prune.argtypes = [ctypes.POINTER(LogAlphaItem), i32, ctypes.c_float, vp, vp]
    L.btx_dropout_fwd.restype = i32
    L.btx_dropout_fwd.argtypes = [vp, vp, i32, i64, i64, i64, i32, i32, u32, f32, i32, i64, ctypes.POINTER(Rng), vp]
    L.btx_dropout_bwd.restype = i32
    L.btx_dropout_bwd.argtypes = [vp, vp, i32, i64, i64, i64, i32, i32, u32, f32, ctypes.POINTER(Rng), vp]
    if L.btx_abi_version() != ABI_VERSION:
        raise BtxError("libbtx.so ABI %d != expected %d" % (L.btx_abi_version(), ABI_VERSION))
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        raise BtxError("libbtx: %s (code %d)" % (lib().btx_strerror(rc).decode(), rc))
