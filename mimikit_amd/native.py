"""ctypes binding of ``libmmk_hip.so`` (the C ABI declared in ``include/mmk.h``).

The library is the only compute path of this package: there is no CPU or
eager-PyTorch fallback.  Every wrapper takes torch tensors that already live on
a HIP device, passes raw ``data_ptr()``s and enqueues on torch's current HIP
stream.  A missing library, or a tensor that is not on a HIP device, raises.
"""
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MMK_DIAG_LIB (read once, at import): "1" selects the diagnostic build (`python -m mimikit_amd.build --diag`): the same library with
# in-kernel phase stamps and the timing experiments compiled in; the path of a `.so` selects that file (the A/B variants of
# scripts/build_variant.sh: loaded from where they lie, the product library is never overwritten).  Unset or empty: the product library,
# which contains neither and must carry the digest of the tree's sources
_DIAG = os.environ.get("MMK_DIAG_LIB", "")
DIAGNOSTIC = _DIAG != ""
LIB_PATH = (os.path.join(_HERE, "libmmk_hip_diag.so") if _DIAG == "1" else os.path.abspath(_DIAG) if _DIAG.endswith(".so")
            else os.path.join(_HERE, "libmmk_hip.so"))
if DIAGNOSTIC and _DIAG != "1" and not _DIAG.endswith(".so"):
    raise ImportError(f"MMK_DIAG_LIB={_DIAG!r}: expected 1 (the diagnostic build) or the path of a library variant (*.so)")

MAX_LAYERS, MAX_COND, MAX_TIERS, MAX_STREAMS = 128, 4, 8, 4
ABI_VERSION = 6          # include/mmk.h: MMK_ABI_VERSION (bumped whenever a config struct or a signature changes)
ACT = {"none": 0, None: 0, "Identity": 0, "Tanh": 1, "Sigmoid": 2, "Mish": 3, "Abs": 4, "ReLU": 5, "Softplus": 6, "Sin": 7, "Cos": 8}      # include/mmk.h: MMK_ACT_*

i32, i64, f32, vp, cp = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_char_p


def only_mlp(estimator) -> bool:
    """an MLPIO's estimator: Sequential(MLP) - or Sequential(MLP, Dropout[, Dropout1d]): IOModule.wrap hangs the spec's dropout modules behind the core as
    well (modules/io.py:94-97); identities in eval mode, which mlp_head_problem insists on"""
    return (isinstance(estimator, torch.nn.Sequential) and len(estimator) >= 1 and type(estimator[0]).__name__ == "MLP"
            and all(isinstance(m, (torch.nn.Dropout, torch.nn.Dropout1d)) for m in list(estimator)[1:]))


def mlp_head_problem(mlp, training: bool):
    """what keeps an MLP head (networks/mlp.py:20-63) off the HIP path, or None: its activation must be one the kernels evaluate (ACT), its Linears need their
    bias, and Dropout / Dropout1d modules are identities only in eval mode (where the generate loop runs a network, loops/generate.py)"""
    if type(mlp.activation).__name__ not in ACT:
        return f"MLP head activation {type(mlp.activation).__name__}"
    if not mlp.bias:
        return "MLP head without bias"
    if (mlp.dropout or mlp.dropout1d) and training:
        return "MLP head with dropout in training mode"
    return None


def mlp_act(mlp) -> int:
    return ACT[type(mlp.activation).__name__]


def mlp_linear_keys(sd: dict, prefix: str, mlp) -> dict:
    """``fc`` of an MLP is Sequential(Linear, act, *dropouts, [Linear, act, *dropouts] * n, Linear) (networks/mlp.py:42-53): with dropout modules in it the
    Linears sit at indices i (2 + n_dropouts), and the plans bind ``fc.{2 i}``.  Returns ``sd`` with the head's keys under the names the plans know."""
    n_dp = int(mlp.dropout > 0) + int(mlp.dropout1d > 0)
    if n_dp == 0:
        return sd
    out = {k: v for k, v in sd.items() if not k.startswith(prefix + "fc.")}
    for i in range(mlp.n_hidden_layers + 2):
        for leaf in ("weight", "bias"):
            src = f"{prefix}fc.{i * (2 + n_dp)}.{leaf}"
            if src in sd:
                out[f"{prefix}fc.{2 * i}.{leaf}"] = sd[src]
    return out


class NativeError(RuntimeError):
    pass


WN_BPIPE_MIN_CLIPS = 105  # csrc/wavenet_plan.hip: kBpipeMinClips (tests/test_host_logic.py holds the two together)
WN_BPIPE_ALWAYS_CLIPS = 129  # csrc/wavenet_plan.hip: kBpipeAlwaysClips = one more than a ring takes


def wn_bpipe_by_default(batch: int) -> bool:
    """csrc/wavenet_plan.hip: bpipe_by_default - which batches of a stage-pipeline network run in groups of 16 clips (wavenet_bpipe.hip) unless the plan
    switch MMK_WN_BPIPE says otherwise: more than one ring's 128, and from 105 on the counts the ring's two-clip visits do not take (odd ones)"""
    return batch >= WN_BPIPE_ALWAYS_CLIPS or (batch >= WN_BPIPE_MIN_CLIPS and batch % 2 != 0)
TUNING_CHARS = 256        # include/mmk.h: MMK_TUNING_CHARS

# Execution switches handed to every plan this process creates, as {"MMK_WN_CHAIN": "0", ...} (merged under a network's own
# ``exec_tuning``).  They travel inside the plan's config (``tuning``): the library reads no environment variable, so nothing outside
# this dictionary and the network decides which kernel a plan gets.  The parity tests use it to put one network on every kernel.
PLAN_TUNING: Dict[str, str] = {}


def tuning_text(*dicts) -> bytes:
    merged = {}
    for d in dicts:
        merged.update(d or {})
    text = ";".join(f"{k}={v}" for k, v in merged.items())
    if len(text) >= TUNING_CHARS:
        raise ValueError(f"execution switches do not fit the config's {TUNING_CHARS} characters: {text}")
    return text.encode()


class WaveNetConfig(C.Structure):
    _fields_ = [
        ("n_layers", i32), ("kernel_size", i32 * MAX_LAYERS), ("dilation", i32 * MAX_LAYERS),
        ("q_levels", i32), ("in_dim", i32), ("dim_dilated", i32), ("residuals_dim", i32), ("skips_dim", i32),
        ("n_cond", i32), ("cond_in_dim", i32 * MAX_COND), ("cond_dim", i32 * MAX_COND), ("cond_q_levels", i32 * MAX_COND),
        ("bias", i32), ("gated", i32), ("act_f", i32), ("act_g", i32), ("head_kind", i32), ("mlp_hidden", i32), ("mlp_n_hidden", i32), ("mlp_act", i32),
        ("out_dim", i32), ("learn_temp", i32), ("min_temp", f32), ("max_batch", i32),
        ("res_explicit", i32), ("layer_has_res", i32 * MAX_LAYERS), ("layerwise_inputs", i32), ("exec_mode", i32), ("with_affine_residuals", i32),
        ("n_targets", i32), ("x_out_dim", i32 * MAX_STREAMS), ("x_mlp_hidden", i32 * MAX_STREAMS), ("x_mlp_n_hidden", i32 * MAX_STREAMS),
        ("x_learn_temp", i32 * MAX_STREAMS), ("x_min_temp", f32 * MAX_STREAMS),
        ("tuning", C.c_char * TUNING_CHARS),
    ]


class SrnnConfig(C.Structure):
    _fields_ = [
        ("n_tiers", i32), ("frame_size", i32 * MAX_TIERS), ("hidden_dim", i32), ("rnn_kind", i32),
        ("rnn_bias", i32), ("h0_ones", i32), ("q_levels", i32), ("mlp_hidden", i32), ("mlp_n_hidden", i32),
        ("learn_temp", i32), ("mlp_act", i32), ("min_temp", f32), ("max_batch", i32), ("n_rnn", i32), ("exec_mode", i32),
        ("n_inputs", i32), ("n_targets", i32), ("inputs_mode", i32), ("in_class", i32 * MAX_STREAMS),
        ("x_q_levels", i32 * MAX_STREAMS), ("x_mlp_hidden", i32 * MAX_STREAMS), ("x_mlp_n_hidden", i32 * MAX_STREAMS),
        ("x_learn_temp", i32 * MAX_STREAMS), ("x_min_temp", f32 * MAX_STREAMS),
        ("tuning", C.c_char * TUNING_CHARS),
    ]


class S2SConfig(C.Structure):
    _fields_ = [
        ("in_dim", i32), ("out_dim", i32), ("model_dim", i32), ("hop", i32), ("enc_n_lstm", i32),
        ("dec_n_lstm", i32), ("out_abs", i32), ("max_batch", i32), ("enc_downsampling", i32), ("dec_upsampling", i32),
        ("enc_apply_residuals", i32), ("dec_apply_residuals", i32),
        ("in_classes", i32), ("head_kind", i32), ("mlp_hidden", i32), ("mlp_n_hidden", i32), ("mlp_act", i32), ("learn_temp", i32), ("min_temp", f32),
        ("exec_mode", i32),
        ("tuning", C.c_char * TUNING_CHARS),
    ]


class TransformerConfig(C.Structure):
    _fields_ = [
        ("model_dim", i32), ("n_heads", i32), ("feedforward_dim", i32), ("num_layers", i32), ("rf", i32), ("final_norm", i32),
        ("in_kind", i32), ("in_classes", i32), ("in_dim", i32), ("head_kind", i32), ("out_dim", i32), ("out_abs", i32),
        ("mlp_hidden", i32), ("mlp_n_hidden", i32), ("mlp_act", i32), ("learn_temp", i32), ("min_temp", f32), ("max_batch", i32),
        ("tuning", C.c_char * TUNING_CHARS),
    ]


_SIGNATURES = {
    "mmk_abi_version": (i32, []),
    "mmk_config_bytes": (i64, [i32]),
    "mmk_build_digest": (cp, []),
    "mmk_last_error": (cp, []),
    "mmk_pack_launch_count": (i64, []),
    "mmk_fingerprint_u32": (i32, [vp, i64, vp, vp]),
    "mmk_fingerprint_buffers_u32": (i32, [vp, vp, i32, vp, vp]),
    "mmk_mulaw_compress_f32_i64": (i32, [vp, vp, i64, i32, f32, vp, vp]),
    "mmk_mulaw_expand_i64_f32": (i32, [vp, vp, i64, i32, f32, vp, vp]),
    "mmk_resample_n_out": (i64, [i64, i32, i32]),
    "mmk_resample_f32": (i32, [vp, i64, i32, i64, vp, i32, i32, i32, vp, i64, vp]),
    "mmk_lfilter1_workspace_floats": (C.c_size_t, [i32, i64]),
    "mmk_lfilter1_f32": (i32, [vp, i64, i32, i64, f32, f32, f32, vp, i64, vp, vp]),
    "mmk_row_normalize_workspace_floats": (C.c_size_t, [i32, i64]),
    "mmk_row_normalize_f32": (i32, [vp, i64, i32, i64, i32, f32, vp, i64, vp, vp]),
    "mmk_inv_row_norm_f32": (i32, [vp, i64, i64, i32, i64, i32, vp, vp]),
    "mmk_cosine_cost_f32": (i32, [vp, i64, i64, vp, i32, i32, vp, i64, vp, i64, i32, vp, vp]),
    "mmk_dtw_subseq_f32": (i32, [vp, i32, i32, i64, vp, vp, vp, vp]),
    "mmk_nn_cosine_workspace_bytes": (C.c_size_t, [i64, i64]),
    "mmk_nn_cosine_f32": (i32, [vp, i64, vp, i64, vp, i64, vp, i64, i32, vp, vp, vp, C.c_size_t, vp]),
    "mmk_cum_entropy_i64": (i32, [vp, i64, i32, i64, vp, vp, i64, vp]),
    "mmk_nn_cosine_self_f32": (i32, [vp, i64, vp, i64, i32, vp, vp, vp, C.c_size_t, vp]),
    "mmk_nn_components_workspace_bytes": (C.c_size_t, [i64]),
    "mmk_nn_components_i64": (i32, [vp, i64, vp, vp, vp, C.c_size_t, vp]),
    "mmk_segment_mean_f32": (i32, [vp, i64, i64, i32, vp, vp, i64, vp, i64, vp]),
    "mmk_nn_topk_workspace_bytes": (C.c_size_t, [i64, i64, i32]),
    "mmk_nn_topk_f32": (i32, [vp, i64, vp, i64, vp, i64, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, vp, C.c_size_t, vp]),
    "mmk_half_neg_sqnorm_f32": (i32, [vp, i64, i64, i32, vp, vp]),
    "mmk_edge_components_workspace_bytes": (C.c_size_t, [i64]),
    "mmk_edge_components_i64": (i32, [vp, vp, i64, i64, vp, vp, vp, C.c_size_t, vp]),
    "mmk_pca_colstats_workspace_bytes": (C.c_size_t, [i64, i32]),
    "mmk_pca_colstats_f64": (i32, [vp, i64, i64, i32, vp, vp, vp, C.c_size_t, vp]),
    "mmk_pca_cov_workspace_bytes": (C.c_size_t, [i64, i32]),
    "mmk_pca_cov_f64": (i32, [vp, i64, i64, i32, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_pca_eig_workspace_bytes": (C.c_size_t, [i32, i32]),
    "mmk_pca_eig_f64": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_pca_project_f32": (i32, [vp, i64, i64, i32, vp, vp, vp, i32, vp, i64, vp]),
    "mmk_stft_n_frames": (i64, [i64, i32, i32, i32]),
    "mmk_stft_mag_f32": (i32, [vp, i64, i32, i64, i32, i32, i32, vp, vp]),
    "mmk_stft_f32": (i32, [vp, i64, i32, i64, i32, i32, i32, i32, i32, vp, vp]),
    "mmk_stft_energy_f32": (i32, [vp, i64, i32, i64, i32, i32, i32, i32, vp, vp]),
    "mmk_interp1d_f32": (i32, [vp, i64, i32, i64, vp, i64, i64, i32, i32, vp]),
    "mmk_derivative_f32": (i32, [vp, i64, i32, i64, i32, vp, i64, vp]),
    "mmk_hpss_f32": (i32, [vp, i64, i64, i32, i64, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, i64, i64, vp]),
    "mmk_melbank_f32": (i32, [vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp]),
    "mmk_stft_mel_f32": (i32, [vp, i64, i32, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp]),
    "mmk_novelty_f32": (i32, [vp, i64, i64, vp, i32, i64, i32, vp, i32, vp, vp]),
    "mmk_novelty_finish_workspace_floats": (C.c_size_t, [i32, i32, i64]),
    "mmk_novelty_finish_f32": (i32, [vp, i32, i32, i64, vp, vp, vp, C.c_size_t, vp]),
    "mmk_pick_peaks_workspace_bytes": (C.c_size_t, [i64]),
    "mmk_pick_peaks_f32": (i32, [vp, i64, i32, i32, C.c_double, vp, vp, C.c_size_t, vp]),
    "mmk_istft_n_samples": (i64, [i64, i32, i32]),
    "mmk_istft_workspace_floats": (C.c_size_t, [i32, i64, i32]),
    "mmk_istft_f32": (i32, [vp, i32, i32, i64, i32, i32, vp, vp, vp]),
    "mmk_gla_workspace_floats": (C.c_size_t, [i32, i64, i32, i32]),
    "mmk_gla_f32": (i32, [vp, vp, i32, i64, i32, i32, i32, f32, vp, vp, vp]),
    "mmk_packed_weight_floats": (i64, [i32, i32]),
    "mmk_pack_weight_f32": (i32, [vp, i64, i32, i32, vp, vp]),
    "mmk_linear_f32": (i32, [vp, i64, i32, vp, vp, i32, i32, vp, i64, i32, vp]),
    "mmk_gemm_f32": (i32, [vp, i64, i64, vp, i32, i32, vp, i64, i64, i32, i32, vp]),
    "mmk_gemm_partial_floats": (i64, [i32, i32, i32, i32]),
    "mmk_gemm_bias_act_f32": (i32, [vp, i64, i32, vp, vp, i32, i32, vp, i64, i32, i32, i32, i64, i64, vp, i64, i32, vp]),
    "mmk_skinny_linear_f32": (i32, [vp, i64, i32, vp, vp, i32, i32, vp, i64, i32, vp]),
    "mmk_tr_attention_f32": (i32, [vp, i64, i64, vp, vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, i32, f32, i32, vp]),
    "mmk_tr_add_ln_f32": (i32, [vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, vp]),
    "mmk_categorical_sample_f32_i64": (i32, [vp, i64, i32, i32, i32, f32, vp, vp, vp, i64, vp]),
    "mmk_wavenet_plan_create": (i32, [C.POINTER(WaveNetConfig), C.POINTER(vp)]),
    "mmk_wavenet_plan_destroy": (None, [vp]),
    "mmk_wavenet_plan_bind": (i32, [vp, cp, vp, i64]),
    "mmk_wavenet_receptive_field": (i64, [vp]),
    "mmk_wavenet_workspace_bytes": (C.c_size_t, [vp]),
    "mmk_wavenet_commit": (i32, [vp, vp, C.c_size_t, vp]),
    "mmk_wavenet_warmup": (i32, [vp, i32, vp, i64, C.POINTER(vp), C.POINTER(i64), i64, i64, vp]),
    "mmk_wavenet_generate": (i32, [vp, i32, vp, i64, C.POINTER(vp), C.POINTER(i64), i64, i64, vp, vp, vp]),
    "mmk_wavenet_last_logits": (i32, [vp, i32, vp, i64, vp]),
    "mmk_wavenet_last_logits_of": (i32, [vp, i32, i32, vp, i64, vp]),
    "mmk_wavenet_profile_steps": (i32, [vp, i32, vp, i64, C.POINTER(vp), C.POINTER(i64), i64, i64,
                                        C.POINTER(C.c_double), C.POINTER(i64), vp]),
    "mmk_wavenet_mode": (i32, [vp]),
    "mmk_wavenet_pair_visits": (i32, [vp]),
    "mmk_wavenet_sync_status": (i32, [vp, vp]),
    "mmk_wavenet_inject_sync_error": (i32, [vp, vp]),
    "mmk_srnn_plan_create": (i32, [C.POINTER(SrnnConfig), C.POINTER(vp)]),
    "mmk_srnn_plan_destroy": (None, [vp]),
    "mmk_srnn_plan_bind": (i32, [vp, cp, vp, i64]),
    "mmk_srnn_workspace_bytes": (C.c_size_t, [vp]),
    "mmk_srnn_commit": (i32, [vp, vp, C.c_size_t, vp]),
    "mmk_srnn_reset": (i32, [vp, vp]),
    "mmk_srnn_warmup": (i32, [vp, i32, vp, i64, i64, vp]),
    "mmk_srnn_generate": (i32, [vp, i32, vp, i64, i64, i64, vp, vp, vp]),
    "mmk_srnn_last_logits": (i32, [vp, i32, vp, i64, vp]),
    "mmk_srnn_warmup_multi": (i32, [vp, i32, C.POINTER(vp), C.POINTER(i64), i64, vp]),
    "mmk_srnn_generate_multi": (i32, [vp, i32, C.POINTER(vp), C.POINTER(i64), i64, i64, vp, vp, vp]),
    "mmk_srnn_last_logits_of": (i32, [vp, i32, i32, vp, i64, vp]),
    "mmk_srnn_resident_blocks": (i64, [vp]),
    "mmk_srnn_resident_warmups": (i64, [vp]),
    "mmk_srnn_bottom_kernel": (i32, [vp]),
    "mmk_srnn_sync_status": (i32, [vp, vp]),
    "mmk_srnn_inject_sync_error": (i32, [vp, vp]),
    "mmk_s2s_plan_create": (i32, [C.POINTER(S2SConfig), C.POINTER(vp)]),
    "mmk_s2s_plan_destroy": (None, [vp]),
    "mmk_s2s_plan_bind": (i32, [vp, cp, vp, i64]),
    "mmk_s2s_workspace_bytes": (C.c_size_t, [vp]),
    "mmk_s2s_commit": (i32, [vp, vp, C.c_size_t, vp]),
    "mmk_s2s_step": (i32, [vp, i32, vp, i64, i64, vp, i64, i64, vp]),
    "mmk_s2s_generate": (i32, [vp, i32, vp, i64, i64, i64, i64, i64, vp]),
    "mmk_s2s_step_classes": (i32, [vp, i32, vp, i64, i64, vp, i64, i64, vp]),
    "mmk_s2s_generate_classes": (i32, [vp, i32, vp, i64, i64, i64, i64, i64, vp]),
    "mmk_s2s_last_logits": (i32, [vp, i32, vp, i64, vp]),
    "mmk_s2s_sync_status": (i32, [vp, vp]),
    "mmk_s2s_inject_sync_error": (i32, [vp, vp]),
    "mmk_s2s_resident_launches": (i64, [vp]),
    "mmk_tr_plan_create": (i32, [C.POINTER(TransformerConfig), C.POINTER(vp)]),
    "mmk_tr_plan_destroy": (None, [vp]),
    "mmk_tr_plan_bind": (i32, [vp, cp, vp, i64]),
    "mmk_tr_workspace_bytes": (C.c_size_t, [vp]),
    "mmk_tr_commit": (i32, [vp, vp, C.c_size_t, vp]),
    "mmk_tr_step": (i32, [vp, i32, vp, i64, i64, vp, i64, vp, vp, vp]),
    "mmk_tr_generate": (i32, [vp, i32, vp, i64, i64, i64, i64, vp, vp, vp]),
    "mmk_tr_last_logits": (i32, [vp, i32, vp, i64, vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# include/mmk_kmeans.h: the k-means entry points, a header and a table of their own beside include/mmk.h (the ABI version does not change)
_KMEANS_SIGNATURES = {
    "mmk_kmeans_assign_f32": (i32, [vp, i64, vp, i64, i32, vp, i64, vp, i32, vp, vp, vp, vp]),
    "mmk_kmeans_label_sums_workspace_bytes": (C.c_size_t, [i64, i32, i32]),
    "mmk_kmeans_label_sums_f64": (i32, [vp, i64, vp, i64, i32, vp, i32, vp, vp, vp, i64, vp, vp, vp, C.c_size_t, vp]),
    "mmk_kmeans_pp_step_workspace_bytes": (C.c_size_t, []),
    "mmk_kmeans_pp_step_f64": (i32, [vp, i64, vp, i64, i32, vp, i32, vp, vp, vp, vp, C.c_size_t, vp]),
}

KMEANS_SYMBOLS = tuple(_KMEANS_SIGNATURES)

# include/mmk_nn_filter.h: the nearest-neighbour filter's entry point, a header and a table of its own like the k-means ones
_NN_FILTER_SIGNATURES = {
    "mmk_nn_aggregate_f32": (i32, [vp, i64, i64, i32, vp, i32, i32, i32, vp, i64, vp, vp]),
}

NN_FILTER_SYMBOLS = tuple(_NN_FILTER_SIGNATURES)

# include/mmk_nmf.h: the NMF entry points, a header and a table of their own like the two above
_NMF_SIGNATURES = {
    "mmk_nmf_start_workspace_bytes": (C.c_size_t, [i64, i32, i32]),
    "mmk_nmf_start_f64": (i32, [vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_nmf_half_workspace_bytes": (C.c_size_t, [i64, i32, i32]),
    "mmk_nmf_w_half_f64": (i32, [vp, i64, i64, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_nmf_h_half_f64": (i32, [vp, i64, i64, i32, i32, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_nmf_solve_workspace_bytes": (C.c_size_t, [i64, i32, i32]),
    "mmk_nmf_solve_f64": (i32, [vp, i64, i64, i32, i32, vp, vp, i32, C.c_double, i32, i32, i32, vp, vp, C.c_size_t, vp]),
}

NMF_SYMBOLS = tuple(_NMF_SIGNATURES)

# include/mmk_samplify.h: the quadratic spline and the onset-cut entry points of Samplifyer, a header and a table of their own like the three above
_SAMPLIFY_SIGNATURES = {
    "mmk_spline2_coef_f64": (i32, [vp, i64, i32, i64, vp, i64, vp]),
    "mmk_spline2_eval_f32": (i32, [vp, i64, i32, i64, vp, i64, i64, vp]),
    "mmk_periods_workspace_bytes": (C.c_size_t, [i64]),
    "mmk_periods_count_i64": (i32, [vp, i64, vp, i64, vp, vp, C.c_size_t, vp]),
    "mmk_periods_fill_i64": (i32, [vp, i64, vp, i64, vp, C.c_size_t, i64, i64, vp, vp, vp, vp]),
    "mmk_samplify_scores_f32": (i32, [vp, i64, i64, vp, vp, i64, C.c_float, vp, vp, vp, vp, vp]),
    "mmk_samplify_cuts_i64": (i32, [vp, i64, vp, vp, vp, i32, vp, vp, i64, vp, vp, vp, vp]),
}

SAMPLIFY_SYMBOLS = tuple(_SAMPLIFY_SIGNATURES)

# include/mmk_spec_filter.h: the two harmonic spectrogram filters (AutoConvolve, F0Filter), a header and a table of their own like the four above
_SPEC_FILTER_SIGNATURES = {
    "mmk_auto_convolve_f32": (i32, [vp, i64, i64, i32, i32, i32, i32, vp, i64, i64, vp]),
    "mmk_f0_filter_f32": (i32, [vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp, i64, i64, vp]),
}

SPEC_FILTER_SYMBOLS = tuple(_SPEC_FILTER_SIGNATURES)

# include/mmk_factor_analysis.h: the EM entry and the transform matrix of FactorAnalysis, a header and a table of their own like the five above
_FACTOR_ANALYSIS_SIGNATURES = {
    "mmk_fa_fit_workspace_bytes": (C.c_size_t, [i32, i32]),
    "mmk_fa_fit_f64": (i32, [vp, i32, i32, i64, C.c_double, i32, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "mmk_fa_transform_matrix_workspace_bytes": (C.c_size_t, [i32, i32]),
    "mmk_fa_transform_matrix_f64": (i32, [vp, vp, i32, i32, vp, vp, C.c_size_t, vp]),
}

FACTOR_ANALYSIS_SYMBOLS = tuple(_FACTOR_ANALYSIS_SIGNATURES)

_lib = None


def load_library(path: Optional[str] = None):
    """dlopen the HIP library and type its entry points (no GPU needed for this)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise NativeError(
            f"{path} is missing: build it with `python -m mimikit_amd.build` (hipcc, --offload-arch=gfx950). "
            "There is no CPU fallback for the generate path.")
    lib = C.CDLL(path)
    for name, (res, args) in {**_SIGNATURES, **_KMEANS_SIGNATURES, **_NN_FILTER_SIGNATURES, **_NMF_SIGNATURES, **_SAMPLIFY_SIGNATURES,
                              **_SPEC_FILTER_SIGNATURES, **_FACTOR_ANALYSIS_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mmk_abi_version() != ABI_VERSION:
        raise NativeError(f"ABI version mismatch: library reports {lib.mmk_abi_version()}, binding expects {ABI_VERSION} "
                          "(a stale libmmk_hip.so: rebuild with `python -m mimikit_amd.build`)")
    if not DIAGNOSTIC or path != LIB_PATH:          # (the product library must be the one these sources make; a diagnostic build or a
        from .build import source_digest             #  variant is asked for by name through MMK_DIAG_LIB and is never found under the product's name)
        have, want = lib.mmk_build_digest().decode(), source_digest()
        if have != want:
            raise NativeError(f"{path} was built from other sources (digest {have}, the tree's is {want}): rebuild with "
                              "`python -m mimikit_amd.build`")
    for which, struct in enumerate((WaveNetConfig, SrnnConfig, S2SConfig, TransformerConfig)):
        if lib.mmk_config_bytes(which) != C.sizeof(struct):
            raise NativeError(f"{struct.__name__} is {C.sizeof(struct)} bytes here and {lib.mmk_config_bytes(which)} in the library "
                              "(a stale libmmk_hip.so: rebuild with `python -m mimikit_amd.build`)")
    _lib = lib
    return lib


def lib():
    return load_library()


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().mmk_last_error().decode("utf-8", "replace")
        kind = {-1: ValueError, -3: NotImplementedError, -6: KeyError}.get(rc, NativeError)
        raise kind(f"{what or 'libmmk_hip'} failed (code {rc}): {msg}")


def require_device(*tensors: torch.Tensor):
    """The hot path only runs on a HIP device; anything else is an error, never a fallback."""
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t)}")
        if t.device.type != "cuda":
            raise RuntimeError(
                f"mimikit_amd runs its generate path on the MI355X only: got a tensor on '{t.device}'. "
                "Move the network and its inputs to the HIP device ('cuda'); there is no CPU implementation "
                "in this package (the CPU restatement under oracle/ is test infrastructure).")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _workspace(n_bytes: int, device) -> torch.Tensor:
    """scratch for a ``*_workspace_bytes`` / ``*_workspace_floats`` entry point: at least ``n_bytes`` (never zero elements) of float64, which
    the allocator hands out aligned far beyond the 8 bytes any of them asks for; the size passed on stays the one the library returned"""
    return torch.empty((max((n_bytes + 7) // 8, 1),), dtype=torch.float64, device=device)


# ---------------------------------------------------------------------------
# feature functionals
# ---------------------------------------------------------------------------
def mulaw_compress(x: torch.Tensor, q_levels: int, compression: float, edges: torch.Tensor) -> torch.Tensor:
    require_device(x, edges)
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    out = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    check(lib().mmk_mulaw_compress_f32_i64(ptr(x), ptr(out), x.numel(), q_levels, compression, ptr(edges),
                                           stream_ptr(x.device)), "mmk_mulaw_compress_f32_i64")
    return out


def mulaw_expand(codes: torch.Tensor, q_levels: int, compression: float, table: torch.Tensor) -> torch.Tensor:
    require_device(codes, table)
    codes = codes.contiguous()
    if codes.dtype != torch.int64:
        codes = codes.long()
    out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    check(lib().mmk_mulaw_expand_i64_f32(ptr(codes), ptr(out), codes.numel(), q_levels, compression, ptr(table),
                                         stream_ptr(codes.device)), "mmk_mulaw_expand_i64_f32")
    return out


def resample(x: torch.Tensor, table: torch.Tensor, orig: int, new: int, width: int) -> torch.Tensor:
    """x: (..., n) fp32 -> (..., ceil(new * n / orig)); `table`: the (new, 2 * width + orig) polyphase filter bank"""
    require_device(x, table)
    if x.dtype != torch.float32:
        x = x.float()
    lead = x.shape[:-1]
    x2 = _rows(x)
    n_out = lib().mmk_resample_n_out(x2.shape[-1], orig, new)
    out = torch.empty((x2.shape[0], n_out), dtype=torch.float32, device=x.device)
    check(lib().mmk_resample_f32(ptr(x2), x2.stride(0), x2.shape[0], x2.shape[-1], ptr(table), orig, new, width, ptr(out), out.stride(0),
                                 stream_ptr(x.device)), "mmk_resample_f32")
    return out.reshape(*lead, n_out)


# include/mmk.h: MMK_LFILTER1_RUN / _WG / _CHUNK - samples per lane, lanes per workgroup and samples per workgroup of the filter and
# normalisation kernels (csrc/filters.hip); the tests place their lengths on these boundaries
LFILTER1_RUN = 16
LFILTER1_WG = 256
LFILTER1_CHUNK = LFILTER1_RUN * LFILTER1_WG
NORM_ORDERS = {float("inf"): 0, 1: 1, 2: 2}        # Normalize.p -> the `p` of mmk_row_normalize_f32


def _float32_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    """the argument checks of the row kernels, before the device is asked for: they fail the same way without one"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x)}")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} runs in float32 on the HIP path, got {x.dtype}")
    require_device(x)
    return _rows(x) if x.dim() else x.reshape(1, 1)


def lfilter1(x: torch.Tensor, b0: float, b1: float, a1: float) -> torch.Tensor:
    """x: (..., n) fp32 -> y of the same shape, y[n] = b0 x[n] + b1 x[n-1] - a1 y[n-1] along the last dimension from a zero state:
    torchaudio.functional.lfilter(x, [1, a1], [b0, b1], clamp=False)"""
    x2 = _float32_rows(x, "lfilter1")
    batch, n = x2.shape
    out = torch.empty((batch, n), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out.reshape(x.shape)
    work = _workspace(4 * lib().mmk_lfilter1_workspace_floats(batch, n), x.device) if a1 != 0 else None
    check(lib().mmk_lfilter1_f32(ptr(x2), x2.stride(0), batch, n, b0, b1, a1, ptr(out), out.stride(0), ptr(work), stream_ptr(x.device)),
          "mmk_lfilter1_f32")
    return out.reshape(x.shape)


def row_normalize(x: torch.Tensor, p: float, eps: float = 1e-12) -> torch.Tensor:
    """x: (..., n) fp32 -> x / max(||x||_p, eps) over the last dimension, p in {inf, 1, 2}: torch.nn.functional.normalize"""
    if p not in NORM_ORDERS:
        raise NotImplementedError(f"row_normalize: p={p} is not on the HIP path (inf, 1 or 2)")
    x2 = _float32_rows(x, "row_normalize")
    batch, n = x2.shape
    out = torch.empty((batch, n), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out.reshape(x.shape)
    work = _workspace(4 * lib().mmk_row_normalize_workspace_floats(batch, n), x.device)
    check(lib().mmk_row_normalize_f32(ptr(x2), x2.stride(0), batch, n, NORM_ORDERS[p], eps, ptr(out), out.stride(0), ptr(work),
                                      stream_ptr(x.device)), "mmk_row_normalize_f32")
    return out.reshape(x.shape)


# include/mmk.h: MMK_NNN_MAX_ROWS / _ROW_PAD / _LOOKAHEAD - prompt frames one wave aligns, the granule the cost rows of one corpus frame are
# padded to, and the anti-diagonals the DTW kernel loads its costs ahead (csrc/nnn.hip); the tests place their sizes on these
NNN_MAX_ROWS = 64
NNN_ROW_PAD = 16
NNN_LOOKAHEAD = 16


def nnn_n_pad(n: int) -> int:
    """floats between the costs of consecutive corpus frames in the cost tensor of ``cosine_cost``"""
    return (n + NNN_ROW_PAD - 1) // NNN_ROW_PAD * NNN_ROW_PAD


def _nnn_frames(x: torch.Tensor, dims: int, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x)}")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} runs in float32 on the HIP path, got {x.dtype}")
    if x.dim() != dims:
        raise ValueError(f"{what}: expected {dims} dimensions, got shape {tuple(x.shape)}")
    require_device(x)
    return x if x.stride(-1) == 1 or x.shape[-1] == 1 else x.contiguous()


def inv_row_norm(x: torch.Tensor) -> torch.Tensor:
    """x: (rows, k) or (batch, rows, k) fp32, bins contiguous, rows and clips at any stride -> 1 / |row|_2 per row, 0 for a row of norm 0"""
    x = _nnn_frames(x, 2 if isinstance(x, torch.Tensor) and x.dim() == 2 else 3, "inv_row_norm")
    x3 = x.unsqueeze(0) if x.dim() == 2 else x
    if x3.numel() == 0:
        raise ValueError(f"inv_row_norm: empty input {tuple(x.shape)}")
    out = torch.empty(x3.shape[:2], dtype=torch.float32, device=x.device)
    check(lib().mmk_inv_row_norm_f32(ptr(x3), x3.stride(0), x3.stride(1), x3.shape[0], x3.shape[1], x3.shape[2], ptr(out),
                                     stream_ptr(x.device)), "mmk_inv_row_norm_f32")
    return out.reshape(x.shape[:-1])


def cosine_cost(prompt_frames: torch.Tensor, corpus: torch.Tensor, corpus_inv_norm: torch.Tensor) -> torch.Tensor:
    """prompt_frames (B, N, k), corpus (M, k), corpus_inv_norm (M,) = inv_row_norm(corpus) -> cost (B, M, nnn_n_pad(N)):
    cost[b, j, i] = the cosine distance of |prompt row i of clip b| and |corpus row j|, clipped to [0, 2]; columns i >= N hold 1"""
    x = _nnn_frames(prompt_frames, 3, "cosine_cost")
    y = _nnn_frames(corpus, 2, "cosine_cost")
    require_device(corpus_inv_norm)
    batch, n, k = x.shape
    m = y.shape[0]
    if y.shape[1] != k:
        raise ValueError(f"cosine_cost: the prompt has {k} bins, the corpus {y.shape[1]}")
    if corpus_inv_norm.shape != (m,) or corpus_inv_norm.dtype != torch.float32 or not corpus_inv_norm.is_contiguous():
        raise ValueError(f"cosine_cost: corpus_inv_norm must be {m} contiguous float32 values, got {tuple(corpus_inv_norm.shape)} {corpus_inv_norm.dtype}")
    if n > NNN_MAX_ROWS:
        raise NotImplementedError(f"cosine_cost: N = {n} prompt frames, the limit is {NNN_MAX_ROWS}")
    if min(batch, n, m, k) < 1:
        raise ValueError(f"cosine_cost: empty input (batch={batch}, N={n}, M={m}, bins={k})")
    rx = inv_row_norm(x)
    cost = torch.empty((batch, m, nnn_n_pad(n)), dtype=torch.float32, device=x.device)
    check(lib().mmk_cosine_cost_f32(ptr(x), x.stride(0), x.stride(1), ptr(rx), batch, n, ptr(y), y.stride(0), ptr(corpus_inv_norm), m, k,
                                    ptr(cost), stream_ptr(x.device)), "mmk_cosine_cost_f32")
    return cost


def dtw_subseq(cost: torch.Tensor, n: int, last_row: bool = False):
    """cost: (B, M, nnn_n_pad(n)) as cosine_cost leaves it -> (end (B,) int64, dist (B,) fp32[, D[n-1, :] (B, M) fp32]) of the subsequence DTW"""
    cost = _nnn_frames(cost, 3, "dtw_subseq")
    if n > NNN_MAX_ROWS:
        raise NotImplementedError(f"dtw_subseq: N = {n} prompt frames, the limit is {NNN_MAX_ROWS}")
    if n < 1 or cost.shape[2] != nnn_n_pad(n) or not cost.is_contiguous():
        raise ValueError(f"dtw_subseq: a contiguous cost tensor (B, M, {nnn_n_pad(max(n, 1))}) is expected for N = {n}, got {tuple(cost.shape)}")
    batch, m = cost.shape[:2]
    end = torch.empty((batch,), dtype=torch.int64, device=cost.device)
    dist = torch.empty((batch,), dtype=torch.float32, device=cost.device)
    row = torch.empty((batch, m), dtype=torch.float32, device=cost.device) if last_row else None
    check(lib().mmk_dtw_subseq_f32(ptr(cost), batch, n, m, ptr(end), ptr(dist), ptr(row), stream_ptr(cost.device)), "mmk_dtw_subseq_f32")
    return (end, dist, row) if last_row else (end, dist)


def nnn_end_columns(prompt_frames: torch.Tensor, corpus: torch.Tensor, corpus_inv_norm: torch.Tensor):
    """the column where the best subsequence-DTW alignment of each clip's (N, k) prompt frames against the (M, k) corpus ends, and its
    accumulated cosine distance: (end (B,) int64, dist (B,) fp32), on torch's current stream, without a host round trip
    (NearestNextNeighbor.predict_start_frame of the reference = end + 1)"""
    cost = cosine_cost(prompt_frames, corpus, corpus_inv_norm)
    return dtw_subseq(cost, prompt_frames.shape[1])


# include/mmk.h: MMK_NN_SPAN / MMK_CUM_ENTROPY_MAX_T - corpus frames of one workgroup of the search kernel (csrc/nn_search.h) and the longest row the
# entropy kernel ranks (csrc/neighbors.hip); the tests place their sizes on these
NN_SPAN = 2048
CUM_ENTROPY_MAX_T = 32768


def nn_cosine(x: torch.Tensor, corpus: torch.Tensor, corpus_inv_norm: torch.Tensor):
    """x (rows, k), corpus (M, k), corpus_inv_norm (M,) = inv_row_norm(corpus) -> (index (rows,) int64, cos_best (rows,) fp32): per row of x the
    first corpus frame of the largest cosine similarity and that cosine, clamped to [-1, 1].  The (rows, M) matrix is never formed: the
    workspace is 8 bytes per row and span of NN_SPAN corpus frames"""
    x = _nnn_frames(x, 2, "nn_cosine")
    y = _nnn_frames(corpus, 2, "nn_cosine")
    require_device(corpus_inv_norm)
    rows, k = x.shape
    m = y.shape[0]
    if y.shape[1] != k:
        raise ValueError(f"nn_cosine: the queries have {k} bins, the corpus {y.shape[1]}")
    if corpus_inv_norm.shape != (m,) or corpus_inv_norm.dtype != torch.float32 or not corpus_inv_norm.is_contiguous():
        raise ValueError(f"nn_cosine: corpus_inv_norm must be {m} contiguous float32 values, got {tuple(corpus_inv_norm.shape)} {corpus_inv_norm.dtype}")
    if min(rows, m, k) < 1:
        raise ValueError(f"nn_cosine: empty input (rows={rows}, M={m}, bins={k})")
    rx = inv_row_norm(x)
    index = torch.empty((rows,), dtype=torch.int64, device=x.device)
    best = torch.empty((rows,), dtype=torch.float32, device=x.device)
    n_work = lib().mmk_nn_cosine_workspace_bytes(rows, m)
    work = _workspace(n_work, x.device)
    check(lib().mmk_nn_cosine_f32(ptr(x), x.stride(0), ptr(rx), rows, ptr(y), y.stride(0), ptr(corpus_inv_norm), m, k, ptr(index), ptr(best),
                                  ptr(work), n_work, stream_ptr(x.device)), "mmk_nn_cosine_f32")
    return index, best


def cum_entropy(items: torch.Tensor, per_step: bool = False):
    """items (B, T) int64 -> total (B,) fp32, the sum over s of the entropy e[s] of the histogram of items[b, :s + 1]; with ``per_step`` also
    e (B, T) fp32"""
    if not isinstance(items, torch.Tensor):
        raise TypeError(f"cum_entropy: expected a torch.Tensor, got {type(items)}")
    if items.dtype != torch.int64:
        raise TypeError(f"cum_entropy takes int64 items (indices of neighbours), got {items.dtype}")
    if items.dim() != 2:
        raise ValueError(f"cum_entropy: expected (B, T) items, got shape {tuple(items.shape)}")
    batch, t = items.shape
    if batch < 1 or t < 1:
        raise ValueError(f"cum_entropy: empty input {tuple(items.shape)}")
    if t > CUM_ENTROPY_MAX_T:
        raise NotImplementedError(f"cum_entropy: T = {t} items per row, the limit is {CUM_ENTROPY_MAX_T}")
    require_device(items)
    if items.stride(1) != 1 and t > 1:
        items = items.contiguous()
    total = torch.empty((batch,), dtype=torch.float32, device=items.device)
    e = torch.empty((batch, t), dtype=torch.float32, device=items.device) if per_step else None
    check(lib().mmk_cum_entropy_i64(ptr(items), items.stride(0), batch, t, ptr(total), ptr(e), t if per_step else 0, stream_ptr(items.device)),
          "mmk_cum_entropy_i64")
    return (total, e) if per_step else total


def nn_cosine_self(x: torch.Tensor, inv_norm: Optional[torch.Tensor] = None):
    """x (rows >= 2, k), inv_norm (rows,) = inv_row_norm(x) (computed here if not given) -> (index (rows,) int64, cos_best (rows,) fp32): per
    row the first OTHER row of x of the largest cosine similarity and that cosine.  The (rows, rows) matrix is never formed"""
    x = _nnn_frames(x, 2, "nn_cosine_self")
    rows, k = x.shape
    if rows < 2 or k < 1:
        raise ValueError(f"nn_cosine_self: at least two frames of at least one bin, got {tuple(x.shape)}")
    rx = inv_row_norm(x) if inv_norm is None else inv_norm
    require_device(rx)
    if rx.shape != (rows,) or rx.dtype != torch.float32 or not rx.is_contiguous():
        raise ValueError(f"nn_cosine_self: inv_norm must be {rows} contiguous float32 values, got {tuple(rx.shape)} {rx.dtype}")
    index = torch.empty((rows,), dtype=torch.int64, device=x.device)
    best = torch.empty((rows,), dtype=torch.float32, device=x.device)
    n_work = lib().mmk_nn_cosine_workspace_bytes(rows, rows)
    work = _workspace(n_work, x.device)
    check(lib().mmk_nn_cosine_self_f32(ptr(x), x.stride(0), ptr(rx), rows, k, ptr(index), ptr(best), ptr(work), n_work, stream_ptr(x.device)),
          "mmk_nn_cosine_self_f32")
    return index, best


def nn_components(nearest: torch.Tensor):
    """nearest (n,) int64 with entries in [0, n) -> (labels (n,) int64, n_components () int64, on the device): the weakly connected components
    of the graph i -> nearest[i], numbered by rising smallest member"""
    if not isinstance(nearest, torch.Tensor):
        raise TypeError(f"nn_components: expected a torch.Tensor, got {type(nearest)}")
    if nearest.dtype != torch.int64:
        raise TypeError(f"nn_components takes int64 indices, got {nearest.dtype}")
    if nearest.dim() != 1 or nearest.shape[0] < 1:
        raise ValueError(f"nn_components: expected (n >= 1,) indices, got shape {tuple(nearest.shape)}")
    require_device(nearest)
    nearest = nearest.contiguous()
    n = nearest.shape[0]
    labels = torch.empty((n,), dtype=torch.int64, device=nearest.device)
    count = torch.empty((), dtype=torch.int64, device=nearest.device)
    n_work = lib().mmk_nn_components_workspace_bytes(n)
    work = _workspace(n_work, nearest.device)
    check(lib().mmk_nn_components_i64(ptr(nearest), n, ptr(labels), ptr(count), ptr(work), n_work, stream_ptr(nearest.device)),
          "mmk_nn_components_i64")
    return labels, count


def segment_mean(x: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """x (n, k) fp32, order (n,) int64 row numbers, offsets (S + 1,) int64 rising positions in `order` -> (S, k) fp32: row s is the mean of the
    rows x[order[offsets[s] : offsets[s + 1]]], added in that order in fp64 and rounded once"""
    x = _nnn_frames(x, 2, "segment_mean")
    n, k = x.shape
    for name, t in (("order", order), ("offsets", offsets)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise TypeError(f"segment_mean: {name} must be a 1-D int64 tensor")
    require_device(order, offsets)
    n_segments = offsets.shape[0] - 1
    if n < 1 or k < 1 or order.shape[0] != n or n_segments < 1 or n_segments > n:
        raise ValueError(f"segment_mean: x {tuple(x.shape)}, order {tuple(order.shape)}, {n_segments} segments")
    order, offsets = order.contiguous(), offsets.contiguous()
    out = torch.empty((n_segments, k), dtype=torch.float32, device=x.device)
    check(lib().mmk_segment_mean_f32(ptr(x), x.stride(0), n, k, ptr(order), ptr(offsets), n_segments, ptr(out), out.stride(0),
                                     stream_ptr(x.device)), "mmk_segment_mean_f32")
    return out


# include/mmk.h: MMK_NN_TOPK_MAX - the neighbours per row a lane of the search kernel keeps in registers (csrc/nn_search.h)
NN_TOPK_MAX = 16
NN_TOPK_METRICS = ("euclidean", "cosine")


def nn_topk(x: torch.Tensor, y: torch.Tensor, t: int, metric: str = "euclidean", self_exclude: bool = False):
    """x (rows, k), y (M, k), 1 <= t <= NN_TOPK_MAX -> (index (rows, t) int64, key (rows, t) fp32): per row of x the t nearest rows of y
    under `metric`, nearest first, equal keys by rising index; slots past the last candidate hold -1 / -inf.  key is the cosine similarity
    ("cosine": clamped to [-1, 1], with t = 1 exactly nn_cosine / nn_cosine_self) or <x, y> - |y|^2 / 2 ("euclidean": the largest key is the smallest distance; |x - y|^2 = |x|^2 - 2 key).  With
    ``self_exclude`` y must be x itself and row r is left out of its own list.  The (rows, M) matrix is never formed: the workspace is
    8 t bytes per row and span of NN_SPAN rows of y, allocated in one piece - this wrapper does not walk the rows in blocks (268 MB at
    rows = M = 65536, t = 16)"""
    same = y is x
    x = _nnn_frames(x, 2, "nn_topk")
    y = x if self_exclude and same else _nnn_frames(y, 2, "nn_topk")
    if metric not in NN_TOPK_METRICS:
        raise NotImplementedError(f"nn_topk: metric={metric!r} is not on the HIP path ({', '.join(NN_TOPK_METRICS)})")
    rows, k = x.shape
    m = y.shape[0]
    if y.shape[1] != k:
        raise ValueError(f"nn_topk: the queries have {k} bins, the corpus {y.shape[1]}")
    if min(rows, m, k) < 1:
        raise ValueError(f"nn_topk: empty input (rows={rows}, M={m}, bins={k})")
    t = int(t)
    if t < 1:
        raise ValueError(f"nn_topk: t = {t} < 1")
    if t > NN_TOPK_MAX:
        raise NotImplementedError(f"nn_topk: t = {t} neighbours per row, the limit is {NN_TOPK_MAX} (NN_TOPK_MAX)")
    if self_exclude and (y.data_ptr() != x.data_ptr() or y.shape != x.shape or y.stride() != x.stride()):
        raise ValueError("nn_topk: self_exclude takes y = x, the same rows")
    dev = x.device
    if metric == "cosine":
        qscale = inv_row_norm(x)
        cscale = qscale if self_exclude else inv_row_norm(y)
        cshift = torch.zeros((m,), dtype=torch.float32, device=dev)
        lo, hi = -1.0, 1.0
    else:
        lo, hi = float("-inf"), float("inf")
        qscale = torch.ones((max(rows, m),), dtype=torch.float32, device=dev)
        cscale = qscale
        cshift = torch.empty((m,), dtype=torch.float32, device=dev)
        check(lib().mmk_half_neg_sqnorm_f32(ptr(y), y.stride(0), m, k, ptr(cshift), stream_ptr(dev)), "mmk_half_neg_sqnorm_f32")
    index = torch.empty((rows, t), dtype=torch.int64, device=dev)
    key = torch.empty((rows, t), dtype=torch.float32, device=dev)
    n_work = lib().mmk_nn_topk_workspace_bytes(rows, m, t)
    work = _workspace(n_work, dev)
    check(lib().mmk_nn_topk_f32(ptr(x), x.stride(0), ptr(qscale), rows, ptr(y), y.stride(0), ptr(cscale), ptr(cshift), lo, hi, m, k, t,
                                1 if self_exclude else 0, ptr(index), ptr(key), ptr(work), n_work, stream_ptr(dev)), "mmk_nn_topk_f32")
    return index, key


def edge_components(src: torch.Tensor, dst: torch.Tensor, n: int):
    """src, dst (n_edges,) int64 with entries in [0, n) -> (labels (n,) int64, n_components () int64, on the device): the connected
    components of the undirected graph of those edges over n nodes, numbered by rising smallest member.  The call waits for the stream
    once per four rounds of hooking (it reads a changed-flag back)"""
    for name, e in (("src", src), ("dst", dst)):
        if not isinstance(e, torch.Tensor):
            raise TypeError(f"edge_components: expected a torch.Tensor for {name}, got {type(e)}")
        if e.dtype != torch.int64:
            raise TypeError(f"edge_components takes int64 indices, {name} is {e.dtype}")
        if e.dim() != 1:
            raise ValueError(f"edge_components: expected (n_edges,) indices, {name} has shape {tuple(e.shape)}")
    n = int(n)
    if src.shape != dst.shape or n < 1:
        raise ValueError(f"edge_components: src {tuple(src.shape)}, dst {tuple(dst.shape)}, n = {n}")
    require_device(src, dst)
    src, dst = src.contiguous(), dst.contiguous()
    labels = torch.empty((n,), dtype=torch.int64, device=src.device)
    count = torch.empty((), dtype=torch.int64, device=src.device)
    n_work = lib().mmk_edge_components_workspace_bytes(n)
    work = _workspace(n_work, src.device)
    n_edges = src.shape[0]
    check(lib().mmk_edge_components_i64(ptr(src) if n_edges else None, ptr(dst) if n_edges else None, n_edges, n, ptr(labels), ptr(count),
                                        ptr(work), n_work, stream_ptr(src.device)), "mmk_edge_components_i64")
    return labels, count


# include/mmk_nn_filter.h: MMK_NN_AGG_* in the order of their codes
NN_AGGREGATES = ("median", "mean", "max", "min")


def nn_aggregate(x: torch.Tensor, index: torch.Tensor, op: str = "median", mutual: bool = True, return_count: bool = False):
    """x (n, k) fp32, index (n, t <= NN_TOPK_MAX) int64 as nn_topk returns it -> (n, k) fp32: every row replaced by the `op` (NN_AGGREGATES)
    of the rows its list names, bin by bin; a slot outside [0, n) (nn_topk's -1) or equal to its own row number is empty, and a row
    without a neighbour keeps its values.  With ``mutual`` row j counts for row i only if row j's list holds i.  median / max / min
    return numpy's bits on float32 (an even count: fl32(fl32(a + b) / 2)), mean is the float64 sum in slot order rounded once.
    ``return_count``: also the (n,) int32 number of neighbours of every row.  One launch; nothing of size n x t x k is allocated"""
    x = _nnn_frames(x, 2, "nn_aggregate")
    if not isinstance(index, torch.Tensor):
        raise TypeError(f"nn_aggregate: expected a torch.Tensor for index, got {type(index)}")
    if index.dtype != torch.int64:
        raise TypeError(f"nn_aggregate takes the int64 index of nn_topk, got {index.dtype}")
    if index.dim() != 2:
        raise ValueError(f"nn_aggregate: expected an (n, t) index, got shape {tuple(index.shape)}")
    require_device(index)
    if op not in NN_AGGREGATES:
        raise ValueError(f"nn_aggregate: op={op!r} is none of {', '.join(NN_AGGREGATES)}")
    n, k = x.shape
    t = index.shape[1]
    if min(n, k) < 1 or index.shape[0] != n:
        raise ValueError(f"nn_aggregate: x {tuple(x.shape)}, index {tuple(index.shape)}")
    if t < 1:
        raise ValueError(f"nn_aggregate: t = {t} < 1")
    if t > NN_TOPK_MAX:
        raise NotImplementedError(f"nn_aggregate: t = {t} neighbours per row, the limit is {NN_TOPK_MAX} (NN_TOPK_MAX)")
    index = index.contiguous()
    out = torch.empty((n, k), dtype=torch.float32, device=x.device)
    count = torch.empty((n,), dtype=torch.int32, device=x.device) if return_count else None
    check(lib().mmk_nn_aggregate_f32(ptr(x), x.stride(0), n, k, ptr(index), t, 1 if mutual else 0, NN_AGGREGATES.index(op), ptr(out), out.stride(0),
                                     ptr(count), stream_ptr(x.device)), "mmk_nn_aggregate_f32")
    return (out, count) if return_count else out


# include/mmk_spec_filter.h: MMK_SPEC_FILTER_* / MMK_AUTO_CONVOLVE_* / MMK_F0_FILTER_* - the bins of a frame a workgroup keeps in LDS beside
# their float64 weights, the frames a workgroup takes in turn, the longest product window and the harmonic counts
SPEC_FILTER_MAX_BINS = 4097
SPEC_FILTER_TILE_FRAMES = 4
AUTO_CONVOLVE_MAX_WINDOW = 64
F0_FILTER_MAX_OVERTONE = 16
F0_FILTER_MAX_UNDERTONE = 16


def _spec_filter_input(s, who: str) -> torch.Tensor:
    """the checks the two filters share, made on the host before a device is asked for -> (B, T, F) with bins contiguous"""
    if not isinstance(s, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor, got {type(s)}")
    if s.dtype != torch.float32:
        raise TypeError(f"{who} runs in float32 on the HIP path, got {s.dtype}")
    if s.dim() not in (2, 3):
        raise ValueError(f"{who} takes (T, F) or (B, T, F), got shape {tuple(s.shape)}")
    if min(s.shape) < 1 or s.shape[-1] < 2:
        raise ValueError(f"{who}: at least one frame of at least 2 bins, got shape {tuple(s.shape)}")
    if s.shape[-1] > SPEC_FILTER_MAX_BINS:
        raise NotImplementedError(f"{who}: {s.shape[-1]} bins, the limit of the HIP path is {SPEC_FILTER_MAX_BINS} (native.SPEC_FILTER_MAX_BINS)")
    require_device(s)
    s3 = s if s.dim() == 3 else s.unsqueeze(0)
    if s3.stride(2) != 1 or s3.stride(1) < 0 or s3.stride(0) < 0:
        s3 = s3.contiguous()
    return s3


def auto_convolve(s: torch.Tensor, window_size: int = 3) -> torch.Tensor:
    """s: (T, F) or (B, T, F) non-negative fp32 magnitudes, rows and clips at any stride -> fp32 of s's shape: the reference's AutoConvolve
    (``mmk_auto_convolve_f32``, one launch on the current stream, no synchronisation, no workspace): per bin the float64 product over the
    frames t - k // 2 ... t - k // 2 + k - 1 of the clip (1 outside it), log(1.0 + p), normalised over the frame, times s.
    ``window_size`` < 2 raises ValueError (the reference's own slice is empty at 1), above AUTO_CONVOLVE_MAX_WINDOW NotImplementedError."""
    k = int(window_size)
    if k < 2:
        raise ValueError(f"auto_convolve: window_size = {k}, at least 2 is needed")
    if k > AUTO_CONVOLVE_MAX_WINDOW:
        raise NotImplementedError(f"auto_convolve: window_size = {k}, the limit of the HIP path is {AUTO_CONVOLVE_MAX_WINDOW} "
                                  "(native.AUTO_CONVOLVE_MAX_WINDOW)")
    s3 = _spec_filter_input(s, "auto_convolve")
    batch, frames, bins = s3.shape
    out = torch.empty((batch, frames, bins), dtype=torch.float32, device=s.device)
    check(lib().mmk_auto_convolve_f32(ptr(s3), s3.stride(0), s3.stride(1), batch, frames, bins, k, ptr(out), frames * bins, bins,
                                      stream_ptr(s.device)), "mmk_auto_convolve_f32")
    return out.reshape(s.shape)


def f0_filter(s: torch.Tensor, n_overtone: int = 4, n_undertone: int = 4, soft: bool = True, normalize: bool = True) -> torch.Tensor:
    """s: (T, F) or (B, T, F) non-negative fp32 magnitudes, rows and clips at any stride -> fp32 of s's shape: the reference's F0Filter on a
    uniform frequency grid (``mmk_f0_filter_f32``, one launch on the current stream, no synchronisation, no workspace): per bin the float64
    sum of the overtones z[h b], h < n_overtone, minus the interpolated undertones at b / x, 2 <= x < n_undertone; the positive part (or
    its indicator without ``soft``), normalised over the frame with ``normalize``, times s.  Counts above F0_FILTER_MAX_OVERTONE /
    F0_FILTER_MAX_UNDERTONE raise NotImplementedError, negative ones ValueError."""
    n_over, n_under = int(n_overtone), int(n_undertone)
    if n_over < 0 or n_under < 0:
        raise ValueError(f"f0_filter: n_overtone = {n_over}, n_undertone = {n_under}: neither may be negative")
    if n_over > F0_FILTER_MAX_OVERTONE or n_under > F0_FILTER_MAX_UNDERTONE:
        raise NotImplementedError(f"f0_filter: n_overtone = {n_over}, n_undertone = {n_under}, the limits of the HIP path are "
                                  f"{F0_FILTER_MAX_OVERTONE} (native.F0_FILTER_MAX_OVERTONE) and {F0_FILTER_MAX_UNDERTONE} "
                                  "(native.F0_FILTER_MAX_UNDERTONE)")
    s3 = _spec_filter_input(s, "f0_filter")
    batch, frames, bins = s3.shape
    out = torch.empty((batch, frames, bins), dtype=torch.float32, device=s.device)
    check(lib().mmk_f0_filter_f32(ptr(s3), s3.stride(0), s3.stride(1), batch, frames, bins, n_over, n_under, 1 if soft else 0,
                                  1 if normalize else 0, ptr(out), frames * bins, bins, stream_ptr(s.device)), "mmk_f0_filter_f32")
    return out.reshape(s.shape)


# include/mmk_kmeans.h: MMK_KMEANS_* - the centres of one assignment (the widest centre tile of csrc/kmeans.hip), the candidates of one
# seeding step, the slabs of the float64 sums
KMEANS_MAX_K = 256
KMEANS_PP_MAX_TRIALS = 8
KMEANS_MAX_SLABS = 1024


def _kmeans_offset(offset: Optional[torch.Tensor], d: int, what: str) -> Optional[torch.Tensor]:
    if offset is None:
        return None
    if not isinstance(offset, torch.Tensor) or offset.dtype != torch.float32 or tuple(offset.shape) != (d,):
        raise TypeError(f"{what}: offset must be a float32 tensor of shape ({d},)")
    require_device(offset)
    return offset.contiguous()


def kmeans_assign(x: torch.Tensor, offset: Optional[torch.Tensor], centres: torch.Tensor, labels: torch.Tensor, changed: Optional[torch.Tensor] = None,
                  key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (N, D) fp32, offset (D,) fp32 or None, centres (K <= KMEANS_MAX_K, D) fp32 in the coordinates of x' = fl32(x - offset), labels (N,)
    int32 IN/OUT -> labels: the first centre with the largest <x'_r, c_j> - |c_j|^2 / 2, the nearest one.  ``changed`` (() int64) is
    incremented for every row whose label differs from the one found in ``labels``; ``key`` (N,) fp32 receives the largest key.  One
    launch behind mmk_half_neg_sqnorm_f32 of the centres; nothing of size N x K is allocated"""
    x = _nnn_frames(x, 2, "kmeans_assign")
    centres = _nnn_frames(centres, 2, "kmeans_assign")
    n, d = x.shape
    k = centres.shape[0]
    if min(n, d, k) < 1 or centres.shape[1] != d:
        raise ValueError(f"kmeans_assign: x {tuple(x.shape)}, centres {tuple(centres.shape)}")
    if k > KMEANS_MAX_K:
        raise NotImplementedError(f"kmeans_assign: {k} centres, the limit of the HIP path is {KMEANS_MAX_K} (native.KMEANS_MAX_K)")
    offset = _kmeans_offset(offset, d, "kmeans_assign")
    for name, t, dtype, shape in (("labels", labels, torch.int32, (n,)), ("changed", changed, torch.int64, ()), ("key", key, torch.float32, (n,))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise TypeError(f"kmeans_assign: {name} must be a contiguous {dtype} tensor of shape {shape}")
    require_device(labels, changed, key)
    dev = x.device
    shift = torch.empty((k,), dtype=torch.float32, device=dev)
    check(lib().mmk_half_neg_sqnorm_f32(ptr(centres), centres.stride(0), k, d, ptr(shift), stream_ptr(dev)), "mmk_half_neg_sqnorm_f32")
    check(lib().mmk_kmeans_assign_f32(ptr(x), x.stride(0), ptr(offset), n, d, ptr(centres), centres.stride(0), ptr(shift), k, ptr(labels), ptr(key),
                                      ptr(changed), stream_ptr(dev)), "mmk_kmeans_assign_f32")
    return labels


def kmeans_label_sums(x: torch.Tensor, offset: Optional[torch.Tensor], labels: torch.Tensor, k: int, centres: Optional[torch.Tensor] = None,
                      row_d2: bool = False):
    """x (N, D) fp32, labels (N,) int32 in [0, k) -> (sums (k, D) fp64, counts (k,) int64): the float64 sum of x' = fl32(x - offset) over every
    label's rows, in one fixed order, the rows read once and in order.  With ``centres`` (k, D) fp32 also (inertia () fp64, row_d2 (N,) fp64 or
    None): |x'_r - c_label_r|^2 computed directly in float64, and their sum"""
    x = _nnn_frames(x, 2, "kmeans_label_sums")
    n, d = x.shape
    k = int(k)
    if min(n, d, k) < 1:
        raise ValueError(f"kmeans_label_sums: x {tuple(x.shape)}, k = {k}")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise TypeError(f"kmeans_label_sums: labels must be a contiguous int32 tensor of shape ({n},)")
    require_device(labels)
    offset = _kmeans_offset(offset, d, "kmeans_label_sums")
    dev = x.device
    sums = torch.empty((k, d), dtype=torch.float64, device=dev)
    counts = torch.empty((k,), dtype=torch.int64, device=dev)
    inertia = d2 = None
    c_stride = 0
    if centres is not None:
        centres = _nnn_frames(centres, 2, "kmeans_label_sums")
        if tuple(centres.shape) != (k, d):
            raise ValueError(f"kmeans_label_sums: centres {tuple(centres.shape)}, expected {(k, d)}")
        c_stride = centres.stride(0)
        inertia = torch.empty((), dtype=torch.float64, device=dev)
        d2 = torch.empty((n,), dtype=torch.float64, device=dev) if row_d2 else None
    n_work = lib().mmk_kmeans_label_sums_workspace_bytes(n, d, k)
    work = _workspace(n_work, dev)
    check(lib().mmk_kmeans_label_sums_f64(ptr(x), x.stride(0), ptr(offset), n, d, ptr(labels), k, ptr(sums), ptr(counts), ptr(centres), c_stride,
                                          ptr(d2), ptr(inertia), ptr(work), n_work, stream_ptr(dev)), "mmk_kmeans_label_sums_f64")
    return (sums, counts) if centres is None else (sums, counts, inertia, d2)


def kmeans_pp_step(x: torch.Tensor, offset: Optional[torch.Tensor], cand: torch.Tensor, closest: torch.Tensor, pot: torch.Tensor,
                   chosen: torch.Tensor, work: Optional[torch.Tensor] = None):
    """one step of k-means++ seeding: cand (t <= KMEANS_PP_MAX_TRIALS,) int64 candidate rows, closest (N,) fp64 IN/OUT, pot () fp64 and chosen
    () int64 OUT - the first candidate whose min(closest, |x' - x'_cand|^2) has the smallest sum.  Nothing is read back"""
    x = _nnn_frames(x, 2, "kmeans_pp_step")
    n, d = x.shape
    offset = _kmeans_offset(offset, d, "kmeans_pp_step")
    for name, t, dtype, shape in (("cand", cand, torch.int64, None), ("closest", closest, torch.float64, (n,)), ("pot", pot, torch.float64, ()),
                                  ("chosen", chosen, torch.int64, ())):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != shape) or t.dim() > 1 or not t.is_contiguous():
            raise TypeError(f"kmeans_pp_step: {name} must be a contiguous {dtype} tensor" + (f" of shape {shape}" if shape is not None else ""))
    require_device(cand, closest, pot, chosen)
    t = cand.shape[0]
    if t < 1:
        raise ValueError("kmeans_pp_step: no candidate")
    if t > KMEANS_PP_MAX_TRIALS:
        raise NotImplementedError(f"kmeans_pp_step: {t} candidates, the limit is {KMEANS_PP_MAX_TRIALS} (native.KMEANS_PP_MAX_TRIALS)")
    n_work = lib().mmk_kmeans_pp_step_workspace_bytes()
    if work is None:
        work = _workspace(n_work, x.device)
    check(lib().mmk_kmeans_pp_step_f64(ptr(x), x.stride(0), ptr(offset), n, d, ptr(cand), t, ptr(closest), ptr(pot), ptr(chosen), ptr(work),
                                       work.numel() * 8, stream_ptr(x.device)), "mmk_kmeans_pp_step_f64")
    return chosen


# include/mmk.h: MMK_PCA_* - the widest frames and the most components of the PCA kernels (csrc/pca.hip), the stop rule of the eigen step
PCA_MAX_D = 4096
PCA_MAX_COMPONENTS = 64
PCA_MAX_ITER = 4000
PCA_TOL = 1e-12


def _pca_limits(d: int, n_components: int, what: str):
    if d > PCA_MAX_D:
        raise NotImplementedError(f"{what}: D = {d} bins, the limit of the HIP path is {PCA_MAX_D} (native.PCA_MAX_D)")
    if n_components > PCA_MAX_COMPONENTS:
        raise NotImplementedError(f"{what}: n_components = {n_components}, the limit of the HIP path is {PCA_MAX_COMPONENTS} "
                                  "(native.PCA_MAX_COMPONENTS)")


def _f64_vector(t: torch.Tensor, shape, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise TypeError(f"{what} must be a float64 tensor of shape {tuple(shape)}")
    require_device(t)
    return t.contiguous()


def pca_colstats(x: torch.Tensor):
    """x (N, D) fp32 -> (mean (D,), scale (D,)) fp64 on the device: sklearn's StandardScaler statistics (population standard deviation, 1 for
    a constant column) with the mean that sklearn's PCA subtracts afterwards folded into `mean`"""
    x = _nnn_frames(x, 2, "pca_colstats")
    n, d = x.shape
    if n < 1 or d < 1:
        raise ValueError(f"pca_colstats: empty input {tuple(x.shape)}")
    _pca_limits(d, 1, "pca_colstats")
    mean = torch.empty((d,), dtype=torch.float64, device=x.device)
    scale = torch.empty((d,), dtype=torch.float64, device=x.device)
    n_work = lib().mmk_pca_colstats_workspace_bytes(n, d)
    work = _workspace(n_work, x.device)
    check(lib().mmk_pca_colstats_f64(ptr(x), x.stride(0), n, d, ptr(mean), ptr(scale), ptr(work), n_work, stream_ptr(x.device)),
          "mmk_pca_colstats_f64")
    return mean, scale


def pca_cov(x: torch.Tensor, mean: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x (N >= 2, D) fp32, mean and scale (D,) fp64 -> C (D, D) fp64 = Z^T Z / (N - 1), Z = (x - mean) / scale; Z is never written"""
    x = _nnn_frames(x, 2, "pca_cov")
    n, d = x.shape
    if n < 2 or d < 1:
        raise ValueError(f"pca_cov: x must be (N >= 2, D >= 1), got {tuple(x.shape)}")
    _pca_limits(d, 1, "pca_cov")
    mean, scale = _f64_vector(mean, (d,), "pca_cov: mean"), _f64_vector(scale, (d,), "pca_cov: scale")
    c = torch.empty((d, d), dtype=torch.float64, device=x.device)
    n_work = lib().mmk_pca_cov_workspace_bytes(n, d)
    work = _workspace(n_work, x.device)
    check(lib().mmk_pca_cov_f64(ptr(x), x.stride(0), n, d, ptr(mean), ptr(scale), ptr(c), ptr(work), n_work, stream_ptr(x.device)),
          "mmk_pca_cov_f64")
    return c


def pca_eig(c: torch.Tensor, n_components: int, max_iter: int = 0):
    """c (D, D) fp64 symmetric -> (components (n_components, D), variance (n_components,), n_iter): the eigenpairs of the largest
    eigenvalues, falling, each vector's entry of largest magnitude positive.  Block subspace iteration to PCA_TOL |C|_inf; the call waits
    for the stream every 8 iterations; reaching ``max_iter`` (0: PCA_MAX_ITER) raises RuntimeError with the residual reached"""
    d = c.shape[0] if isinstance(c, torch.Tensor) and c.dim() == 2 else -1
    c = _f64_vector(c, (d, d), "pca_eig: c")
    n_components, max_iter = int(n_components), int(max_iter)
    if d < 1 or not 1 <= n_components <= d or max_iter < 0:
        raise ValueError(f"pca_eig: n_components = {n_components} must lie in [1, D = {d}], max_iter = {max_iter} at 0 or above")
    _pca_limits(d, n_components, "pca_eig")
    components = torch.empty((n_components, d), dtype=torch.float64, device=c.device)
    variance = torch.empty((n_components,), dtype=torch.float64, device=c.device)
    n_iter = i32(0)
    n_work = lib().mmk_pca_eig_workspace_bytes(d, n_components)
    work = _workspace(n_work, c.device)
    check(lib().mmk_pca_eig_f64(ptr(c), d, n_components, max_iter, ptr(components), ptr(variance), C.byref(n_iter), ptr(work), n_work,
                                stream_ptr(c.device)), "mmk_pca_eig_f64")
    return components, variance, int(n_iter.value)


def pca_project(y: torch.Tensor, mean: torch.Tensor, scale: torch.Tensor, components: torch.Tensor) -> torch.Tensor:
    """y (M, D) fp32, mean and scale (D,), components (k, D) fp64 -> (M, k) fp32 = ((y - mean) / scale) components^T, summed in fp64"""
    y = _nnn_frames(y, 2, "pca_project")
    m, d = y.shape
    k = components.shape[0] if isinstance(components, torch.Tensor) and components.dim() == 2 else -1
    if m < 1 or d < 1 or k < 1:
        raise ValueError(f"pca_project: y {tuple(y.shape)}, {k} components")
    _pca_limits(d, k, "pca_project")
    mean, scale = _f64_vector(mean, (d,), "pca_project: mean"), _f64_vector(scale, (d,), "pca_project: scale")
    components = _f64_vector(components, (k, d), "pca_project: components")
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    check(lib().mmk_pca_project_f32(ptr(y), y.stride(0), m, d, ptr(mean), ptr(scale), ptr(components), k, ptr(out), out.stride(0),
                                    stream_ptr(y.device)), "mmk_pca_project_f32")
    return out


# include/mmk_nmf.h: MMK_NMF_* - the PCA limits (the Gram matrix and its eigenpairs come from the PCA kernels), the host's read interval of
# the convergence flag, the cut of sklearn's start and the margin of the rank test
NMF_MAX_D = PCA_MAX_D
NMF_MAX_COMPONENTS = PCA_MAX_COMPONENTS
NMF_POLL = 8
NMF_EPS = 1e-6
NMF_RANK_MARGIN = 64.0


def _nmf_shape(x: torch.Tensor, k: int, what: str, start: bool = False):
    """the start needs n_components <= min(N, D) (sklearn's condition for NNDSVDA); the sweeps take any 1 <= n_components <= the limit"""
    x = _nnn_frames(x, 2, what)
    n, d = x.shape
    if n < 1 or d < 1:
        raise ValueError(f"{what}: empty input {tuple(x.shape)}")
    if k < 1 or (start and k > min(n, d)):
        raise ValueError(f"{what}: n_components = {k} must lie in [1, min(N, D) = {min(n, d)}]" if start else
                         f"{what}: n_components = {k} must be at least 1")
    if d > NMF_MAX_D:
        raise NotImplementedError(f"{what}: D = {d} bins, the limit of the HIP path is {NMF_MAX_D} (native.NMF_MAX_D)")
    if k > NMF_MAX_COMPONENTS:
        raise NotImplementedError(f"{what}: n_components = {k}, the limit of the HIP path is {NMF_MAX_COMPONENTS} "
                                  "(native.NMF_MAX_COMPONENTS)")
    return x, n, d


def _nmf_factor(t: torch.Tensor, shape, what: str) -> torch.Tensor:
    """a factor that a call updates in place: float64, contiguous (a copy would take the update with it)"""
    if isinstance(t, torch.Tensor) and not t.is_contiguous():
        raise ValueError(f"{what} is updated in place and must be contiguous, got strides {tuple(t.stride())}")
    return _f64_vector(t, shape, what)


def nmf_start(x: torch.Tensor, n_components: int):
    """x (N >= 2, D) fp32 >= 0 -> (w (N, k), ht (D, k), s (k,), v (k, D)) fp64 on the device and part (k,) int32: sklearn's NNDSVDA start
    from the k leading eigenpairs of X^T X (mmk_nmf.h).  Waits for the stream.  ValueError for a negative entry and for n_components
    beyond the numerical rank of the frames"""
    k = int(n_components)
    x, n, d = _nmf_shape(x, k, "nmf_start", start=True)
    if n < 2:
        raise ValueError(f"nmf_start: N = {n} frames, at least 2 are needed")
    w = torch.empty((n, k), dtype=torch.float64, device=x.device)
    ht = torch.empty((d, k), dtype=torch.float64, device=x.device)
    s = torch.empty((k,), dtype=torch.float64, device=x.device)
    v = torch.empty((k, d), dtype=torch.float64, device=x.device)
    part = torch.empty((k,), dtype=torch.int32, device=x.device)
    n_work = lib().mmk_nmf_start_workspace_bytes(n, d, k)
    work = _workspace(n_work, x.device)
    check(lib().mmk_nmf_start_f64(ptr(x), x.stride(0), n, d, k, ptr(w), ptr(ht), ptr(s), ptr(v), ptr(part), ptr(work), n_work, stream_ptr(x.device)),
          "mmk_nmf_start_f64")
    return w, ht, s, v, part


def _nmf_half(which: str, x: torch.Tensor, w: torch.Tensor, ht: torch.Tensor) -> torch.Tensor:
    k = w.shape[1] if isinstance(w, torch.Tensor) and w.dim() == 2 else -1
    x, n, d = _nmf_shape(x, k, f"nmf_{which}_half")
    w, ht = _nmf_factor(w, (n, k), f"nmf_{which}_half: w"), _nmf_factor(ht, (d, k), f"nmf_{which}_half: ht")
    violation = torch.empty((1,), dtype=torch.float64, device=x.device)
    n_work = lib().mmk_nmf_half_workspace_bytes(n, d, k)
    work = _workspace(n_work, x.device)
    if which == "w":
        rc = lib().mmk_nmf_w_half_f64(ptr(x), x.stride(0), n, d, k, ptr(ht), ptr(w), ptr(violation), ptr(work), n_work, stream_ptr(x.device))
    else:
        rc = lib().mmk_nmf_h_half_f64(ptr(x), x.stride(0), n, d, k, ptr(w), ptr(ht), ptr(violation), ptr(work), n_work, stream_ptr(x.device))
    check(rc, f"mmk_nmf_{which}_half_f64")
    return violation


def nmf_w_half(x: torch.Tensor, w: torch.Tensor, ht: torch.Tensor) -> torch.Tensor:
    """one W half-sweep of sklearn's coordinate descent, w (N, k) fp64 contiguous IN PLACE from ht (D, k); returns the violation (1,)"""
    return _nmf_half("w", x, w, ht)


def nmf_h_half(x: torch.Tensor, w: torch.Tensor, ht: torch.Tensor) -> torch.Tensor:
    """one H half-sweep, ht (D, k) fp64 contiguous IN PLACE from w (N, k); returns the violation (1,)"""
    return _nmf_half("h", x, w, ht)


def nmf_solve(x: torch.Tensor, w: torch.Tensor, ht: torch.Tensor, update_h: bool = True, tol: float = 1e-4, max_iter: int = 200, poll: int = 0,
              check_nonneg: bool = False) -> int:
    """sklearn's _fit_coordinate_descent from (w, ht), both fp64 contiguous and updated IN PLACE (ht only with update_h); returns n_iter.
    The call waits for the stream every ``poll`` iterations (0: NMF_POLL) to read its convergence flag; the result does not depend on it"""
    k = w.shape[1] if isinstance(w, torch.Tensor) and w.dim() == 2 else -1
    x, n, d = _nmf_shape(x, k, "nmf_solve")
    w, ht = _nmf_factor(w, (n, k), "nmf_solve: w"), _nmf_factor(ht, (d, k), "nmf_solve: ht")
    tol, max_iter, poll = float(tol), int(max_iter), int(poll)
    if max_iter < 1 or poll < 0 or not tol >= 0.0:
        raise ValueError(f"nmf_solve: max_iter = {max_iter} must be at least 1, poll = {poll} and tol = {tol} 0 or above")
    n_iter = i32(0)
    n_work = lib().mmk_nmf_solve_workspace_bytes(n, d, k)
    work = _workspace(n_work, x.device)
    check(lib().mmk_nmf_solve_f64(ptr(x), x.stride(0), n, d, k, ptr(w), ptr(ht), 1 if update_h else 0, tol, max_iter, poll, 1 if check_nonneg else 0,
                                  C.byref(n_iter), ptr(work), n_work, stream_ptr(x.device)), "mmk_nmf_solve_f64")
    return int(n_iter.value)


# include/mmk_factor_analysis.h: MMK_FA_* - the PCA limits (the eigen step is the PCA kernels' subspace iteration), the host's read interval
# and sklearn's SMALL
FA_MAX_D = PCA_MAX_D
FA_MAX_COMPONENTS = PCA_MAX_COMPONENTS
FA_POLL = 8
FA_SMALL = 1e-12


def _fa_shape(d: int, k: int, what: str):
    if d < 1 or not 1 <= k <= d:
        raise ValueError(f"{what}: n_components = {k} must lie in [1, D = {d}]")
    if d > FA_MAX_D:
        raise NotImplementedError(f"{what}: D = {d} bins, the limit of the HIP path is {FA_MAX_D} (native.FA_MAX_D)")
    if k > FA_MAX_COMPONENTS:
        raise NotImplementedError(f"{what}: n_components = {k}, the limit of the HIP path is {FA_MAX_COMPONENTS} (native.FA_MAX_COMPONENTS)")


def fa_fit(c: torch.Tensor, n: int, n_components: int, tol: float = 1e-2, max_iter: int = 1000):
    """c (D, D) fp64 = Xc^T Xc / n of n frames -> (components (k, D), noise_variance (D,), loglike (n_iter,), n_iter, converged, (inner
    iterations in all, those of EM step 0)): sklearn's FactorAnalysis EM in Gram form (mmk_factor_analysis.h), the whole loop on the
    device.  The call waits for the stream every 8 inner iterations; an eigen step that does not converge raises NativeError"""
    d = c.shape[0] if isinstance(c, torch.Tensor) and c.dim() == 2 else -1
    c = _f64_vector(c, (d, d), "fa_fit: c")
    n, k, tol, max_iter = int(n), int(n_components), float(tol), int(max_iter)
    _fa_shape(d, k, "fa_fit")
    if n < 2 or max_iter < 1 or not tol >= 0.0:
        raise ValueError(f"fa_fit: n = {n} frames must be at least 2, max_iter = {max_iter} at least 1 and tol = {tol} 0 or above")
    components = torch.empty((k, d), dtype=torch.float64, device=c.device)
    noise = torch.empty((d,), dtype=torch.float64, device=c.device)
    loglike = torch.empty((max_iter,), dtype=torch.float64, device=c.device)
    n_iter, converged, inner = i32(0), i32(0), (i32 * 2)(0, 0)
    n_work = lib().mmk_fa_fit_workspace_bytes(d, k)
    work = _workspace(n_work, c.device)
    check(lib().mmk_fa_fit_f64(ptr(c), d, k, n, tol, max_iter, ptr(components), ptr(noise), ptr(loglike), C.byref(n_iter), C.byref(converged), inner,
                               ptr(work), n_work, stream_ptr(c.device)), "mmk_fa_fit_f64")
    return components, noise, loglike[:int(n_iter.value)].clone(), int(n_iter.value), bool(converged.value), (int(inner[0]), int(inner[1]))


def fa_transform_matrix(components: torch.Tensor, noise_variance: torch.Tensor) -> torch.Tensor:
    """components (k, D), noise_variance (D,) fp64 -> A (k, D) fp64 = (I + Wpsi W^T)^-1 Wpsi, Wpsi = components / noise_variance: sklearn's
    FactorAnalysis.transform is ``pca_project(y, mean_, ones, A)``.  A Cholesky of the k x k matrix in one workgroup; returns without waiting"""
    if not isinstance(components, torch.Tensor) or components.dim() != 2:
        raise TypeError("fa_transform_matrix: components must be a (k, D) float64 tensor")
    k, d = components.shape
    components = _f64_vector(components, (k, d), "fa_transform_matrix: components")
    noise_variance = _f64_vector(noise_variance, (d,), "fa_transform_matrix: noise_variance")
    _fa_shape(d, k, "fa_transform_matrix")
    a = torch.empty((k, d), dtype=torch.float64, device=components.device)
    n_work = lib().mmk_fa_transform_matrix_workspace_bytes(d, k)
    work = _workspace(n_work, components.device)
    check(lib().mmk_fa_transform_matrix_f64(ptr(components), ptr(noise_variance), d, k, ptr(a), ptr(work), n_work, stream_ptr(components.device)),
          "mmk_fa_transform_matrix_f64")
    return a


def _rows(x: torch.Tensor) -> torch.Tensor:
    """(..., n) -> (rows, n) with unit stride along n and ONE stride between rows, without a copy where the layout already
    is that (the length fix-up of STFT hands over a slice ``x[..., -keep:]`` of a contiguous tensor: rows keep their old
    stride, and the kernels take a row stride)"""
    if x.stride(-1) == 1 or x.shape[-1] == 1:
        if x.dim() == 1:
            return x.unsqueeze(0)
        if x.dim() == 2:
            return x
        lead, st = x.shape[:-1], x.stride()[:-1]
        if all(st[i] == st[i + 1] * lead[i + 1] for i in range(len(lead) - 1)):
            return x.as_strided((int(torch.Size(lead).numel()), x.shape[-1]), (st[-1], 1), x.storage_offset())
    return x.reshape(-1, x.shape[-1]).contiguous()


def stft_mag(x: torch.Tensor, n_fft: int, hop: int, center: bool) -> torch.Tensor:
    """x: (..., n_samples) fp32 -> (..., n_frames, n_fft//2+1)"""
    require_device(x)
    if x.dtype != torch.float32:
        x = x.float()
    lead = x.shape[:-1]
    x2 = _rows(x)
    n = x2.shape[-1]
    n_frames = lib().mmk_stft_n_frames(n, n_fft, hop, int(center))
    if n_frames <= 0:
        raise RuntimeError(f"stft: input of {n} samples is shorter than one frame of {n_fft}")
    out = torch.empty((x2.shape[0], n_frames, n_fft // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib().mmk_stft_mag_f32(ptr(x2), x2.stride(0), x2.shape[0], n, n_fft, hop, int(center), ptr(out),
                                 stream_ptr(x.device)), "mmk_stft_mag_f32")
    return out.reshape(*lead, n_frames, n_fft // 2 + 1)


STFT_COORDINATES = {"car": 0, "pol": 1, "angle": 2}


def stft(x: torch.Tensor, n_fft: int, hop: int, center: bool, pad_mode: str, coordinate: str) -> torch.Tensor:
    """x: (..., n_samples) fp32 -> (..., n_frames, n_fft//2+1[, 2]) in the 'car' / 'pol' / 'angle' coordinate"""
    require_device(x)
    if pad_mode not in ("constant", "reflect"):
        raise NotImplementedError(f"HIP STFT covers pad_mode 'constant' and 'reflect', got '{pad_mode}'")
    if x.dtype != torch.float32:
        x = x.float()
    lead = x.shape[:-1]
    x2 = _rows(x)
    n = x2.shape[-1]
    n_frames = lib().mmk_stft_n_frames(n, n_fft, hop, int(center))
    if n_frames <= 0:
        raise RuntimeError(f"stft: input of {n} samples is shorter than one frame of {n_fft}")
    tail = (n_frames, n_fft // 2 + 1) + (() if coordinate == "angle" else (2,))
    out = torch.empty((x2.shape[0],) + tail, dtype=torch.float32, device=x.device)
    check(lib().mmk_stft_f32(ptr(x2), x2.stride(0), x2.shape[0], n, n_fft, hop, int(center), int(pad_mode == "reflect"),
                             STFT_COORDINATES[coordinate], ptr(out), stream_ptr(x.device)), "mmk_stft_f32")
    return out.reshape(*lead, *tail)


def stft_energy(x: torch.Tensor, n_fft: int, hop: int, center: bool, pad_mode: str) -> torch.Tensor:
    """x: (..., n_samples) fp32 -> (..., n_frames): the sum over the bins of each frame's STFT magnitudes (the frames of ``stft``), without
    the spectrogram ever being written"""
    require_device(x)
    if pad_mode not in ("constant", "reflect"):
        raise NotImplementedError(f"HIP STFT covers pad_mode 'constant' and 'reflect', got '{pad_mode}'")
    if x.dtype != torch.float32:
        x = x.float()
    lead = x.shape[:-1]
    x2 = _rows(x)
    n = x2.shape[-1]
    n_frames = lib().mmk_stft_n_frames(n, n_fft, hop, int(center))
    if n_frames <= 0:
        raise RuntimeError(f"stft_energy: input of {n} samples is shorter than one frame of {n_fft}")
    out = torch.empty((x2.shape[0], n_frames), dtype=torch.float32, device=x.device)
    check(lib().mmk_stft_energy_f32(ptr(x2), x2.stride(0), x2.shape[0], n, n_fft, hop, int(center), int(pad_mode == "reflect"), ptr(out),
                                    stream_ptr(x.device)), "mmk_stft_energy_f32")
    return out.reshape(*lead, n_frames)


# include/mmk.h: MMK_INTERP_* / MMK_DERIV_* - the modes of mmk_interp1d_f32, the largest max_lag of mmk_derivative_f32 and the samples one
# workgroup of it owns (csrc/envelope.hip); the tests place their sizes on these
INTERP_MODES = {"linear": 0, "previous": 1}
DERIV_MAX_LAG = 64
DERIV_TILE = 1024


def interp1d(x: torch.Tensor, n_out: int, mode: str = "linear", align: bool = True) -> torch.Tensor:
    """x: (..., n) fp32 -> (..., n_out) along the last dimension.  ``align``: the positions of np.linspace(0, n - 1, n_out) in float64 (scipy's
    interp1d as Interpolate.np_func calls it); otherwise those of torch.nn.functional.interpolate(mode="linear", align_corners=False).
    ``mode``: 'linear', or 'previous' (with ``align`` only)"""
    if mode not in INTERP_MODES:
        raise NotImplementedError(f"interp1d: mode '{mode}' is not on the HIP path ('linear' or 'previous')")
    if mode == "previous" and not align:
        raise ValueError("interp1d: mode 'previous' exists with align=True only")
    x2 = _float32_rows(x, "interp1d")
    batch, n = x2.shape
    n_out = int(n_out)
    if n < 2 or n_out < 1:
        raise ValueError(f"interp1d: needs n >= 2 knots and n_out >= 1 points, got {n} and {n_out}")
    out = torch.empty((batch, n_out), dtype=torch.float32, device=x.device)
    if batch == 0:
        return out.reshape(*x.shape[:-1], n_out)
    check(lib().mmk_interp1d_f32(ptr(x2), x2.stride(0), batch, n, ptr(out), out.stride(0), n_out, INTERP_MODES[mode], int(bool(align)),
                                 stream_ptr(x.device)), "mmk_interp1d_f32")
    return out.reshape(*x.shape[:-1], n_out)


def derivative(x: torch.Tensor, max_lag: int) -> torch.Tensor:
    """x: (..., n) fp32 -> the same shape: the mean over lags 1 .. max_lag of the centred differences (x[i+d] - x[i-d]) / 2d along the last
    dimension, the row continued by odd reflection about its ends (the reference's derivative_torch)"""
    max_lag = int(max_lag)
    if max_lag < 1:
        raise ValueError(f"derivative: max_lag must be at least 1, got {max_lag}")
    if max_lag > DERIV_MAX_LAG:
        raise NotImplementedError(f"derivative: max_lag = {max_lag}, the limit is {DERIV_MAX_LAG}")
    x2 = _float32_rows(x, "derivative")
    batch, n = x2.shape
    if n <= max_lag:
        raise ValueError(f"derivative: the odd reflection of max_lag = {max_lag} needs more than {max_lag} samples, got {n}")
    out = torch.empty((batch, n), dtype=torch.float32, device=x.device)
    if batch == 0:
        return out.reshape(x.shape)
    check(lib().mmk_derivative_f32(ptr(x2), x2.stride(0), batch, n, max_lag, ptr(out), out.stride(0), stream_ptr(x.device)),
          "mmk_derivative_f32")
    return out.reshape(x.shape)


# include/mmk_samplify.h: MMK_SPLINE2_* / MMK_PERIODS_TILE / MMK_SAMPLIFY_* - the knots one workgroup of the coefficient kernel owns and the
# halo a coefficient is solved from, the outputs per step of the evaluation, the samples one workgroup of the period kernels owns, the levels,
# the half window and the lanes per cut of the cut kernel (csrc/samplify.hip); the tests place their sizes on these
SPLINE2_TILE = 256
SPLINE2_HALO = 32
SPLINE2_EVAL_TILE = 256
PERIODS_TILE = 1024
SAMPLIFY_MAX_LEVELS = 6
SAMPLIFY_MAX_WINDOW = 2000
SAMPLIFY_GROUP = 256


def spline2_coef(x: torch.Tensor) -> torch.Tensor:
    """x: (..., n) fp32, rows at any stride -> (..., n) float64: the B-spline coefficients of scipy's interp1d(np.arange(n), x, kind="quadratic")
    (make_interp_spline(k=2), not-a-knot ends) of every row; n >= 3"""
    x2 = _float32_rows(x, "spline2_coef")
    batch, n = x2.shape
    if n < 3:
        raise ValueError(f"spline2_coef: a quadratic spline needs n >= 3 knots, got {n}")
    out = torch.empty((batch, n), dtype=torch.float64, device=x.device)
    if batch == 0:
        return out.reshape(x.shape)
    check(lib().mmk_spline2_coef_f64(ptr(x2), x2.stride(0), batch, n, ptr(out), out.stride(0), stream_ptr(x.device)), "mmk_spline2_coef_f64")
    return out.reshape(x.shape)


def _spline_coef(coef: torch.Tensor, what: str, rows: bool = False) -> torch.Tensor:
    if not isinstance(coef, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(coef)}")
    if coef.dtype != torch.float64:
        raise TypeError(f"{what} takes the float64 coefficients of spline2_coef, got {coef.dtype}")
    require_device(coef)
    if not rows and coef.dim() != 1:
        raise ValueError(f"{what}: expected one row of coefficients, got shape {tuple(coef.shape)}")
    if coef.dim() == 0 or coef.shape[-1] < 3:
        raise ValueError(f"{what}: a quadratic spline needs n >= 3 knots, got shape {tuple(coef.shape)}")
    return coef if rows else coef.contiguous()


def spline2_eval(coef: torch.Tensor, n_out: int) -> torch.Tensor:
    """coef: (..., n) float64 as spline2_coef returns it -> (..., n_out) fp32: the spline at np.linspace(0, n - 1, n_out) (the positions of
    interp1d with align=True), evaluated in float64 and rounded once"""
    coef = _spline_coef(coef, "spline2_eval", rows=True)
    n_out = int(n_out)
    if n_out < 1:
        raise ValueError(f"spline2_eval: needs n_out >= 1 points, got {n_out}")
    c2 = _rows(coef)
    batch, n = c2.shape
    out = torch.empty((batch, n_out), dtype=torch.float32, device=coef.device)
    if batch == 0:
        return out.reshape(*coef.shape[:-1], n_out)
    check(lib().mmk_spline2_eval_f32(ptr(c2), c2.stride(0), batch, n, ptr(out), out.stride(0), n_out, stream_ptr(coef.device)), "mmk_spline2_eval_f32")
    return out.reshape(*coef.shape[:-1], n_out)


def periods(coef: Optional[torch.Tensor], n_samples: int, row: Optional[torch.Tensor] = None):
    """coef: (n,) float64, the spline of a gradient, or (coef None) row: (n_samples,) fp32, the gradient itself -> (att, dec, peaks) int64,
    rising: attack_decay of the reference on the spline's n_samples float32 values, which are never written, or on the row as it is.
    ONE host synchronisation: the two counts the lists are sized by."""
    if (coef is None) == (row is None):
        raise ValueError("periods: exactly one of coef and row must be given")
    if coef is not None:
        src = coef = _spline_coef(coef, "periods")
        n, n_samples = coef.shape[0], int(n_samples)
    else:
        row = _float32_rows(row, "periods")
        if row.shape[0] != 1:
            raise ValueError(f"periods: row must be one (T,) curve, got {row.shape[0]} rows")
        src = row = row[0]
        n, n_samples = 0, row.shape[0]
    if n_samples < 1:
        raise ValueError(f"periods: n_samples = {n_samples} < 1")
    dev = src.device
    n_work = lib().mmk_periods_workspace_bytes(n_samples)
    work = _workspace(n_work, dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    check(lib().mmk_periods_count_i64(ptr(coef), n, ptr(row), n_samples, ptr(counts), ptr(work), n_work, stream_ptr(dev)), "mmk_periods_count_i64")
    n_att, n_peak = (int(v) for v in counts.tolist())
    att, dec = torch.empty((n_att,), dtype=torch.int64, device=dev), torch.empty((n_att,), dtype=torch.int64, device=dev)
    peaks = torch.empty((n_peak,), dtype=torch.int64, device=dev)
    check(lib().mmk_periods_fill_i64(ptr(coef), n, ptr(row), n_samples, ptr(work), n_work, n_att, n_peak, ptr(att) if n_att else None,
                                     ptr(dec) if n_att else None, ptr(peaks) if n_peak else None, stream_ptr(dev)), "mmk_periods_fill_i64")
    return att, dec, peaks


def _index_list(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(t)}")
    if t.dtype != torch.int64 or t.dim() != 1:
        raise TypeError(f"{what} takes (count,) int64 indices, got {t.dtype} of shape {tuple(t.shape)}")
    require_device(t)
    return t.contiguous()


def samplify_scores(env_coef: torch.Tensor, n_samples: int, att: torch.Tensor, dec: torch.Tensor, sensitivity: float = 0.0):
    """-> (scores, env_att, env_dec) fp32 and keep (bool) per attack: the envelope spline at the attack and at its peak, their float32
    difference, and whether it is above fl32(sensitivity)"""
    env_coef = _spline_coef(env_coef, "samplify_scores")
    att, dec = _index_list(att, "samplify_scores"), _index_list(dec, "samplify_scores")
    if att.shape != dec.shape:
        raise ValueError(f"samplify_scores: {att.shape[0]} attacks and {dec.shape[0]} peaks")
    count, dev = att.shape[0], env_coef.device
    scores, ea, ed = (torch.empty((count,), dtype=torch.float32, device=dev) for _ in range(3))
    keep = torch.empty((count,), dtype=torch.uint8, device=dev)
    if count:
        check(lib().mmk_samplify_scores_f32(ptr(env_coef), env_coef.shape[0], int(n_samples), ptr(att), ptr(dec), count, float(sensitivity), ptr(scores),
                                            ptr(ea), ptr(ed), ptr(keep), stream_ptr(dev)), "mmk_samplify_scores_f32")
    return scores, ea, ed, keep.bool()


def samplify_cuts(y: torch.Tensor, env_coefs: Sequence[torch.Tensor], grad_coefs: Sequence[torch.Tensor], coarse_cuts: torch.Tensor,
                  coarse_peaks: torch.Tensor):
    """y (T,) fp32, the levels' envelope and gradient coefficients (level 0 the coarse one), the kept attacks and their peaks ->
    (sides, lr_scores, cuts): which side of each coarse cut the finest envelope falls below the coarse one (0 left, 1 right), the (count, 2)
    left / right scores that decide it, and the refined cuts snapped to a zero crossing of y (include/mmk_samplify.h)"""
    y = _float32_rows(y, "samplify_cuts")
    if y.shape[0] != 1:
        raise ValueError(f"samplify_cuts: y must be one (T,) signal, got {y.shape[0]} rows")
    y = y[0]
    levels = len(env_coefs)
    if levels < 1 or len(grad_coefs) != levels:
        raise ValueError(f"samplify_cuts: {levels} envelope and {len(grad_coefs)} gradient levels")
    if levels > SAMPLIFY_MAX_LEVELS:
        raise NotImplementedError(f"samplify_cuts: {levels} levels, the limit is {SAMPLIFY_MAX_LEVELS} (SAMPLIFY_MAX_LEVELS)")
    env_coefs = [_spline_coef(c, "samplify_cuts") for c in env_coefs]
    grad_coefs = [_spline_coef(c, "samplify_cuts") for c in grad_coefs]
    if any(e.shape != g.shape for e, g in zip(env_coefs, grad_coefs)):
        raise ValueError("samplify_cuts: a level's envelope and gradient have different numbers of knots")
    cc, cp = _index_list(coarse_cuts, "samplify_cuts"), _index_list(coarse_peaks, "samplify_cuts")
    if cc.shape != cp.shape:
        raise ValueError(f"samplify_cuts: {cc.shape[0]} cuts and {cp.shape[0]} peaks")
    count, dev = cc.shape[0], y.device
    sides, cuts = torch.empty((count,), dtype=torch.int64, device=dev), torch.empty((count,), dtype=torch.int64, device=dev)
    lr = torch.empty((count, 2), dtype=torch.float32, device=dev)
    if count:
        e_ptrs = (vp * levels)(*[c.data_ptr() for c in env_coefs])
        g_ptrs = (vp * levels)(*[c.data_ptr() for c in grad_coefs])
        knots = (i64 * levels)(*[c.shape[0] for c in env_coefs])
        check(lib().mmk_samplify_cuts_i64(ptr(y), y.shape[0], e_ptrs, g_ptrs, knots, levels, ptr(cc), ptr(cp), count, ptr(sides), ptr(lr), ptr(cuts),
                                          stream_ptr(dev)), "mmk_samplify_cuts_i64")
    return sides, lr, cuts


# include/mmk.h: MMK_HPSS_* - the largest median window of mmk_hpss_f32 and the frames x bins one workgroup of it owns (csrc/hpss.hip)
HPSS_MAX_KERNEL = 63
HPSS_TILE_FRAMES = 64
HPSS_TILE_BINS = 64


def _pair(v, what: str):
    """a scalar sets both members, a 2-sequence gives (harmonic, percussive), as librosa.decompose.hpss takes them"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"hpss: {what} must be a scalar or a pair (harmonic, percussive), got {v!r}")
        return v[0], v[1]
    return v, v


def hpss(s: torch.Tensor, kernel_size=31, power: float = 1.0, margin=1.0, harmonic: bool = True, percussive: bool = True,
         medians: bool = False):
    """s: (T, F) or (B, T, F) non-negative fp32 magnitudes, time-major -> the requested tensors of s's shape, in the order harmonic,
    percussive, harm_median, perc_median (``medians`` asks for the last two): librosa.decompose.hpss(s^T, kernel_size, power, margin) with
    scipy's reflecting median filters (``mmk_hpss_f32``, one launch on the current stream, no synchronisation, no workspace).  An axis
    shorter than half its window raises ValueError (scipy folds it more than once; not reproduced), a window above HPSS_MAX_KERNEL
    NotImplementedError.  Negative or NaN bins are not looked for: librosa raises on negative ones, here their results are unspecified."""
    if not isinstance(s, torch.Tensor):
        raise TypeError(f"hpss: expected a torch.Tensor, got {type(s)}")
    if s.is_complex():
        raise NotImplementedError("hpss: complex input (librosa's magphase branch) is not on the HIP path: pass the magnitudes")
    if s.dtype != torch.float32:
        raise TypeError(f"hpss runs in float32 on the HIP path, got {s.dtype}")
    if s.dim() not in (2, 3):
        raise ValueError(f"hpss takes (T, F) or (B, T, F), got shape {tuple(s.shape)}")
    win_harm, win_perc = (int(w) for w in _pair(kernel_size, "kernel_size"))
    margin_harm, margin_perc = (float(m) for m in _pair(margin, "margin"))
    power = float(power)
    if win_harm < 1 or win_perc < 1:
        raise ValueError(f"hpss: windows must be at least 1, got ({win_harm}, {win_perc})")
    if margin_harm < 1 or margin_perc < 1:
        raise ValueError(f"hpss: margins must be at least 1, got ({margin_harm}, {margin_perc})")
    if not power > 0:
        raise ValueError(f"hpss: power must be positive, got {power}")
    if win_harm > HPSS_MAX_KERNEL or win_perc > HPSS_MAX_KERNEL:
        raise NotImplementedError(f"hpss: windows ({win_harm}, {win_perc}), the limit of the HIP path is {HPSS_MAX_KERNEL} "
                                  "(native.HPSS_MAX_KERNEL)")
    if not (harmonic or percussive or medians):
        raise ValueError("hpss: no output requested")
    frames, bins = s.shape[-2], s.shape[-1]
    if min(s.shape) < 1 or frames < win_harm // 2 or bins < win_perc // 2:
        raise ValueError(f"hpss: windows ({win_harm}, {win_perc}) need at least ({win_harm // 2}, {win_perc // 2}) frames and bins, "
                         f"got shape {tuple(s.shape)}")
    require_device(s)
    s3 = s if s.dim() == 3 else s.unsqueeze(0)
    if s3.stride(2) != 1 or s3.stride(1) < bins or s3.stride(0) < 0:
        s3 = s3.contiguous()
    batch = s3.shape[0]
    outs = [torch.empty((batch, frames, bins), dtype=torch.float32, device=s.device) if want else None
            for want in (harmonic, percussive, medians, medians)]
    check(lib().mmk_hpss_f32(ptr(s3), s3.stride(0), s3.stride(1), batch, frames, bins, win_harm, win_perc, power, margin_harm, margin_perc,
                             *(ptr(o) for o in outs), frames * bins, bins, stream_ptr(s.device)), "mmk_hpss_f32")
    return tuple(o.reshape(s.shape) for o in outs if o is not None)


# include/mmk.h: MMK_MELBANK_MAX_ROW - the floats of LDS a wave of mmk_melbank_f32 has for a row and its bands (csrc/melbank.hip)
MELBANK_MAX_ROW = 4096


def _bank_args(bank, dct, who: str):
    """(bank_n_bins, n_mels, band_host, band, weights, n_weights, dct, n_mfcc) of include/mmk.h from a features.mel.DeviceBank (or None) and
    a transposed DCT matrix (n_mels, n_mfcc) on the device (or None)"""
    if bank is None and dct is None:
        raise ValueError(f"{who}: neither a bank nor a DCT matrix")
    if dct is not None:
        if dct.dtype != torch.float32 or dct.dim() != 2 or not dct.is_contiguous():
            raise TypeError(f"{who}: the DCT matrix is a contiguous float32 (n_mels, n_mfcc) tensor")
        require_device(dct)
    n_mels = bank.n_mels if bank is not None else dct.shape[0]
    if dct is not None and dct.shape[0] != n_mels:
        raise ValueError(f"{who}: a DCT matrix over {dct.shape[0]} bands behind a bank of {n_mels}")
    n_mfcc = dct.shape[1] if dct is not None else 0
    if bank is None:
        return (0, n_mels, None, None, None, 0, ptr(dct), n_mfcc)
    return (bank.n_bins, n_mels, bank.table_host.ctypes.data, ptr(bank.table), ptr(bank.weights), bank.weights.numel(), ptr(dct), n_mfcc)


def melbank(s: torch.Tensor, bank=None, dct: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s: (..., n_bins) fp32 magnitudes -> (..., n_mels) through ``bank`` (features.mel.device_bank), or (..., n_mfcc) with the DCT matrix
    ``dct`` (features.mel.device_dct: transposed, (n_mels, n_mfcc)) behind it; ``bank=None`` applies the DCT alone to rows that already are
    mel bands.  One launch of ``mmk_melbank_f32`` on the current stream."""
    if not isinstance(s, torch.Tensor):
        raise TypeError(f"melbank: expected a torch.Tensor, got {type(s)}")
    if s.dtype != torch.float32:
        raise TypeError(f"melbank runs in float32 on the HIP path, got {s.dtype}")
    if s.dim() < 1 or s.shape[-1] < 1:
        raise ValueError(f"melbank takes (..., n_bins), got shape {tuple(s.shape)}")
    require_device(s)
    args = _bank_args(bank, dct, "melbank")
    n_bins = s.shape[-1]
    if bank is not None and bank.n_bins != n_bins:
        raise ValueError(f"melbank: the bank was built for {bank.n_bins} bins, the input has {n_bins}")
    if bank is None and n_bins != args[1]:
        raise ValueError(f"melbank: the DCT matrix takes {args[1]} bands, the input has {n_bins}")
    if n_bins + args[1] > MELBANK_MAX_ROW:
        raise NotImplementedError(f"melbank: n_bins + n_mels = {n_bins} + {args[1]}, the limit of the HIP path is {MELBANK_MAX_ROW}")
    n_out = args[7] if dct is not None else args[1]
    s2 = _rows(s)
    out = torch.empty((s2.shape[0], n_out), dtype=torch.float32, device=s.device)
    if s2.shape[0] == 0:
        return out.reshape(*s.shape[:-1], n_out)
    check(lib().mmk_melbank_f32(ptr(s2), s2.stride(0), s2.shape[0], n_bins, *args, ptr(out), stream_ptr(s.device)), "mmk_melbank_f32")
    return out.reshape(*s.shape[:-1], n_out)


# include/mmk.h: MMK_NOVELTY_* - output frames of one workgroup of mmk_novelty_f32, the half-widths one launch sums, the largest of them and the
# longest wait of mmk_pick_peaks_f32 (csrc/novelty.hip); the tests place their sizes on these
NOVELTY_TILE = 64
NOVELTY_MAX_KERNELS = 8
NOVELTY_MAX_HALF = 32
NOVELTY_MAX_WAIT = 1024


def _novelty_halves(halves, what: str):
    halves = [int(h) for h in halves]
    if not halves or min(halves) < 1:
        raise ValueError(f"{what}: half-widths must be positive integers, got {halves}")
    if len(halves) > NOVELTY_MAX_KERNELS:
        raise NotImplementedError(f"{what}: {len(halves)} half-widths, the limit is {NOVELTY_MAX_KERNELS}")
    if max(halves) > NOVELTY_MAX_HALF:
        raise NotImplementedError(f"{what}: half-width {max(halves)}, the limit is {NOVELTY_MAX_HALF}")
    return halves


def novelty(x: torch.Tensor, halves: Sequence[int], inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (T, D) or (B, T, D) fp32, bins contiguous, frames and clips at any stride; halves: up to NOVELTY_MAX_KERNELS half-widths in
    [1, NOVELTY_MAX_HALF]; inv_norm (T,) / (B, T) = inv_row_norm(x), computed inside the kernel if not given -> raw (len(halves), T) or
    (B, len(halves), T) fp32: the normalised checkerboard of 2 h + 1 summed along the diagonal of the cosine self-distance matrix, centred on
    (i, i - 1), terms outside the matrix counting 0 (``mmk_novelty_f32``, one launch, the matrix is never formed)"""
    halves = _novelty_halves(halves, "novelty")
    x = _nnn_frames(x, 2 if isinstance(x, torch.Tensor) and x.dim() == 2 else 3, "novelty")
    x3 = x.unsqueeze(0) if x.dim() == 2 else x
    batch, frames, bins = x3.shape
    if batch < 1 or bins < 1 or frames < 2:
        raise ValueError(f"novelty: at least two frames of at least one bin per clip, got {tuple(x.shape)}")
    if inv_norm is not None:
        require_device(inv_norm)
        if inv_norm.shape != x.shape[:-1] or inv_norm.dtype != torch.float32 or not inv_norm.is_contiguous():
            raise ValueError(f"novelty: inv_norm must be {tuple(x.shape[:-1])} contiguous float32 values, got {tuple(inv_norm.shape)} {inv_norm.dtype}")
    raw = torch.empty((batch, len(halves), frames), dtype=torch.float32, device=x.device)
    check(lib().mmk_novelty_f32(ptr(x3), x3.stride(0), x3.stride(1), ptr(inv_norm), batch, frames, bins, (i32 * len(halves))(*halves), len(halves),
                                ptr(raw), stream_ptr(x.device)), "mmk_novelty_f32")
    return raw[0] if x.dim() == 2 else raw


def novelty_finish(raw: torch.Tensor):
    """raw (n_half, T) or (B, n_half, T) fp32 -> (scores of the same shape, dg (T,) or (B, T)): scores = raw minus its minimum over the frames,
    dg = the mean of the scores over the half-widths (``mmk_novelty_finish_f32``)"""
    raw = _nnn_frames(raw, 2 if isinstance(raw, torch.Tensor) and raw.dim() == 2 else 3, "novelty_finish").contiguous()
    r3 = raw.unsqueeze(0) if raw.dim() == 2 else raw
    batch, n_half, frames = r3.shape
    if min(batch, n_half, frames) < 1:
        raise ValueError(f"novelty_finish: empty input {tuple(raw.shape)}")
    if n_half > NOVELTY_MAX_KERNELS:
        raise NotImplementedError(f"novelty_finish: {n_half} half-widths, the limit is {NOVELTY_MAX_KERNELS}")
    scores = torch.empty_like(r3)
    dg = torch.empty((batch, frames), dtype=torch.float32, device=raw.device)
    n_work = lib().mmk_novelty_finish_workspace_floats(batch, n_half, frames)
    work = _workspace(4 * n_work, raw.device)
    check(lib().mmk_novelty_finish_f32(ptr(r3), batch, n_half, frames, ptr(scores), ptr(dg), ptr(work), n_work, stream_ptr(raw.device)),
          "mmk_novelty_finish_f32")
    return (scores[0], dg[0]) if raw.dim() == 2 else (scores, dg)


def pick_peaks(x: torch.Tensor, wait_before: int, wait_after: int, min_strength: float = 0.02) -> torch.Tensor:
    """x (T,) fp32 -> picked (T,) bool on the device: the indices the reference's pick_globally_sorted_maxes accepts (equal values taken by
    rising index); no host synchronisation (``mmk_pick_peaks_f32``)"""
    wait_before, wait_after = int(wait_before), int(wait_after)
    if min(wait_before, wait_after) < 0 or wait_before + wait_after < 1:
        raise ValueError(f"pick_peaks: waits must be non-negative and not both zero, got {wait_before}, {wait_after}")
    if max(wait_before, wait_after) > NOVELTY_MAX_WAIT:
        raise NotImplementedError(f"pick_peaks: waits of {wait_before}, {wait_after}, the limit is {NOVELTY_MAX_WAIT}")
    x = _nnn_frames(x, 1, "pick_peaks")
    if x.shape[0] < 1:
        raise ValueError("pick_peaks: empty input")
    n = x.shape[0]
    picked = torch.empty((n,), dtype=torch.uint8, device=x.device)
    n_work = lib().mmk_pick_peaks_workspace_bytes(n)
    work = _workspace(n_work, x.device)
    check(lib().mmk_pick_peaks_f32(ptr(x), n, wait_before, wait_after, float(min_strength), ptr(picked), ptr(work), n_work, stream_ptr(x.device)),
          "mmk_pick_peaks_f32")
    return picked.bool()


def stft_mel(x: torch.Tensor, n_fft: int, hop: int, center: bool, pad_mode: str, bank, dct: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: (..., n_samples) fp32 -> (..., n_frames, n_mels), or (..., n_frames, n_mfcc) with ``dct``: ``melbank(stft magnitudes, bank, dct)``
    as ONE launch (``mmk_stft_mel_f32``); the spectrogram is never written.  With pad_mode 'constant' the result equals
    ``melbank(stft_mag(x, ...), bank, dct)`` bit for bit."""
    require_device(x)
    if pad_mode not in ("constant", "reflect"):
        raise NotImplementedError(f"HIP STFT covers pad_mode 'constant' and 'reflect', got '{pad_mode}'")
    if bank is None:
        raise ValueError("stft_mel: needs a bank")
    if x.dtype != torch.float32:
        x = x.float()
    args = _bank_args(bank, dct, "stft_mel")
    if bank.n_bins != n_fft // 2 + 1:
        raise ValueError(f"stft_mel: the bank was built for {bank.n_bins} bins, n_fft = {n_fft} gives {n_fft // 2 + 1}")
    if bank.n_mels > n_fft // 2:
        raise NotImplementedError(f"stft_mel: n_mels = {bank.n_mels}, the limit of the fused path at n_fft = {n_fft} is {n_fft // 2}")
    lead = x.shape[:-1]
    x2 = _rows(x)
    n = x2.shape[-1]
    n_frames = lib().mmk_stft_n_frames(n, n_fft, hop, int(center))
    if n_frames <= 0:
        raise RuntimeError(f"stft_mel: input of {n} samples is shorter than one frame of {n_fft}")
    n_out = args[7] if dct is not None else args[1]
    out = torch.empty((x2.shape[0], n_frames, n_out), dtype=torch.float32, device=x.device)
    check(lib().mmk_stft_mel_f32(ptr(x2), x2.stride(0), x2.shape[0], n, n_fft, hop, int(center), int(pad_mode == "reflect"), *args, ptr(out),
                                 stream_ptr(x.device)), "mmk_stft_mel_f32")
    return out.reshape(*lead, n_frames, n_out)


def istft(spec: torch.Tensor, n_fft: int, hop: int, polar: bool) -> torch.Tensor:
    """spec: (..., n_frames, n_fft//2+1, 2) fp32, (re, im) or (abs, angle) -> (..., hop * (n_frames - 1))"""
    require_device(spec)
    if spec.shape[-1] != 2 or spec.shape[-2] != n_fft // 2 + 1:
        raise RuntimeError(f"istft: expected (..., n_frames, {n_fft // 2 + 1}, 2), got {tuple(spec.shape)}")
    lead = spec.shape[:-3]
    s3 = spec.reshape(-1, *spec.shape[-3:]).contiguous().float()
    batch, n_frames = s3.shape[0], s3.shape[1]
    n_out = lib().mmk_istft_n_samples(n_frames, n_fft, hop)
    n_work = lib().mmk_istft_workspace_floats(batch, n_frames, n_fft)
    work = torch.empty(n_work, dtype=torch.float32, device=spec.device) if n_work else None
    out = torch.empty((batch, n_out), dtype=torch.float32, device=spec.device)
    check(lib().mmk_istft_f32(ptr(s3), int(polar), batch, n_frames, n_fft, hop, ptr(work), ptr(out), stream_ptr(spec.device)),
          "mmk_istft_f32")
    return out.reshape(*lead, n_out)


def griffin_lim(mag: torch.Tensor, n_fft: int, hop: int, n_iter: int = 32, momentum: float = 0.99,
                init: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mag: (..., n_frames, n_fft//2+1) fp32; init: complex64 of the same shape (initial phase estimates) or None (ones)"""
    require_device(mag)
    lead = mag.shape[:-2]
    m3 = mag.reshape(-1, *mag.shape[-2:]).contiguous().float()
    batch, n_frames = m3.shape[0], m3.shape[1]
    init_ri = None
    if init is not None:
        if tuple(init.shape) != tuple(mag.shape) or not init.is_complex():
            raise RuntimeError("griffin_lim: init must be a complex tensor shaped like mag")
        init_ri = torch.view_as_real(init.to(torch.complex64).reshape(m3.shape).contiguous())
    n_out = lib().mmk_istft_n_samples(n_frames, n_fft, hop)
    work = torch.empty(lib().mmk_gla_workspace_floats(batch, n_frames, n_fft, hop), dtype=torch.float32, device=mag.device)
    out = torch.empty((batch, n_out), dtype=torch.float32, device=mag.device)
    check(lib().mmk_gla_f32(ptr(m3), ptr(init_ri) if init_ri is not None else None, batch, n_frames, n_fft, hop, n_iter,
                            momentum, ptr(work), ptr(out), stream_ptr(mag.device)), "mmk_gla_f32")
    return out.reshape(*lead, n_out)


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------
def pack_weight(w: torch.Tensor) -> torch.Tensor:
    require_device(w)
    w = w.contiguous().float()
    n, k = w.shape
    out = torch.empty(lib().mmk_packed_weight_floats(n, k), dtype=torch.float32, device=w.device)
    check(lib().mmk_pack_weight_f32(ptr(w), w.stride(0), n, k, ptr(out), stream_ptr(w.device)), "mmk_pack_weight_f32")
    return out


def _act_code(act) -> int:
    """an ACT name, or an MMK_ACT_* code passed through as it is (the library refuses codes outside 0..8)"""
    return act if isinstance(act, int) else ACT[act]


def linear(x: torch.Tensor, packed_w: torch.Tensor, bias: Optional[torch.Tensor], n: int, k: int,
           act="none") -> torch.Tensor:
    require_device(x, packed_w, bias)
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], n), dtype=torch.float32, device=x.device)
    check(lib().mmk_linear_f32(ptr(x2), x2.stride(0), x2.shape[0], ptr(packed_w), ptr(bias), n, k, ptr(y), y.stride(0),
                               _act_code(act), stream_ptr(x.device)), "mmk_linear_f32")
    return y.reshape(*x.shape[:-1], n)


# The single kernels behind the plans (include/mmk.h: building blocks), for the unit tests.  They write into caller-owned tensors at
# the strides (in elements) they are given: the caller sizes the buffers, exactly as a C caller would.
def gemm_f32(a: torch.Tensor, lda: int, a_batch: int, packed_w: torch.Tensor, n: int, k: int, c: torch.Tensor, ldc: int, c_batch: int,
             m: int, batch: int = 1):
    """C[b][m, n] = A[b][m, k] @ W^T (csrc/gemm.hip: gemm_f32_kernel)"""
    require_device(a, packed_w, c)
    check(lib().mmk_gemm_f32(ptr(a), lda, a_batch, ptr(packed_w), n, k, ptr(c), ldc, c_batch, m, batch, stream_ptr(a.device)),
          "mmk_gemm_f32")


def gemm_partial_floats(m: int, n: int, k: int, k_split: int = 0) -> int:
    return int(lib().mmk_gemm_partial_floats(m, n, k, k_split))


def gemm_bias_act(a: torch.Tensor, lda: int, m: int, packed_w: torch.Tensor, bias: Optional[torch.Tensor], n: int, k: int,
                  c: torch.Tensor, ldc: int, act="none", row_map=(0, 0, 0, 0), partial: Optional[torch.Tensor] = None,
                  k_split: int = 0):
    """C = act(A @ W^T + bias) (csrc/gemm.hip: gemm_bias_act_kernel, gemm_split_reduce_kernel); row_map = (group, kept,
    group_stride, row_stride); partial: gemm_partial_floats(m, n, k, k_split) floats, or None"""
    require_device(a, packed_w, bias, c, partial)
    group, kept, group_stride, row_stride = row_map
    check(lib().mmk_gemm_bias_act_f32(ptr(a), lda, m, ptr(packed_w), ptr(bias), n, k, ptr(c), ldc, _act_code(act), group, kept,
                                      group_stride, row_stride, ptr(partial), 0 if partial is None else partial.numel(), k_split,
                                      stream_ptr(a.device)), "mmk_gemm_bias_act_f32")


def skinny_linear(a: torch.Tensor, lda: int, m: int, packed_w: torch.Tensor, bias: Optional[torch.Tensor], n: int, k: int,
                  c: torch.Tensor, ldc: int, act="none"):
    """C = act(A @ W^T + bias) for m <= 64 (csrc/skinny.hip)"""
    require_device(a, packed_w, bias, c)
    check(lib().mmk_skinny_linear_f32(ptr(a), lda, m, ptr(packed_w), ptr(bias), n, k, ptr(c), ldc, _act_code(act),
                                      stream_ptr(a.device)), "mmk_skinny_linear_f32")


def tr_attention(q: torch.Tensor, q_ld: int, q_cs: int, k: torch.Tensor, v: torch.Tensor, kv_ld: int, kv_cs: int, out: torch.Tensor,
                 o_ld: int, o_cs: int, n_q: int, q_pos0: int, n_keys: int, n_heads: int, head_dim: int, scale: float, batch: int):
    """causal multi-head attention (csrc/transformer.hip: tr_attention_kernel); q / k / v / out point at row 0, column 0 of clip 0"""
    require_device(q, k, v, out)
    check(lib().mmk_tr_attention_f32(ptr(q), q_ld, q_cs, ptr(k), ptr(v), kv_ld, kv_cs, ptr(out), o_ld, o_cs, n_q, q_pos0, n_keys,
                                     n_heads, head_dim, scale, batch, stream_ptr(q.device)), "mmk_tr_attention_f32")


def tr_add_ln(y: torch.Tensor, y_ld: int, res: Optional[torch.Tensor], res_ld: int, w: torch.Tensor, b: torch.Tensor,
              out: torch.Tensor, out_ld: int, rows: int, d: int):
    """out = LayerNorm(y + res) * w + b, eps 1e-5 (csrc/transformer.hip: tr_add_ln_kernel); res None: no residual; out may be res"""
    require_device(y, res, w, b, out)
    check(lib().mmk_tr_add_ln_f32(ptr(y), y_ld, ptr(res), res_ld, ptr(w), ptr(b), ptr(out), out_ld, rows, d, stream_ptr(y.device)),
          "mmk_tr_add_ln_f32")


def categorical_sample(logits: torch.Tensor, n_classes: int, has_temp_col: bool, min_temp: float,
                       temperature: Optional[torch.Tensor], uniforms: Optional[torch.Tensor]) -> torch.Tensor:
    require_device(logits, temperature, uniforms)
    lg = logits.reshape(-1, logits.shape[-1])
    if lg.stride(-1) != 1:
        lg = lg.contiguous()
    rows = lg.shape[0]
    out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    check(lib().mmk_categorical_sample_f32_i64(ptr(lg), lg.stride(0), rows, n_classes, int(has_temp_col), min_temp,
                                               ptr(temperature), ptr(uniforms), ptr(out), 1,
                                               stream_ptr(logits.device)), "mmk_categorical_sample_f32_i64")
    return out.reshape(logits.shape[:-1])


# ---------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------
class _Plan:
    """Owns one native plan handle and its torch-allocated workspace."""
    _prefix = ""
    _has_sync_status = False    # the library keeps an error word for this plan's waiting kernels (`<prefix>_sync_status`, `<prefix>_inject_sync_error`)

    def __init__(self, cfg_struct, device: torch.device):
        self._lib = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"plans live on the HIP device; got '{device}' (no CPU implementation in this package)")
        self.cfg = cfg_struct
        if not cfg_struct.tuning:         # (a network's own switches are already in it; the process-wide ones otherwise)
            cfg_struct.tuning = tuning_text(PLAN_TUNING)
        handle = vp()
        check(getattr(self._lib, self._prefix + "_plan_create")(C.byref(cfg_struct), C.byref(handle)),
              self._prefix + "_plan_create")
        self.handle = handle
        self.workspace = None
        self._bound = {}

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                if torch.cuda.is_available():
                    torch.cuda.synchronize(self.device)
                getattr(self._lib, self._prefix + "_plan_destroy")(self.handle)
                self.handle = None
        except Exception:
            pass

    def bind_state_dict(self, tensors):
        for key, t in tensors.items():
            if not torch.is_floating_point(t) or t.dim() == 0:
                continue
            require_device(t)
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            self._bound[key] = t  # keep alive: the plan reads these pointers at commit
            check(getattr(self._lib, self._prefix + "_plan_bind")(self.handle, key.encode(), ptr(t), t.numel()),
                  self._prefix + "_plan_bind")

    def commit(self):
        need = getattr(self._lib, self._prefix + "_workspace_bytes")(self.handle)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = self.workspace.data_ptr()
        aligned = (base + 255) // 256 * 256
        check(getattr(self._lib, self._prefix + "_commit")(self.handle, aligned, need, stream_ptr(self.device)),
              self._prefix + "_commit")
        self.workspace_bytes = need

    def sync_status(self):
        """wait for the stream and raise if a wait between workgroups of one of the plan's kernels (a hand-off of the persistent
        WaveNet kernels, the resident SampleRNN and bi-LSTM kernels) timed out"""
        if not self._has_sync_status:
            raise AttributeError(f"{type(self).__name__} has no sync_status: its kernels do not wait for each other")
        check(getattr(self._lib, self._prefix + "_sync_status")(self.handle, stream_ptr(self.device)), self._prefix + "_sync_status")

    def inject_sync_error(self):
        """fault injection for tests: the next ``sync_status`` fails as after a timed-out wait (include/mmk.h)"""
        if not self._has_sync_status:
            raise AttributeError(f"{type(self).__name__} has no inject_sync_error: its kernels do not wait for each other")
        check(getattr(self._lib, self._prefix + "_inject_sync_error")(self.handle, stream_ptr(self.device)),
              self._prefix + "_inject_sync_error")

    def _logit_columns(self, classes: str, target: int) -> int:
        """columns of target k's raw head outputs: its classes (config field ``classes``, ``x_<classes>`` from target 1 on) and
        the learned temperature's column"""
        c = self.cfg
        if target == 0:
            return getattr(c, classes) + (1 if c.learn_temp else 0)
        return getattr(c, "x_" + classes)[target] + (1 if c.x_learn_temp[target] else 0)

    def _check_uniforms(self, uniforms: Optional[torch.Tensor], batch: int, n_steps: int):
        n_tgt = max(int(self.cfg.n_targets), 1)
        if uniforms is not None and (uniforms.dtype != torch.float32 or not uniforms.is_contiguous()
                                     or uniforms.numel() != n_tgt * batch * n_steps):
            raise ValueError("uniforms must be contiguous fp32 of shape (batch, n_steps) - (n_targets, batch, n_steps) with several targets")


def pack_launch_count() -> int:
    """weight re-packing kernels launched so far (diagnostic; see include/mmk.h)"""
    return int(lib().mmk_pack_launch_count())


def weights_identity(module: torch.nn.Module):
    """host-side identity of a module's weights as a plan packed them: storage address, in-place version counter and shape of
    every state_dict entry.  Optimiser steps and ``load_state_dict`` bump the version, ``.to(device)`` moves the storage."""
    return tuple((k, v.data_ptr(), v._version, tuple(v.shape)) for k, v in module.state_dict(keep_vars=True).items())


def weights_fingerprint(module: torch.nn.Module) -> int:
    """A write through ``.data`` (``p.data.copy_(ema)``, weight surgery) bumps no version counter and moves no storage: a
    position-mixed hash of all fp32 entries is summed on their device (``mmk_fingerprint_buffers_u32``: the entries where they lie,
    one launch per 96 of them, one read-back - which waits for the stream).  Taken where a generation starts (``before_generate``),
    not on every step of one.  Entries on the host are hashed there."""
    entries = [v.detach() for v in module.state_dict(keep_vars=True).values() if v.dtype == torch.float32 and v.numel() > 0]
    if not entries:
        return 0
    dev = entries[0].device
    if dev.type != "cuda":
        import zlib
        return zlib.crc32(b"".join(v.contiguous().cpu().numpy().tobytes() for v in entries))
    entries = [v if v.is_contiguous() else v.contiguous() for v in entries]
    n = len(entries)
    ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in entries])
    counts = (i64 * n)(*[v.numel() for v in entries])
    out = torch.empty(1, dtype=torch.int64, device=dev)
    check(lib().mmk_fingerprint_buffers_u32(ptrs, counts, n, ptr(out), stream_ptr(dev)), "mmk_fingerprint_buffers_u32")
    return int(out.item())


class WeightsTracker:
    """decides whether a plan's packed copy of the weights is still current"""

    def __init__(self):
        self.ident, self.print_ = None, None

    def changed(self, module: torch.nn.Module, content: bool) -> bool:
        """``content``: also compare the content fingerprint (the start of a generation); without it only the host-side identity"""
        ident = weights_identity(module)
        if ident != self.ident:
            return True
        return content and weights_fingerprint(module) != self.print_

    def committed(self, module: torch.nn.Module):
        self.ident, self.print_ = weights_identity(module), weights_fingerprint(module)


def abs_ptr(view: torch.Tensor, t_first: int) -> int:
    """address A such that A + t * stride(1) * itemsize is ``view[:, t - t_first]``: lets a window
    view of a longer (batch, T, ...) tensor be addressed by absolute time on the device"""
    return view.data_ptr() - t_first * view.stride(1) * view.element_size()


def _cond_arrays(cond: Sequence[torch.Tensor], t_first: int):
    n = len(cond)
    ptrs = (vp * max(n, 1))(*[abs_ptr(c, t_first) for c in cond])
    strides = (i64 * max(n, 1))(*[c.stride(0) for c in cond])
    return ptrs, strides


class WaveNetPlan(_Plan):
    """``in0`` / ``cond`` arguments are (batch, T[, dim]) tensors (or views) whose column 0 is
    absolute time ``t_first``; all ``t`` arguments are absolute times."""
    _prefix = "mmk_wavenet"
    _has_sync_status = True
    MODE_CHAIN, MODE_LPIPE, MODE_SPIPE, MODE_BPIPE = 2, 4, 5, 6      # mmk_wavenet_mode (include/mmk.h); 0: the per-layer launch path

    @property
    def rf(self) -> int:
        return self._lib.mmk_wavenet_receptive_field(self.handle)

    def _check_inputs(self, in0, cond):
        require_device(in0, *cond)
        if self.cfg.q_levels > 0:
            if in0.dtype != torch.int64 or in0.dim() != 2 or in0.stride(1) != 1:
                raise ValueError("input 0 must be int64 (batch, T) with unit stride along time")
        else:
            if in0.dtype != torch.float32 or in0.dim() != 3 or in0.stride(2) != 1 or in0.stride(1) != in0.shape[2]:
                raise ValueError("input 0 must be fp32 (batch, T, dim), contiguous along time and dim")
        if len(cond) != self.cfg.n_cond:
            raise ValueError(f"expected {self.cfg.n_cond} conditioning inputs, got {len(cond)}")
        for j, c in enumerate(cond):
            if self.cfg.cond_q_levels[j] > 0:
                if c.dtype != torch.int64 or c.dim() != 2 or c.stride(1) != 1:
                    raise ValueError(f"input {j + 1} is a class stream: int64 (batch, T) with unit stride along time")
            elif c.dtype != torch.float32 or c.dim() != 3 or c.stride(2) != 1 or c.stride(1) != c.shape[2]:
                raise ValueError("conditioning inputs must be fp32 (batch, T, dim), contiguous along time and dim")

    def warmup(self, in0: torch.Tensor, cond: Sequence[torch.Tensor], t_begin: int, t_end: int, t_first: int = 0):
        self._check_inputs(in0, cond)
        ptrs, strides = _cond_arrays(cond, t_first)
        check(self._lib.mmk_wavenet_warmup(self.handle, in0.shape[0], abs_ptr(in0, t_first), in0.stride(0), ptrs,
                                           strides, t_begin, t_end, stream_ptr(self.device)), "mmk_wavenet_warmup")

    def generate(self, in0: torch.Tensor, cond: Sequence[torch.Tensor], t0: int, n_steps: int,
                 temperature: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
                 t_first: int = 0):
        self._check_inputs(in0, cond)
        require_device(temperature, uniforms)
        self._check_uniforms(uniforms, in0.shape[0], n_steps)
        ptrs, strides = _cond_arrays(cond, t_first)
        check(self._lib.mmk_wavenet_generate(self.handle, in0.shape[0], abs_ptr(in0, t_first), in0.stride(0), ptrs,
                                             strides, t0, n_steps, ptr(temperature), ptr(uniforms),
                                             stream_ptr(self.device)), "mmk_wavenet_generate")

    @property
    def persistent(self) -> bool:
        return bool(self._lib.mmk_wavenet_mode(self.handle))

    @property
    def chain(self) -> bool:
        """persistent mode with one hand-off per layer (csrc/wavenet_chain.hip)"""
        return self._lib.mmk_wavenet_mode(self.handle) == self.MODE_CHAIN

    @property
    def layer_pipelined(self) -> bool:
        """persistent mode with four workgroups per clip that own whole layers (csrc/wavenet_lpipe.hip)"""
        return self._lib.mmk_wavenet_mode(self.handle) == self.MODE_LPIPE

    @property
    def stage_pipelined(self) -> bool:
        """persistent mode with one layer per stage of 8 CUs: the clips streamed through one at a time (csrc/wavenet_spipe.hip) or,
        large batches, in groups of 16 (csrc/wavenet_bpipe.hip)"""
        return self._lib.mmk_wavenet_mode(self.handle) in (self.MODE_SPIPE, self.MODE_BPIPE)

    @property
    def pair_visits(self) -> bool:
        """the last launch of the one-clip ring took two clips per visit (csrc/wavenet_spipe_pair.inc)"""
        return bool(self._lib.mmk_wavenet_pair_visits(self.handle))

    @property
    def batch_pipelined(self) -> bool:
        """the stage pipeline with groups of 16 clips per visit on the matrix pipe (csrc/wavenet_bpipe.hip)"""
        return self._lib.mmk_wavenet_mode(self.handle) == self.MODE_BPIPE

    def profile_steps(self, in0: torch.Tensor, cond: Sequence[torch.Tensor], t0: int, n_steps: int, t_first: int = 0):
        """measurement aid: per-kernel-class device time from HIP events (see include/mmk.h);
        returns {"layer_a": (ms_total, launches), "layer_b": ..., "other": ...}"""
        self._check_inputs(in0, cond)
        ptrs, strides = _cond_arrays(cond, t_first)
        ms = (C.c_double * 3)()
        cnt = (i64 * 3)()
        check(self._lib.mmk_wavenet_profile_steps(self.handle, in0.shape[0], abs_ptr(in0, t_first), in0.stride(0), ptrs,
                                                  strides, t0, n_steps, ms, cnt, stream_ptr(self.device)),
              "mmk_wavenet_profile_steps")
        return {name: (ms[i], cnt[i]) for i, name in enumerate(("layer_a", "layer_b", "other"))}

    def last_logits(self, batch: int, target: int = 0) -> torch.Tensor:
        out = torch.empty((batch, self._logit_columns("out_dim", target)), dtype=torch.float32, device=self.device)
        check(self._lib.mmk_wavenet_last_logits_of(self.handle, target, batch, ptr(out), out.stride(0), stream_ptr(self.device)),
              "mmk_wavenet_last_logits_of")
        return out


SPIPE_MAX_CLIPS = 128      # clips one ring of the stage pipeline streams (csrc/wavenet_spipe.h: kSpMaxClips)
BPIPE_MAX_CLIPS = 512      # clips one launch of its large-batch form takes, in groups of 16 (csrc/wavenet_bpipe.h: kBpMaxClips)


class WaveNetPlanSet:
    """Several :class:`WaveNetPlan` s, each owning a contiguous slice of the batch, behind the interface of one.

    The stage pipeline (``csrc/wavenet_spipe.hip``) streams at most ``SPIPE_MAX_CLIPS`` clips through its ring; the reference's
    loop takes any batch (``loops/generate.py:207-219``), so a larger one runs as successive passes of the same kernel, one
    per slice - each slice has its own history rings and message blocks, the weights are packed once per plan."""

    def __init__(self, plans: Sequence["WaveNetPlan"], sizes: Sequence[int]):
        self.plans, self.sizes = list(plans), list(sizes)
        self.cfg, self.device = self.plans[0].cfg, self.plans[0].device

    def _slices(self, batch: int):
        off = 0
        for plan, size in zip(self.plans, self.sizes):
            n = min(size, batch - off)
            if n <= 0:
                break
            yield plan, off, off + n
            off += n
        if off < batch:
            raise ValueError(f"batch of {batch} clips exceeds the {sum(self.sizes)} this plan set was built for")

    def bind_state_dict(self, tensors):
        for plan in self.plans:
            plan.bind_state_dict(tensors)

    def commit(self):
        for plan in self.plans:
            plan.commit()

    @property
    def rf(self) -> int:
        return self.plans[0].rf

    def warmup(self, in0, cond, t_begin, t_end, t_first=0):
        for plan, a, b in self._slices(in0.shape[0]):
            plan.warmup(in0[a:b], [c[a:b] for c in cond], t_begin, t_end, t_first=t_first)

    def generate(self, in0, cond, t0, n_steps, temperature=None, uniforms=None, t_first=0):
        for plan, a, b in self._slices(in0.shape[0]):
            plan.generate(in0[a:b], [c[a:b] for c in cond], t0, n_steps,
                          None if temperature is None else temperature[a:b].contiguous(),
                          None if uniforms is None else uniforms[a:b].contiguous(), t_first=t_first)

    persistent = property(lambda self: self.plans[0].persistent)
    chain = property(lambda self: self.plans[0].chain)
    layer_pipelined = property(lambda self: self.plans[0].layer_pipelined)
    stage_pipelined = property(lambda self: self.plans[0].stage_pipelined)
    batch_pipelined = property(lambda self: self.plans[0].batch_pipelined)
    pair_visits = property(lambda self: all(plan.pair_visits for plan in self.plans))

    def sync_status(self):
        err = None
        for plan in self.plans:          # (every plan's error word is read and cleared; the first error is the one raised)
            try:
                plan.sync_status()
            except NativeError as e:
                err = err or e
        if err is not None:
            raise err

    def inject_sync_error(self):
        self.plans[-1].inject_sync_error()

    def profile_steps(self, *args, **kwargs):
        raise NotImplementedError("profile_steps measures the per-layer launch path of ONE plan")

    def last_logits(self, batch: int, target: int = 0) -> torch.Tensor:
        return torch.cat([plan.last_logits(b - a, target) for plan, a, b in self._slices(batch)], dim=0)


def make_wavenet_plan(describe, batch: int, device) -> "WaveNetPlan":
    """``describe(max_batch)`` -> :class:`WaveNetConfig`.  One plan for the batch, unless the batch is beyond what one launch of the
    stage pipeline takes and the network is one that kernel runs: then evenly sized slices - of at most ``BPIPE_MAX_CLIPS`` clips where
    the plan takes the large-batch form (groups of 16 clips), else of at most ``SPIPE_MAX_CLIPS``."""
    batch = max(int(batch), 1)
    if batch > SPIPE_MAX_CLIPS:
        n = -(-batch // BPIPE_MAX_CLIPS)
        size = -(-batch // n)
        first = WaveNetPlan(describe(size), device)
        if first.batch_pipelined:
            if n == 1:
                return first
            assert max(int(first.cfg.n_targets), 1) == 1, "a plan set slices clips along dimension 0: one target only"
            sizes = [size] * (n - 1) + [batch - size * (n - 1)]
            return WaveNetPlanSet([first] + [WaveNetPlan(describe(sz), device) for sz in sizes[1:]], sizes)
        del first
        n = -(-batch // SPIPE_MAX_CLIPS)
        size = -(-batch // n)
        first = WaveNetPlan(describe(size), device)
        if first.stage_pipelined:
            # (the set slices clips along dimension 0 of every per-clip tensor; with several targets the uniforms are (targets, clips, steps))
            assert max(int(first.cfg.n_targets), 1) == 1, "a plan set slices clips along dimension 0: one target only"
            sizes = [size] * (n - 1) + [batch - size * (n - 1)]
            return WaveNetPlanSet([first] + [WaveNetPlan(describe(sz), device) for sz in sizes[1:]], sizes)
    return WaveNetPlan(describe(batch), device)


class SrnnPlan(_Plan):
    _prefix = "mmk_srnn"
    _has_sync_status = True

    def reset(self):
        check(self._lib.mmk_srnn_reset(self.handle, stream_ptr(self.device)), "mmk_srnn_reset")

    def _streams(self, idx):
        """one (batch, T) int64 tensor per input of the network (a single tensor: the network's only input)"""
        idx = (idx,) if isinstance(idx, torch.Tensor) else tuple(idx)
        n_in = max(int(self.cfg.n_inputs), 1)
        if len(idx) != n_in:
            raise ValueError(f"expected {n_in} input streams, got {len(idx)}")
        require_device(*idx)
        for x in idx:
            if x.dtype != torch.int64 or x.dim() != 2 or x.stride(1) != 1 or x.shape != idx[0].shape:
                raise ValueError("SampleRNN inputs must be int64 (batch, T) of one shape, contiguous along time")
        return idx

    def warmup(self, idx, prompt_len: int):
        """idx: (batch, >= prompt_len) prompt, column 0 = time 0 (a tuple of them for a network of several inputs)"""
        idx = self._streams(idx)
        if idx[0].shape[1] < prompt_len:
            raise ValueError(f"prompt tensor holds {idx[0].shape[1]} steps, prompt_len={prompt_len}")
        ptrs = (vp * len(idx))(*[ptr(x) for x in idx])
        strides = (i64 * len(idx))(*[x.stride(0) for x in idx])
        check(self._lib.mmk_srnn_warmup_multi(self.handle, idx[0].shape[0], ptrs, strides, prompt_len,
                                              stream_ptr(self.device)), "mmk_srnn_warmup_multi")

    def generate(self, idx, t0: int, n_steps: int, temperature=None, uniforms=None, t_first: int = 0):
        """idx: (batch, T) tensor or view whose column 0 is absolute time t_first (a tuple of them for several inputs: the class of
        target k is written into idx[k]); uniforms: (batch, n_steps), (n_targets, batch, n_steps) with several targets"""
        idx = self._streams(idx)
        require_device(temperature, uniforms)
        self._check_uniforms(uniforms, idx[0].shape[0], n_steps)
        ptrs = (vp * len(idx))(*[abs_ptr(x, t_first) for x in idx])
        strides = (i64 * len(idx))(*[x.stride(0) for x in idx])
        check(self._lib.mmk_srnn_generate_multi(self.handle, idx[0].shape[0], ptrs, strides, t0, n_steps,
                                                ptr(temperature), ptr(uniforms), stream_ptr(self.device)),
              "mmk_srnn_generate_multi")

    def resident_blocks(self) -> int:
        """generate blocks run in resident mode so far (diagnostic, see include/mmk.h)"""
        return int(self._lib.mmk_srnn_resident_blocks(self.handle))

    def resident_warmups(self) -> int:
        """warm-ups run as one teacher-forced resident launch so far (diagnostic, see include/mmk.h)"""
        return int(self._lib.mmk_srnn_resident_warmups(self.handle))

    def bottom_kernel(self) -> int:
        """what the most recent bottom-tier steps outside resident mode were emitted as: 0 nothing yet, 1 the fused kernel with one clip per
        workgroup, 2 the fused kernel with four clips per workgroup, 3 one launch per op (diagnostic, see include/mmk.h)"""
        return int(self._lib.mmk_srnn_bottom_kernel(self.handle))

    def last_logits(self, batch: int, target: int = 0) -> torch.Tensor:
        out = torch.empty((batch, self._logit_columns("q_levels", target)), dtype=torch.float32, device=self.device)
        check(self._lib.mmk_srnn_last_logits_of(self.handle, target, batch, ptr(out), out.stride(0), stream_ptr(self.device)),
              "mmk_srnn_last_logits_of")
        return out


class S2SPlan(_Plan):
    _prefix = "mmk_s2s"
    _has_sync_status = True

    def step(self, x: torch.Tensor) -> torch.Tensor:
        require_device(x)
        if x.dtype != torch.float32 or x.stride(2) != 1:
            raise ValueError("Seq2Seq input must be fp32 (batch, hop, n_bins) with unit stride on the last dim")
        y = torch.empty((x.shape[0], self.cfg.hop, self.cfg.out_dim), dtype=torch.float32, device=x.device)
        check(self._lib.mmk_s2s_step(self.handle, x.shape[0], ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0),
                                     y.stride(1), stream_ptr(self.device)), "mmk_s2s_step")
        return y

    def generate(self, frames: torch.Tensor, t0: int, n_steps: int):
        require_device(frames)
        if frames.dtype != torch.float32 or frames.stride(2) != 1:
            raise ValueError("Seq2Seq frames must be fp32 (batch, T, n_bins) with unit stride on the last dim")
        check(self._lib.mmk_s2s_generate(self.handle, frames.shape[0], ptr(frames), frames.stride(0), frames.stride(1),
                                         t0, n_steps, frames.shape[1], stream_ptr(self.device)), "mmk_s2s_generate")

    # -- class indices in and out (embedding input + MLP head, IOSpec.mulaw_io) --------------------------------
    def step_classes(self, x: torch.Tensor) -> torch.Tensor:
        require_device(x)
        if x.dtype != torch.int64 or x.dim() != 2:
            raise ValueError("Seq2Seq class input must be int64 (batch, hop)")
        y = torch.empty((x.shape[0], self.cfg.hop), dtype=torch.int64, device=x.device)
        check(self._lib.mmk_s2s_step_classes(self.handle, x.shape[0], ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0),
                                             y.stride(1), stream_ptr(self.device)), "mmk_s2s_step_classes")
        return y

    def generate_classes(self, classes: torch.Tensor, t0: int, n_steps: int):
        require_device(classes)
        if classes.dtype != torch.int64 or classes.dim() != 2:
            raise ValueError("Seq2Seq classes must be int64 (batch, T)")
        check(self._lib.mmk_s2s_generate_classes(self.handle, classes.shape[0], ptr(classes), classes.stride(0), classes.stride(1),
                                                 t0, n_steps, classes.shape[1], stream_ptr(self.device)), "mmk_s2s_generate_classes")

    def resident_launches(self) -> int:
        """bi-LSTM layers run as one resident launch so far (diagnostic, see include/mmk.h)"""
        return int(self._lib.mmk_s2s_resident_launches(self.handle))

    def last_logits(self, batch: int) -> torch.Tensor:
        """the MLP head's raw outputs of the last step, (batch, hop, out_dim + learn_temp)"""
        n = self.cfg.out_dim + (1 if self.cfg.learn_temp else 0)
        out = torch.empty((batch, self.cfg.hop, n), dtype=torch.float32, device=self.device)
        check(self._lib.mmk_s2s_last_logits(self.handle, batch, ptr(out), n, stream_ptr(self.device)), "mmk_s2s_last_logits")
        return out


class TransformerPlan(_Plan):
    """SimpleTransformer (csrc/transformer_plan.hip): the state_dict is bound by the reference's key names, ``pe.pe`` as stored.
    Class tensors are int64 (batch, T) with unit stride along time; frame tensors fp32 (batch, T, n_bins) with unit stride along the bins."""
    _prefix = "mmk_tr"

    def _check(self, x: torch.Tensor, what: str):
        require_device(x)
        if self.cfg.in_kind == 0:
            if x.dtype != torch.int64 or x.dim() != 2 or x.stride(1) != 1:
                raise ValueError(f"{what} must be int64 class indices (batch, T) with unit stride along time")
        elif x.dtype != torch.float32 or x.dim() != 3 or x.stride(2) != 1 or x.shape[2] != self.cfg.in_dim:
            raise ValueError(f"{what} must be fp32 frames (batch, T, {self.cfg.in_dim}) with unit stride along the bins")

    def _sampling(self, batch: int, n: int, temperature, uniforms):
        require_device(temperature, uniforms)
        if temperature is None:
            return None, None
        if temperature.dtype != torch.float32 or not temperature.is_contiguous() or temperature.numel() != batch:
            raise ValueError("temperature must be contiguous fp32, one per clip")
        if uniforms is None or uniforms.dtype != torch.float32 or not uniforms.is_contiguous() or uniforms.numel() != batch * n:
            raise ValueError(f"uniforms must be contiguous fp32 of shape ({batch}, {n})")
        return ptr(temperature), ptr(uniforms)

    def step(self, x: torch.Tensor, temperature: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: the (batch, rf[, n_bins]) window -> (batch,) classes or (batch, n_bins) frames of the position after it"""
        self._check(x, "the window")
        if x.shape[1] != self.cfg.rf:
            raise ValueError(f"the window holds {x.shape[1]} positions, rf is {self.cfg.rf}")
        batch = x.shape[0]
        if self.cfg.in_kind == 0:
            y = torch.empty(batch, dtype=torch.int64, device=x.device)
        else:
            y = torch.empty((batch, self.cfg.out_dim), dtype=torch.float32, device=x.device)
        tp, up = self._sampling(batch, 1, temperature, uniforms)
        check(self._lib.mmk_tr_step(self.handle, batch, ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0), tp, up,
                                    stream_ptr(self.device)), "mmk_tr_step")
        return y

    def generate(self, data: torch.Tensor, t0: int, n_steps: int, temperature: Optional[torch.Tensor] = None,
                 uniforms: Optional[torch.Tensor] = None):
        """steps t0 .. t0 + n_steps - 1 in place on the loop's tensor; uniforms (batch, n_steps)"""
        self._check(data, "the generated tensor")
        if t0 < self.cfg.rf or n_steps < 0 or t0 + n_steps > data.shape[1]:
            raise ValueError(f"steps [{t0}, {t0 + n_steps}) need rf={self.cfg.rf} positions before them and must lie in the tensor's {data.shape[1]}")
        tp, up = self._sampling(data.shape[0], n_steps, temperature, uniforms)
        check(self._lib.mmk_tr_generate(self.handle, data.shape[0], ptr(data), data.stride(0), data.stride(1), t0, n_steps, tp, up,
                                        stream_ptr(self.device)), "mmk_tr_generate")

    def last_logits(self, batch: int) -> torch.Tensor:
        """the MLP head's raw outputs of the last step, (batch, out_dim + learn_temp)"""
        n = self.cfg.out_dim + (1 if self.cfg.learn_temp else 0)
        out = torch.empty((batch, n), dtype=torch.float32, device=self.device)
        check(self._lib.mmk_tr_last_logits(self.handle, batch, ptr(out), n, stream_ptr(self.device)), "mmk_tr_last_logits")
        return out
