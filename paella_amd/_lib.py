"""ctypes binding of libpaella_hip.so (C ABI declared in include/paella_hip.h).

No torch types cross this boundary: tensors are passed as raw device pointers (tensor.data_ptr()) plus sizes,
the current torch HIP stream as a void*.  The library is built in-tree by paella_amd/build.py; there is no
fallback -- if it is missing or fails to load, every product entry point raises.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpaella_hip.so")

MAX_LEVELS = 8
MAX_BLOCK_TYPES = 8
ABI_VERSION = 8


class UnetConfig(Structure):
    _fields_ = [
        ("c_in", c_int32), ("c_out", c_int32), ("num_labels", c_int32), ("c_r", c_int32), ("patch_size", c_int32),
        ("c_cond", c_int32), ("n_levels", c_int32),
        ("c_hidden", c_int32 * MAX_LEVELS), ("nhead", c_int32 * MAX_LEVELS), ("blocks", c_int32 * MAX_LEVELS),
        ("level_config", (c_char * MAX_BLOCK_TYPES) * MAX_LEVELS),
        ("clip_embd", c_int32), ("byt5_embd", c_int32), ("clip_seq_len", c_int32), ("kernel_size", c_int32),
        ("self_attn", c_int32),
    ]


class VqganConfig(Structure):
    _fields_ = [
        ("levels", c_int32), ("bottleneck_blocks", c_int32), ("c_hidden", c_int32), ("c_latent", c_int32),
        ("codebook_size", c_int32), ("scale_factor", c_float),
    ]


class TestGemmArgs(Structure):
    """paella_amd/csrc/test_hooks.h: paella_test_gemm_args (one fp32 GEMM launch, field by field; tests / tools only)."""
    _fields_ = [
        ("A", c_void_p), ("lda", c_int), ("W", c_void_p), ("ldw", c_int), ("C", c_void_p), ("ldc", c_int),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("bias", c_void_p), ("act", c_int), ("alpha", c_float), ("residual", c_void_p), ("ldr", c_int),
        ("ts", c_void_p), ("ts_stride", c_int), ("rows_per_sample", c_int),
        ("store_mode", c_int), ("sH", c_int), ("sW", c_int), ("sC", c_int), ("py", c_int), ("px", c_int), ("n_seg_x", c_int),
        ("rowstat_out", c_void_p), ("sumsq_out", c_void_p),
        ("remap_in", c_int), ("remap_out", c_int), ("remap_off", c_int),
        ("c16", c_void_p),
        ("mode", c_int), ("scale", c_void_p), ("shift", c_void_p), ("a_rows_per_sample", c_int), ("ln_stats", c_void_p),
        ("cv_enabled", c_int), ("cv_Hi", c_int), ("cv_Wi", c_int), ("cv_C", c_int), ("cv_Ho", c_int), ("cv_Wo", c_int), ("cv_stride", c_int),
        ("cv_ntaps", c_int), ("cv_tw_log2", c_int), ("cv_oy0", c_int), ("cv_ox0", c_int), ("cv_tsign", c_int),
        ("c_capacity", c_size_t), ("c16_capacity", c_size_t), ("rowstat_capacity", c_size_t), ("sumsq_capacity", c_size_t),
    ]


class TailArgs(Structure):
    """include/paella_hip.h: paella_tail_args -- everything a sampling tail can take; zero / None = not given, the form follows from what is present"""
    _fields_ = [
        ("logits_c", c_void_p), ("logits_u", c_void_p), ("rows", c_int64), ("L", c_int32),
        ("cfg", c_float), ("one_minus_cfg", c_float), ("temperature", c_float), ("mode", c_int32), ("seed", c_uint64), ("seed_ptr", c_void_p), ("offset", c_uint64),
        ("row_offset", c_int64), ("row_offset_ptr", c_void_p), ("t_next", c_float), ("noise_q", c_void_p), ("mask_u", c_void_p),
        ("seeds", c_void_p), ("temperature_tab", c_void_p), ("cfg_pairs", c_void_p), ("rows_per_sample", c_int32),
        ("step", c_void_p), ("t_next_tab", c_void_p), ("active", c_void_p),
        ("init_noise", c_void_p), ("pin_keep", c_void_p), ("pin_tokens", c_void_p), ("pin_on", c_void_p),
        ("top_k", c_int32), ("top_p", c_float), ("typical_mass", c_float), ("min_tokens", c_int32), ("filter_k", c_void_p), ("filter_mass", c_void_p),
        ("tokens_out", c_void_p), ("sampled_out", c_void_p), ("logprob_out", c_void_p), ("entropy_out", c_void_p),
    ]


class StepArgs(Structure):
    """include/paella_hip.h: paella_step_args -- one forward; tail = None: logits to logits_out, otherwise the fused step"""
    _fields_ = [
        ("tokens", c_void_p), ("r", c_void_p), ("cond", c_void_p), ("B", c_int32), ("n_unique", c_int32), ("mix_c", c_float), ("mix_u", c_float), ("mix_pairs", c_void_p),
        ("H", c_int32), ("W", c_int32), ("S", c_int32), ("cond_len", c_void_p),
        ("attn_weights", c_void_p), ("n_attn_weights", c_int32),
        ("kw_table", c_void_p), ("kw_len", c_void_p), ("kw_pitch", c_int32),
        ("q_groups", c_void_p), ("qg_pitch", c_int32), ("k_groups", c_void_p), ("kg_pitch", c_int32),
        ("logits_out", c_void_p), ("tail", POINTER(TailArgs)),
    ]


class AdamwTensor(Structure):
    """include/paella_hip.h: paella_adamw_tensor -- one row of the optimizer step's table (88 bytes, every field 8 wide: train_ops.ADAMW_ROW is the same layout in numpy)"""
    _fields_ = [
        ("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n", c_int64), ("chunk_begin", c_int64),
        ("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
    ]


def tensor_fields(block, **tensors):
    """set pointer fields of an argument block from tensors (None = not given)"""
    for name, t in tensors.items():
        setattr(block, name, None if t is None else t.data_ptr())
    return block


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
SIGNATURES = {
    "paella_abi_version": (c_int, []),
    "paella_last_error": (c_char_p, []),
    "paella_source_stamp": (c_char_p, []),
    "paella_workspace_init": (c_int, [c_void_p, c_size_t, c_void_p]),
    "paella_workspace_header_bytes": (c_size_t, []),
    "paella_unet_create": (c_int, [POINTER(UnetConfig), POINTER(c_void_p)]),
    "paella_unet_destroy": (None, [c_void_p]),
    "paella_unet_load_tensor": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int, c_void_p]),
    "paella_unet_set_timestep_freqs": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "paella_unet_finalize": (c_int, [c_void_p, c_void_p]),
    "paella_unet_cond_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "paella_unet_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int, c_int]),
    "paella_unet_cond_prepare": (c_int, [c_void_p, c_void_p, c_int, c_void_p, POINTER(c_void_p), c_int, c_int, c_void_p,
                                         c_size_t, c_void_p, c_size_t, c_void_p]),
    "paella_unet_c_embeddings": (c_int, [c_void_p, c_void_p, c_int, c_void_p, POINTER(c_void_p), c_int, c_int, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
    "paella_unet_r_embedding": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "paella_unet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_shared": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_int,
                                           c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_int,
                                           c_void_p, c_int, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p, c_float, c_void_p,
                                           c_void_p, c_size_t, c_void_p]),
    "paella_sample_tail": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_void_p,
                                   c_uint64, c_uint64, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "paella_sample_tail_ex": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_void_p,
                                      c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "paella_start_tokens": (c_int, [c_uint64, c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "paella_sample_tail_req": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_uint64, c_void_p, c_float, c_void_p, c_void_p,
                                       c_void_p]),
    "paella_start_tokens_req": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "paella_unet_forward_shared_req": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                               c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_req": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                               c_void_p, c_int, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_request_step": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_sample_tail_stream": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "paella_unet_forward_sample_stream": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                                  c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_add_noise": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_int, c_int,
                                 c_int64, c_void_p, c_void_p, c_void_p]),
    "paella_select_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "paella_vqgan_create": (c_int, [POINTER(VqganConfig), POINTER(c_void_p)]),
    "paella_vqgan_destroy": (None, [c_void_p]),
    "paella_vqgan_load_tensor": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int, c_void_p]),
    "paella_vqgan_finalize": (c_int, [c_void_p, c_void_p]),
    "paella_vqgan_set_precision": (c_int, [c_void_p, c_int, c_void_p]),
    "paella_vqgan_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "paella_vqgan_decode_indices": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_vqgan_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_vqgan_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "paella_vqgan_quantize_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_vqgan_lookup_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "paella_unet_set_precision": (c_int, [c_void_p, c_int, c_void_p]),
    "paella_unet_get_precision": (c_int, [c_void_p]),
    "paella_op_gemm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_void_p, c_size_t, c_void_p]),
    "paella_op_layernorm": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "paella_op_dwconv_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                    c_void_p]),
    "paella_op_grn_scale": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "paella_op_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_void_p, c_int, c_void_p]),
    # ragged conditioning (ABI 8): `cond_len` (int32 device table) right after S / Lcond
    "paella_unet_cond_prepare_slots": (c_int, [c_void_p, c_void_p, c_int, c_void_p, POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p,
                                               c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_shared_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_void_p,
                                                  c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_void_p,
                                                  c_void_p, c_int, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p, c_float, c_void_p,
                                                  c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_shared_req_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_req_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                                      c_void_p, c_void_p, c_int, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_stream_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                                         c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                                         c_void_p]),
    "paella_op_attention_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                           c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    # editing requests (ABI 8, additive): the pin tables `pin_keep`, `pin_tokens` (and `pin_on` in the stream forms) right before the outputs
    "paella_request_step_pin": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "paella_sample_tail_pin": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p,
                                       c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_sample_tail_stream_pin": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_unet_forward_sample_pin": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_void_p,
                                               c_void_p, c_int, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_stream_pin": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                                      c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_size_t, c_void_p]),
    # per-request prompt weights (ABI 8, additive): the key-weight table (kw_table, kw_len, kw_pitch) in place of (attn_weights, n_attn_weights)
    "paella_op_attention_kw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "paella_unet_forward_shared_req_kw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_req_kw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_int, c_void_p, c_void_p, c_int, c_uint64, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_size_t, c_void_p]),
    "paella_unet_forward_sample_stream_kw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                     c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_size_t, c_void_p]),
    # regional prompts (ABI 8, additive): the key-group tables (q_groups, qg_pitch, k_groups, kg_pitch) right after the key-weight table
    "paella_op_attention_rg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "paella_unet_forward_shared_req_rg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                  c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_unet_forward_sample_stream_rg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                     c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # truncated sampling (ABI 8, additive): the filter values / tables right before the outputs
    "paella_sample_tail_filter": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p,
                                          c_float, c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "paella_sample_tail_stream_filter": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # confidence-ordered renoise (ABI 8, additive): the _filter tails plus (logprob_out, entropy_out) before the stream, and the renoise stage in both forms
    "paella_sample_tail_stats": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_void_p,
                                         c_float, c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_sample_tail_stream_stats": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # the argument blocks (ABI 8, additive): one forward, one sampling tail; every forward_shared* / forward_sample* / sample_tail* above is a fixed form of these
    "paella_unet_step": (c_int, [c_void_p, POINTER(StepArgs), c_size_t, c_void_p, c_size_t, c_void_p]),
    "paella_sample_tail_args": (c_int, [POINTER(TailArgs), c_size_t, c_void_p]),
    "paella_renoise_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_uint64, c_void_p, c_uint64, c_int64, c_void_p, c_float, c_int, c_float, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "paella_renoise_select_stream": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p]),
    # training loss head (ABI 8, additive): classifier + label-smoothed cross-entropy, forward and backward, no logits tensor
    "paella_head_loss_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "paella_head_loss_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_head_loss_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    # training MLP activation (ABI 8, additive): GELU -> GlobalResponseNorm -> dropout, forward and backward, only u and G [B, C] kept
    "paella_grn_act_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "paella_grn_act_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_uint64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_grn_act_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    # training ResBlock front (ABI 8, additive): depthwise 3x3 (+ skip read in place) + LayerNorm, forward and backward, only rstd [B H W] kept besides y
    "paella_dwconv_ln_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "paella_dwconv_ln_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_dwconv_ln_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    # training attention (ABI 8, additive): softmax(q k^T) v with dropout, forward and backward, only lse [B, nhead, P] kept besides o
    "paella_attn_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "paella_attn_train_forward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_uint64, c_void_p, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "paella_attn_train_backward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                           c_uint64, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    # training timestep modulation (ABI 8, additive): residual add + TimestepBlock [+ LayerNorm], forward and backward, only rstd [B, P] kept besides z
    "paella_mod_ln_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "paella_mod_ln_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_mod_ln_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                             c_size_t, c_void_p]),
    # training optimizer step (ABI 8, additive): global gradient norm + clip coefficient + AdamW over a device table of tensors (AdamwTensor rows), three launches
    "paella_adamw_chunk_elems": (c_int, []),
    "paella_adamw_workspace_bytes": (c_size_t, [c_int, c_int64]),
    "paella_adamw_grad_norm": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_adamw_step": (c_int, [c_void_p, c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # training linear on bf16 operands (ABI 8, additive): the pack (fp32 -> bf16 row-major / transposed / column sums) and forward, dgrad + wgrad + db over it
    "paella_linear_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "paella_linear_train_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_linear_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_pack_bf16": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # training seed table (ABI 8, additive): the dropout seeds of a forward as device words, one launch per iteration; and the two dropout ops with the seed read
    # from such a word (seed_dev in the place of seed) -- what a captured training iteration needs to draw other masks at every replay
    "paella_train_seeds_max_sites": (c_int, []),
    "paella_train_seeds_advance": (c_int, [c_void_p, c_int, c_void_p]),
    "paella_grn_act_forward_seed_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_grn_act_backward_seed_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_size_t, c_void_p]),
    "paella_attn_train_forward_seed_dev": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_attn_train_backward_seed_dev": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                    c_float, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    # training token stem (ABI 8, additive): embedding + LayerNorm + PixelUnshuffle, the forward by the eval engine's launch, the table's gradient in one launch
    "paella_embed_ln_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "paella_embed_ln_train_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "paella_embed_ln_train_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
}

# exported for tests / tools only; declared in paella_amd/csrc/test_hooks.h, not in the public header
TEST_HOOKS = {
    "paella_prof_detail": (c_int64, [c_void_p, c_void_p, c_int64]),
    "paella_prof_epi": (c_int64, [c_void_p, c_int64]),
    "paella_prof_grid": (c_int64, [c_void_p, c_int64]),
    "paella_prof_enable": (c_int, [c_int]),
    "paella_prof_collect": (c_int, [POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_int64)]),
    "paella_test_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_test_gemm_bf16_rule": (c_int, [c_int]),
    "paella_test_grn_apply16": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "paella_test_gemm_bf16_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_test_attention_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "paella_test_attention_bf16_ragged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                                  c_void_p, c_int, c_void_p]),
    "paella_test_attention_bf16_kw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                              c_void_p, c_void_p, c_int, c_void_p]),
    "paella_test_launch_chain": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "paella_test_attention_variant": (c_int, [c_int]),
    "paella_test_gemm_dma": (c_int, [c_int]),
    "paella_test_gemm_epi_specialise": (c_int, [c_int]),
    "paella_test_gemm_raster": (c_int, [c_int]),
    "paella_test_gemm_ring": (c_int, [c_int]),
    "paella_test_ring_resident": (ctypes.c_long, [c_int, c_int]),
    "paella_test_gemm_site": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "paella_test_gemm_site_cfg": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "paella_test_gemm_big_stagger": (c_int, [c_int]),
    "paella_test_grn_fuse": (c_int, [c_int]),
    "paella_test_ln_fold_ratio": (c_int, [c_float]),
    "paella_test_ln_guard_counter": (c_int, [c_void_p]),
    "paella_test_mlp_grn_fused": (c_int, [c_void_p] * 10 + [c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_test_gemm_tail_tile": (c_int, [c_int]),
    "paella_test_tail_scores": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_uint64, c_uint64, c_int64, c_void_p, c_void_p]),
    "paella_test_tail_scores_req": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_uint64, c_void_p, c_void_p]),
    "paella_test_tail_filter_keep": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_float, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_test_renoise_scores": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_uint64, c_uint64, c_int64, c_float, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "paella_test_gemm_prologue": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                          c_void_p, c_size_t, c_void_p]),
    "paella_test_gemm_desc": (c_int, [POINTER(TestGemmArgs), c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "paella_test_gemm_args_size": (c_size_t, []),
    "paella_test_embed_ln_unshuffle": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
}

_lib = None


class PaellaHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once). Raises PaellaHipError when it is absent -- there is no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PaellaHipError(
            "libpaella_hip.so is not built (%s). Run `python -m paella_amd.build` (needs hipcc); "
            "paella_amd has no non-HIP fallback." % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise PaellaHipError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in list(SIGNATURES.items()) + list(TEST_HOOKS.items()):
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch, let it propagate loudly
        fn.restype = res
        fn.argtypes = args
    from ._stamp import source_stamp
    try:
        here = source_stamp()
    except OSError as e:  # the kernel sources ship next to the library; without them its provenance cannot be checked
        raise PaellaHipError("cannot verify %s: the kernel sources it is checked against are missing (%s)" % (LIB_PATH, e)) from e
    built = lib.paella_source_stamp().decode()
    if built != here:
        raise PaellaHipError("libpaella_hip.so was built from other sources (library stamp %s, sources in the tree %s): rebuild with "
                             "`python -m paella_amd.build`; a stale library is never used silently" % (built, here))
    if lib.paella_abi_version() != ABI_VERSION:
        raise PaellaHipError("libpaella_hip.so ABI %d != binding ABI %d" % (lib.paella_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().paella_last_error()
        raise PaellaHipError("libpaella_hip error %d: %s" % (rc, msg.decode("utf-8", "replace") if msg else "?"))


def ptr(t):
    """Device/host pointer of a tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def new_workspace(nbytes, device):
    """A caller-owned workspace with its ticket header initialised (include/paella_hip.h: paella_workspace_init)."""
    import torch
    lib = load()
    nbytes = max(int(nbytes), int(lib.paella_workspace_header_bytes()))
    with torch.cuda.device(device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(lib.paella_workspace_init(ptr(ws), ws.numel(), stream_ptr(device)))
    return ws


def stream_ptr(device=None):
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)
