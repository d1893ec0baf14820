"""ctypes binding of libezaudio_hip.so (include/ezdit.h).

There is NO fallback: if the HIP library is missing or does not export the ABI this module raises,
so a GPU box can never silently run a non-native path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libezaudio_hip.so')
ABI_VERSION = 4


class EzditConfig(C.Structure):
    _fields_ = [('embed_dim', C.c_int32), ('num_heads', C.c_int32), ('depth', C.c_int32),
                ('in_chans', C.c_int32), ('out_chans', C.c_int32), ('context_dim', C.c_int32),
                ('ada_sola_rank', C.c_int32), ('ada_sola_alpha', C.c_float), ('mlp_ratio', C.c_float),
                ('max_len', C.c_int32), ('controlnet', C.c_int32), ('cond_in', C.c_int32), ('cond_c0', C.c_int32),
                ('cond_c1', C.c_int32), ('cond_mask', C.c_int32)]


class EzditParamInfo(C.Structure):
    _fields_ = [('name', C.c_char * 64), ('src', (C.c_char * 96) * 3), ('nsrc', C.c_int32),
                ('dtype', C.c_int32), ('transform', C.c_int32),
                ('rows', C.c_int64), ('cols', C.c_int64), ('rows_pad', C.c_int64), ('ld', C.c_int64),
                ('offset', C.c_int64)]


class EzditDdimCoef(C.Structure):
    _fields_ = [('sa', C.c_float), ('sb', C.c_float), ('c_x0', C.c_float), ('c_dir', C.c_float),
                ('sigma', C.c_float)]


class EzditTestRowArgs(C.Structure):
    """ezdit_test_row_args (include/ezdit.h): the fields of the row operator's argument struct (csrc/common.h RowArgs) and the slot count of its tables."""
    _fields_ = [('h_in', C.c_void_p), ('h_out', C.c_void_p),
                ('part', C.c_void_p), ('nsplit', C.c_int32), ('ld_part', C.c_int32), ('part_stride', C.c_int64), ('part_bf16', C.c_int32), ('mode', C.c_int32),
                ('bias', C.c_void_p), ('gate', C.c_void_p), ('gate_slot_stride', C.c_int64),
                ('ln_g', C.c_void_p), ('ln_c', C.c_void_p), ('ln_slot_stride', C.c_int64),
                ('skip', C.c_void_p), ('cn', C.c_void_p), ('cn_tab', C.c_void_p), ('cn_scale', C.c_float), ('ld_u', C.c_int32),
                ('u', C.c_void_p),
                ('M', C.c_int32), ('D', C.c_int32), ('L', C.c_int32), ('n_slots', C.c_int32),
                ('cur_step', C.c_void_p), ('row_slot', C.c_void_p),
                ('wt', C.c_int32), ('variant', C.c_int32), ('affine', C.c_int32), ('reserved', C.c_int32)]


P_F32, P_BF16 = 0, 1
T_NONE, T_GEGLU8, T_QKROPE = 0, 1, 2

# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
PROTOTYPES = {
    'ezdit_abi_version': (C.c_int, []),
    'ezdit_last_error': (C.c_char_p, []),
    'ezdit_create': (C.c_int, [C.POINTER(EzditConfig), C.POINTER(C.c_void_p)]),
    'ezdit_destroy': (C.c_int, [C.c_void_p]),
    'ezdit_param_count': (C.c_int, [C.c_void_p]),
    'ezdit_param_info': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EzditParamInfo)]),
    'ezdit_param_bytes': (C.c_size_t, [C.c_void_p]),
    'ezdit_bind_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'ezdit_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    'ezdit_bind_workspace': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_prepare_context': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ezdit_prepare_timesteps': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p]),
    'ezdit_set_step': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'ezdit_set_lengths': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    'ezdit_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]),
    'ezdit_prepare_condition': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'ezdit_controlnet_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ezdit_controlnet_residuals': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]),
    'ezdit_sampler_attach_controlnet': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float]),
    'ezdit_set_cn_scale': (C.c_int, [C.c_void_p, C.c_float]),
    'ezdit_sampler_set_pair_lengths': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    'ezdit_sampler_set_cn_scales': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_sampler_begin': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(EzditDdimCoef), C.c_int,
                                      C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ezdit_sampler_begin_composed': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(EzditDdimCoef), C.c_int,
                                               C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    'ezdit_sampler_set_compose_weights': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]),
    'ezdit_cfg_compose_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p]),
    'ezdit_sampler_set_apg': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int,
                                        C.c_void_p, C.c_void_p]),
    'ezdit_cfg_apg_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p]),
    'ezdit_sampler_run': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_cfg_ddim_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    'ezdit_sampler_set_sample_params': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(EzditDdimCoef), C.c_int,
                                                  C.c_void_p]),
    'ezdit_cfg_ddim_step_per_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p]),
    'ezdit_sampler_set_multistep': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]),
    'ezdit_cfg_multistep_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p]),
    'ezdit_add_noise': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_sampler_set_start': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    'ezdit_canvas_blend': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_sampler_set_canvas': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_canvas_blend_loop': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_sampler_set_canvas_loop': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezvae_gemm': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    'ezvae_snake_bf16': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p]),
    'ezvae_conv_out1': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p]),
    'ezvae_conv_in1': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p]),
    'ezvae_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezvae_snake_bf16_seg': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_void_p, C.c_int,
                                       C.c_long, C.c_long, C.c_long, C.c_long, C.c_void_p]),
    'ezvae_conv_out1_seg': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_long,
                                      C.c_void_p]),
    'ezvae_conv_in1_seg': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p]),
    'ezvae_sample_seg': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_long, C.c_void_p]),
    'ezdit_test_gemm': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_debug_gemm_timestamps': (C.c_int, [C.c_void_p, C.c_long]),
    'ezdit_test_resid': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_resid_skip': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    'ezdit_test_resid_dual': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_consumer': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_rope_table': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_cross_attention': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                             C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_attention': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_attention_varlen': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'ezdit_test_final_conv': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    'ezdit_test_row': (C.c_int, [C.POINTER(EzditTestRowArgs), C.c_void_p]),
    'ezdit_test_headnorm': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezdit_test_assemble': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    'ezdit_debug_buffer': (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    'ezdit_last_launch_count': (C.c_int, [C.c_void_p]),
    'ezdit_debug_stop_after': (C.c_int, [C.c_void_p, C.c_int]),
    'ezdit_set_option': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    'ezdit_set_attention_window': (C.c_int, [C.c_void_p, C.c_int]),
    'ezdit_test_attention_band': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p]),
    'ezdit_set_context_weights': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_test_attention_timeline': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_test_cross_attention_timeline': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                                      C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_set_context_token_weights': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_test_attention_keyweights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    'ezdit_test_cross_attention_keyweights': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.c_int, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                                        C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
}


class Ezt5Config(C.Structure):
    _fields_ = [('vocab', C.c_int32), ('d_model', C.c_int32), ('d_kv', C.c_int32), ('num_heads', C.c_int32), ('d_ff', C.c_int32),
                ('num_layers', C.c_int32), ('num_buckets', C.c_int32), ('max_distance', C.c_int32), ('eps', C.c_float),
                ('max_len', C.c_int32), ('ff_act', C.c_int32)]


class Ezt5TensorInfo(C.Structure):
    _fields_ = [('name', C.c_char * 32), ('dtype', C.c_int32), ('reserved', C.c_int32), ('rows', C.c_int64), ('cols', C.c_int64),
                ('offset', C.c_int64)]


FF_GATED_GELU_NEW, FF_RELU, FF_GATED_GELU, FF_OTHER = 0, 1, 2, 3

# the T5 encoder section of the header (ezt5_*), bound by load() like the table above
T5_PROTOTYPES = {
    'ezt5_create': (C.c_int, [C.POINTER(Ezt5Config), C.POINTER(C.c_void_p)]),
    'ezt5_destroy': (C.c_int, [C.c_void_p]),
    'ezt5_tensor_count': (C.c_int, [C.c_void_p]),
    'ezt5_blob_bytes': (C.c_size_t, [C.c_void_p, C.POINTER(Ezt5TensorInfo), C.c_int]),
    'ezt5_bind_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'ezt5_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    'ezt5_bind_workspace': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    'ezt5_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezt5_test_attention': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    'ezt5_test_rms': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezt5_test_attention_ex': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'ezt5_test_embed_rms': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_void_p]),
    'ezt5_test_gated_gelu': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'ezt5_test_gemm': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}

_lib = None


class EzditError(RuntimeError):
    pass


def load():
    """Load the HIP library (raises if it has not been built: run `python -m ezaudio_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime: import it FIRST so that this library binds to the runtime instance torch
    # initialises (loading us first was observed to leave the library with "no ROCm-capable device")
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise EzditError(f'{LIB_PATH} is missing: the HIP extension has not been built '
                         f'(python -m ezaudio_amd.build). There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(PROTOTYPES.items()) + list(T5_PROTOTYPES.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.ezdit_abi_version() != ABI_VERSION:
        raise EzditError(f'ABI version mismatch: library {lib.ezdit_abi_version()} != binding {ABI_VERSION}')
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().ezdit_last_error()
        code = {-1: 'EZDIT_E_INVALID', -2: 'EZDIT_E_UNSUPPORTED', -3: 'EZDIT_E_STATE', -4: 'EZDIT_E_HIP'}.get(rc, str(rc))
        text = f'{code}: {msg.decode() if msg else ""}'
        if rc == -2:
            raise NotImplementedError(text)  # mirrors src/models/udit.py:83,113,127
        if rc == -1:
            raise AssertionError(text)       # shape errors are AssertionError-class in the reference
        raise EzditError(text)
