"""Loads graphflow_amd/csrc/libgf_hip.so (the C-ABI of include/gf_hip.h) and declares its prototypes.

There is NO fallback: if the shared library is missing or a symbol is absent this module raises, and every op in the
package fails with it.  Building happens in-tree (`make -C graphflow_amd/csrc`, driven by __graft_entry__.build()).
"""
import ctypes as C
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("GF_HIP_LIBRARY") or os.path.join(_CSRC, "libgf_hip.so")   # (GF_HIP_LIBRARY: an experimental build, tools/ab_lib.sh)

GF_OK, GF_ERR_INVALID, GF_ERR_HIP, GF_ERR_NOMEM, GF_ERR_UNSUPPORTED, GF_ERR_TIMEOUT = range(6)
GF_OPT_R18_GENERIC_KERNELS = 1
GF_OPT_SMP_FP32_PRODUCTS = 2
GF_DIST_ID_BYTES = 128

_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

SMP_CONFIG_BYTES = 22 * C.sizeof(C.c_int)   # sizeof(gf_smp_config) of include/gf_hip.h (graphflow_amd.smp.SMPConfigCovariant is checked against it)


class ConfigPointer:
    """The `const gf_smp_config *` of a prototype.  gf_smp_config grows at its end, one int per model family, and a zero tail means
    "everything as before"; a caller may still hold a structure of an earlier layout (graphflow_amd.smp.SMPConfig ends at `readout`; a
    test builds its own).  Where the argument says how large the structure behind it is -- a ctypes structure, byref() of one, a typed
    pointer -- and that is less than the library's structure, the library gets a copy with a zero tail instead of reading past the
    caller's.  The library only reads a configuration, so the copy is not seen.  None, an address or a c_void_p pass as they are."""

    @classmethod
    def from_param(cls, obj):
        if obj is None or isinstance(obj, (int, C.c_void_p)):
            return _vp(obj) if isinstance(obj, int) else obj
        src = getattr(obj, "_obj", None)   # byref(x)
        if src is None and isinstance(obj, C._Pointer):
            if not obj:
                return None
            src = obj.contents
        if src is None:
            src = obj
        n = C.sizeof(src)
        if n >= SMP_CONFIG_BYTES:
            return C.cast(C.pointer(src), _vp) if src is obj else obj
        padded = (C.c_char * SMP_CONFIG_BYTES)()
        C.memmove(padded, C.addressof(src), n)
        return C.byref(padded)


_cfgp = ConfigPointer

# name -> (restype, argtypes); mirrors include/gf_hip.h one to one (tests/test_abi.py checks the two agree)
PROTOTYPES = {
    "gf_ctx_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "gf_ctx_use_private_stream": (C.c_int, [_vp]),
    "gf_ctx_destroy": (C.c_int, [_vp]),
    "gf_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "gf_ctx_get_stream": (_vp, [_vp]),
    "gf_ctx_synchronize": (C.c_int, [_vp]),
    "gf_ctx_reserve": (C.c_int, [_vp, C.c_size_t]),
    "gf_ctx_set_timing": (C.c_int, [_vp, C.c_int]),
    "gf_ctx_timing_count": (C.c_int, [_vp]),
    "gf_ctx_timing_get": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "gf_hbm_copy_probe_f32": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "gf_last_error": (C.c_char_p, [_vp]),
    "gf_version": (C.c_char_p, []),
    "gf_ctx_set_option": (C.c_int, [_vp, C.c_int, C.c_int]),
    "gf_dist_unique_id": (C.c_int, [_vp, _vp]),
    "gf_dist_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "gf_dist_finalize": (C.c_int, [_vp]),
    "gf_dist_rank": (C.c_int, [_vp]),
    "gf_dist_world": (C.c_int, [_vp]),
    "gf_dist_allreduce_sum_f32": (C.c_int, [_vp, _vp, C.c_size_t]),
    "gf_dist_broadcast_f32": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int]),
    "gf_dist_quiesce": (C.c_int, [_vp]),
    "gf_contract_forward_f32": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "gf_contract_backward_f32": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "gf_contract_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "gf_contract_forward_host_f64": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), _dp, _dp, C.c_int, C.c_int]),
    "gf_contract_backward_host_f64": (C.c_int, [_vp, C.c_int, _dp, _dp, C.POINTER(_dp), C.c_int, C.c_int]),
    "gf_contract_forward_host_f32": (C.c_int, [_vp, C.c_int, C.POINTER(_fp), _fp, _fp, C.c_int, C.c_int]),
    "gf_contract_backward_host_f32": (C.c_int, [_vp, C.c_int, _fp, _fp, C.POINTER(_fp), C.c_int, C.c_int]),
}

_i = C.c_int
PROTOTYPES.update({
    "gf_contract18_dropout_forward_f32": (_i, [_vp, C.c_uint, C.c_float, _vp, _vp, _vp, _i, _i, _i]),
    "gf_contract18_dropout_backward_f32": (_i, [_vp, C.c_uint, _vp, _vp, _vp, _i, _i, _i, _i]),
    "gf_contract18_dropout_forward_host_f64": (_i, [_vp, C.c_uint, C.c_double, C.POINTER(_dp), _dp, _dp, _i, _i]),
    "gf_contract18_dropout_backward_host_f64": (_i, [_vp, C.c_uint, _dp, _dp, C.POINTER(_dp), _i, _i]),
    "gf_contract18_dropout_forward_host_f32": (_i, [_vp, C.c_uint, C.c_double, C.POINTER(_fp), _fp, _fp, _i, _i]),
    "gf_contract18_dropout_backward_host_f32": (_i, [_vp, C.c_uint, _fp, _fp, C.POINTER(_fp), _i, _i]),
})
for _sfx, _t in (("f64", _dp), ("f32", _fp)):
    PROTOTYPES["gf_matmul_forward_host_" + _sfx] = (_i, [_vp, _t, _t, _t, _i, _i, _i])
    PROTOTYPES["gf_stack_forward_host_" + _sfx] = (_i, [_vp, C.POINTER(_t), _t, _i, C.c_size_t])
    PROTOTYPES["gf_stack_backward_host_" + _sfx] = (_i, [_vp, _t, C.POINTER(_t), _i, C.c_size_t])
    PROTOTYPES["gf_matmul_backward_host_" + _sfx] = (_i, [_vp, _t, _t, _t, _t, _t, _i, _i, _i])
    PROTOTYPES["gf_custommatmultensor_forward_host_" + _sfx] = (_i, [_vp, _t, _t, _t, C.c_longlong, _i, _i])
    PROTOTYPES["gf_custommatmultensor_backward_host_" + _sfx] = (_i, [_vp, _t, _t, _t, _t, _t, C.c_longlong, _i, _i])
    for _op in ("mattensormul", "tensormatmul"):
        PROTOTYPES["gf_%s_forward_host_%s" % (_op, _sfx)] = (_i, [_vp, _t, _t, _t, _i, _i, _i, _i])
        PROTOTYPES["gf_%s_backward_host_%s" % (_op, _sfx)] = (_i, [_vp, _t, _t, _t, _t, _t, _i, _i, _i, _i])
PROTOTYPES.update({
    "gf_matmul_forward_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i]),
    "gf_matmul_backward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "gf_mattensormul_forward_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "gf_mattensormul_backward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "gf_tensormatmul_forward_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "gf_tensormatmul_backward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "gf_custommatmultensor_forward_f32": (_i, [_vp, _vp, _vp, _vp, C.c_longlong, _i, _i]),
    "gf_custommatmultensor_backward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _i, _i, _i]),
    "gf_smp_create": (_i, [_vp, _cfgp, C.POINTER(_vp)]),
    "gf_smp_destroy": (_i, [_vp]),
    "gf_smp_param_count": (C.c_size_t, [_vp]),
    "gf_smp_config_param_count": (C.c_size_t, [_cfgp]),
    "gf_smp_classifier_config_param_count": (C.c_size_t, [_cfgp, _i]),
    "gf_smp_create_classifier": (_i, [_vp, _cfgp, _i, C.POINTER(_vp)]),
    "gf_smp_classes": (_i, [_vp]),
    "gf_smp_class_scores": (_i, [_vp, _vp, _vp]),
    "gf_smp_classifier_uniform_init_host": (_i, [_cfgp, _i, _fp]),
    "gf_smp_prepare": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]),
    "gf_smp_prepare_coulomb": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp]),
    "gf_smp_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_backward": (_i, [_vp, _vp, _vp, _i]),
    "gf_smp_set_grad_allreduce": (_i, [_vp, _i]),
    "gf_smp_feature_width": (C.c_size_t, [_vp]),
    "gf_smp_backward_features": (_i, [_vp, _vp, _vp, _vp, _i]),
    "gf_head_param_count": (C.c_size_t, [_i, C.POINTER(C.c_int)]),
    "gf_head_work_floats": (C.c_size_t, [_i, C.POINTER(C.c_int), _i]),
    "gf_head_forward_f32": (_i, [_vp, _i, C.POINTER(C.c_int), _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gf_head_backward_f32": (_i, [_vp, _i, C.POINTER(C.c_int), _vp, _i, _vp, _vp, _vp, _vp]),
    "gf_ctx_set_timing_filter": (_i, [_vp, C.c_char_p]),
    "gf_smp_parameters_upload": (_i, [_vp, _fp]),
    "gf_smp_parameters_download": (_i, [_vp, _fp, _fp]),
    "gf_smp_forward_host": (_i, [_vp, _dp, _dp, _dp, _dp]),
    "gf_smp_adam_step": (_i, [_vp, _vp, _vp, C.c_double, _i]),
    "gf_smp_adam_reset": (_i, [_vp]),
    "gf_smp_momentum_step": (_i, [_vp, _vp, _vp, C.c_double, _i, C.c_double]),
    "gf_smp_uniform_init_host": (_i, [_cfgp, _fp]),
    "gf_smp_save_model": (_i, [_vp, _vp, C.c_char_p]),
    "gf_smp_load_model": (_i, [_vp, _vp, C.c_char_p]),
    "gf_smp_set_fused": (_i, [_vp, _i]),
    "gf_smp_device_bytes": (_i, [_vp, _vp, _vp]),
    "gf_smp_single_vertex_launches": (C.c_longlong, [_vp]),
    "gf_smp_empty_row_calls": (C.c_longlong, [_vp]),
    "gf_smp_level_projected_f32": (_i, [_vp, _i, _vp]),
    "gf_smp_level_products_f32": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_level_wgrad_f32": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_level_products_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "gf_smp_level_wgrad_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_level_row_classes": (_i, [_vp, _i, _vp, _vp]),
    "gf_smp_level_row_classes_ex": (_i, [_vp, _i, _vp, _vp, _i]),
    "gf_smp_2d_ver5_rows_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_float, _i, _vp]),
    "gf_smp_2d_ver5_cols_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "gf_smp_2d_ver5_wgrad_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gf_smp_neighbourhood_fwd_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i] + [_vp] * 12),
    "gf_smp_neighbourhood_node_bwd_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_neighbourhood_gather_bwd_ex_f32": (_i, [_vp, _i, _i, _i] + [_vp] * 8),
    "gf_smp_neighbourhood_readout_ex_f32": (_i, [_vp, _i, _i, _i] + [_vp] * 9),
    "gf_smp_neighbourhood_fwd2_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gf_smp_neighbourhood_node_bwd2_ex_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i]),
    "gf_smp_neighbourhood_gather_bwd2_ex_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "gf_smp_gru_cell_fwd_ex_f32": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 13),
    "gf_smp_gru_cell_bwd_ex_f32": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 16),
    "gf_smp_gru_readout_fwd_ex_f32": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 11),
    "gf_smp_gru_readout_bwd_ex_f32": (_i, [_vp, _i, _i, _i, _i] + [_vp] * 11),
    "gf_smp_distance_rows_ex_f32": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "gf_smp_prepare_distance": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp]),
    "gf_smp_prepare_pairs": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]),
    "gf_smp_gram": (_i, [_vp, _vp]),
    "gf_smp_pair_readout_ex_f32": (_i, [_vp, _i, _i, _i] + [_vp] * 10),
    "gf_smp_gram_readout_ex_f32": (_i, [_vp, _i, _i, _i] + [_vp] * 6),
    "gf_smp_third_order_pool_fwd_ex_f32": (_i, [_vp, _i, _i] + [_vp] * 5),
    "gf_smp_third_order_pool_bwd_ex_f32": (_i, [_vp, _i, _i] + [_vp] * 8),
    "gf_smp_rowlist_product_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i] + [_vp] * 7 + [_i, _vp]),
    "gf_smp_rowlist_wgrad_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i] + [_vp] * 8),
    "gf_smp_covariant_forward_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i] + [_vp] * 13),
    "gf_smp_covariant_backward_ex_f32": (_i, [_vp, _i, _i, _i, _i, _i] + [_vp] * 12),
    "gf_smp_covariant_molecule_host": (_i, [_cfgp, _i, C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), _vp, _dp]),
    "gf_smp_matrix_form_molecule_host": (_i, [_cfgp, _i, C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]),
    "gf_smp_prepare_molecule_host": (_i, [_cfgp, _i, C.POINTER(C.c_int), _dp, C.POINTER(C.c_int), _dp]),
    "gf_smp_receptive_field": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_int), _i]),
    "gf_smp_read_activation": (C.c_longlong, [_vp, _i, _i, _i, _vp, C.c_size_t]),
    "gf_smp_read_reduced_adjacency": (C.c_longlong, [_vp, _i, _i, _i, _vp, C.c_size_t]),
    "gf_smp_level_sizes": (_i, [_vp, _i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "gf_smp_level_present_rows": (C.c_longlong, [_vp, _i]),
    "gf_smp_level_pairs": (C.c_longlong, [_vp, _i]),
    "gf_smp_level_covered_rows": (C.c_longlong, [_vp, _i]),
    "gf_stack_forward_f32": (_i, [_vp, _vp, _vp, _i, C.c_size_t]),
    "gf_stack_backward_f32": (_i, [_vp, _vp, _vp, _i, C.c_size_t]),
})

PROTOTYPES.update({
    "gf_smp_dropout_masks": (_i, [_vp, _vp, C.c_float]),
    "gf_adam_step_f32": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_double, _i, C.c_ulonglong]),
    "gf_smp_model_create": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "gf_smp_model_config_param_count": (C.c_size_t, [_vp]),
    "gf_smp_model_destroy": (_i, [_vp]),
    "gf_smp_model_param_count": (C.c_size_t, [_vp]),
    "gf_smp_model_set_mode": (_i, [_vp, _i]),
    "gf_smp_model_set_fused": (_i, [_vp, _i]),
    "gf_smp_model_prepare": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gf_smp_model_forward": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "gf_smp_model_backward": (_i, [_vp, _vp, _vp, _i]),
    "gf_smp_model_uniform_init_host": (_i, [_vp, _fp]),
    "gf_smp_model_parameters_upload": (_i, [_vp, _fp]),
    "gf_smp_model_parameters_download": (_i, [_vp, _fp, _fp]),
    "gf_smp_model_forward_host": (_i, [_vp, _dp, _dp, _dp]),
    "gf_smp_model_adam_step": (_i, [_vp, C.c_double, _i]),
})


class FitConfig(C.Structure):
    """gf_smp_fit_config"""
    _fields_ = [("kind", _i), ("optimiser", _i), ("nIterations", _i), ("learning_rate", C.c_double), ("epsilon", C.c_double),
                ("gamma", C.c_double)]


class FitReport(C.Structure):
    """gf_smp_fit_report"""
    _fields_ = [("first", C.c_double), ("second", C.c_double), ("iterations", _i), ("accepted", _i), ("rejected", _i),
                ("left_early", _i), ("learning_rate", C.c_double)]


_fitc, _fitr, _u8p = C.POINTER(FitConfig), C.POINTER(FitReport), C.POINTER(C.c_ubyte)
PROTOTYPES.update({
    "gf_smp_parameters_snapshot": (_i, [_vp, _vp]),
    "gf_smp_parameters_rollback": (_i, [_vp, _vp]),
    "gf_smp_forward_host_samples": (_i, [_vp, _dp, _dp, _dp, _dp]),
    "gf_smp_gram_host": (_i, [_vp, _dp]),
    "gf_smp_fit": (_i, [_vp, _vp, _vp, _vp, _fitc, _fitr, _u8p]),
    "gf_smp_fit_host": (_i, [_vp, _dp, _fitc, _fitr, _u8p]),
    "gf_smp_loss_sum_f32": (_i, [_vp, _vp, C.c_size_t, _dp]),
    "gf_smp_model_parameters_snapshot": (_i, [_vp, _vp]),
    "gf_smp_model_parameters_rollback": (_i, [_vp, _vp]),
    "gf_smp_model_fit": (_i, [_vp, _vp, _vp, _vp, _fitc, _fitr, _u8p]),
    "gf_smp_model_fit_host": (_i, [_vp, _dp, _fitc, _fitr, _u8p]),
})



class OptimConfig(C.Structure):
    """gf_optim_config"""
    _fields_ = [("kind", _i), ("nBatch", _i), ("learning_rate", C.c_double), ("gamma", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("rho", C.c_double), ("epsilon", C.c_double)]


OPTIMISERS = {"adam": 0, "momentum": 1, "sgd": 2, "adamax": 3, "adadelta": 4}   # gf_optim_config.kind = gf_smp_fit_config.optimiser
_optc, _szp = C.POINTER(OptimConfig), C.POINTER(C.c_size_t)
PROTOTYPES.update({
    "gf_smp_config_param_blocks": (C.c_size_t, [_cfgp, _szp, C.c_size_t]),
    "gf_smp_classifier_config_param_blocks": (C.c_size_t, [_cfgp, _i, _szp, C.c_size_t]),
    "gf_smp_model_config_param_blocks": (C.c_size_t, [_vp, _szp, C.c_size_t]),
    "gf_smp_optimiser_step": (_i, [_vp, _vp, _vp, _optc]),
    "gf_smp_model_optimiser_step": (_i, [_vp, _vp, _vp, _optc]),
    "gf_smp_regularise": (_i, [_vp, _vp, _vp, _i, C.c_double, _i, _dp]),
    "gf_smp_model_regularise": (_i, [_vp, _vp, _vp, _i, C.c_double, _i, _dp]),
    "gf_optimiser_step_f32": (_i, [_vp, _optc, _vp, _vp, C.c_size_t, _szp, _i, _vp, _vp, _vp, _dp]),
    "gf_regularise_f32": (_i, [_vp, _vp, _vp, C.c_size_t, _i, C.c_double, _i, _dp]),
})


def param_blocks(call, *args):
    """the offsets [count + 1] of one of the three *_config_param_blocks calls (the count first, then the table), or [] for a refusal"""
    lib = load()
    count = getattr(lib, call)(*args, None, 0)
    if not count:
        return []
    offsets = (C.c_size_t * (count + 1))()
    assert getattr(lib, call)(*args, offsets, count + 1) == count
    return list(offsets)


_lib = None


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the shared library (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", _CSRC, "-j4"], stdout=out)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "graphflow_amd: %s is missing -- build it with `make -C graphflow_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table drift apart
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
