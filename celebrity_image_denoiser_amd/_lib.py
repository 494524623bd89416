"""ctypes binding of include/cid.h -> libcid.so.  No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CID_LIB_PATH: development aid for same-box A/B runs of two builds of the library (bench.py in alternation)
LIB_PATH = os.environ.get("CID_LIB_PATH") or os.path.join(_HERE, "libcid.so")

CID_OK = 0
CID_NUM_PARAMS = 24
CID_NUM_LAUNCHES = 12
CID_ALGO_DIRECT, CID_ALGO_WINOGRAD64, CID_ALGO_WINOGRAD42, CID_ALGO_SPLIT16 = 0, 2, 3, 4
CID_FMT_F32_NCHW, CID_FMT_U8_NHWC = 0, 1
CID_DTYPE_F32, CID_DTYPE_F16 = 0, 1
CID_TAIL_FUSED, CID_TAIL_BANDS, CID_TAIL_TILES = 0, 1, 2
CID_METRIC_PSNR, CID_METRIC_SSIM, CID_METRIC_MS_SSIM = 1, 2, 4
CID_DISC_MOMENTUM_NONE = -1.0
CID_NOISE_GAUSSIAN, CID_NOISE_SALT_PEPPER, CID_NOISE_SPECKLE, CID_NOISE_POISSON, CID_NOISE_UNIFORM = 0, 1, 2, 3, 4
CID_ADAM_MAX_TENSORS = 32
CID_RESAMPLE_BICUBIC = 3
CID_SR_RAW = 1
CID_CG_RAW = 1
CID_LPIPS_UNIT_VIEW = 1
CID_LPIPS_NUM_WEIGHTS = 17
CID_VGG_LPIPS, CID_VGG_CONTENT = 0, 1
CID_VGG_NUM_WEIGHTS = 33
CID_SRD_NUM_WEIGHTS = 14
CID_VGG_MAX_SIDE = 512
CID_ESD_NUM_WEIGHTS = 10
CID_ESD_MAX_SIDE = 4096


class AdamTensor(ctypes.Structure):
    """cid_adam_tensor"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("count", ctypes.c_int64), ("step", ctypes.c_int64)]


class AdamHyper(ctypes.Structure):
    """cid_adam_hyper"""
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double)]


# every symbol include/cid.h declares: (restype, argtypes)
_c = ctypes
SYMBOLS = {
    "cid_version": (_c.c_char_p, []),
    "cid_create": (_c.c_int, [_c.POINTER(_c.c_void_p)]),
    "cid_destroy": (None, [_c.c_void_p]),
    "cid_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_get_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.c_size_t]),
    "cid_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_param_key": (_c.c_char_p, [_c.c_int]),
    "cid_packed_weights_bytes": (_c.c_size_t, []),
    "cid_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_packed_segment": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_char_p), _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t)]),
    "cid_export_packed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "cid_import_packed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "cid_attach_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "cid_out_shape": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                               _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_forward_ex": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_forward_padded": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_view_u8": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "cid_forward_timed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_float)]),
    "cid_timing_begin": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "cid_timing_end": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_float), _c.POINTER(_c.c_int)]),
    "cid_launch_name": (_c.c_char_p, [_c.c_int]),
    "cid_launch_kernel": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_set_conv_algo": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "cid_get_conv_algo": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_set_tail_algo": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "cid_get_tail_algo": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_debug_poison_lds": (_c.c_int, [_c.c_void_p]),
    "cid_debug_winograd_workgroups_per_cu": (_c.c_int, [_c.c_int]),
    "cid_debug_half_workgroups_per_cu": (_c.c_int, [_c.c_int]),
    "cid_debug_winograd_column_block_per_xcd": (_c.c_int, [_c.c_int]),
    "cid_set_compute_dtype": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "cid_get_compute_dtype": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_launch_work_ex": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "cid_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                  _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_comm_available": (_c.c_int, []),
    "cid_comm_unique_id": (_c.c_int, [_c.c_void_p]),
    "cid_comm_init_rank": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_void_p, _c.c_int]),
    "cid_comm_destroy": (_c.c_int, [_c.c_void_p]),
    "cid_comm_count": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_broadcast_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "cid_launch_work": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "cid_quality_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_quality": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                               _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_add_noise": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_double), _c.c_int,
                                 _c.c_uint64, _c.c_uint64, _c.c_void_p]),
    "cid_disc_create": (_c.c_int, [_c.POINTER(_c.c_void_p)]),
    "cid_disc_destroy": (None, [_c.c_void_p]),
    "cid_disc_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_disc_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_disc_packed_weights_bytes": (_c.c_size_t, []),
    "cid_disc_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_disc_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_disc_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                    _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_srd_create": (_c.c_int, [_c.POINTER(_c.c_void_p)]),
    "cid_srd_destroy": (None, [_c.c_void_p]),
    "cid_srd_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_srd_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_srd_packed_weights_bytes": (_c.c_size_t, []),
    "cid_srd_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_srd_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_srd_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                   _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_srd_losses": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_srd_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_srd_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                         _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_srd_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_srd_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                    _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_srd_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_srd_saved_masks": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_esd_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int]),
    "cid_esd_destroy": (None, [_c.c_void_p]),
    "cid_esd_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_esd_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_esd_packed_weights_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "cid_esd_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_esd_export_packed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t]),
    "cid_esd_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esd_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                   _c.c_void_p]),
    "cid_esd_losses": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_esd_trainer_losses": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_void_p]),
    "cid_esd_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esd_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                         _c.c_size_t, _c.c_void_p]),
    "cid_esd_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esd_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                    _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_esd_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_disc_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_disc_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                          _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_disc_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_disc_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                     _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_disc_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_disc_saved_masks": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_disc_losses": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                   _c.c_void_p, _c.c_void_p]),
    "cid_adam_step": (_c.c_int, [_c.POINTER(AdamTensor), _c.c_int, _c.POINTER(AdamHyper), _c.c_void_p]),
    "cid_debug_adam_step_host": (_c.c_int, [_c.POINTER(AdamTensor), _c.c_int, _c.POINTER(AdamHyper)]),
    "cid_resize_plan_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "cid_resize_plan_destroy": (None, [_c.c_void_p]),
    "cid_resize_plan_table": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    "cid_resize": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p]),
    "cid_esr_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int]),
    "cid_esr_destroy": (None, [_c.c_void_p]),
    "cid_esr_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_esr_param_key": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_esr_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_esr_set_bn_eps": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_double]),
    "cid_esr_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_esr_packed_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_esr_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_esr_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esr_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                   _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_esr_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                      _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_esr_train_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esr_forward_train": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_esr_train_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t),
                                            _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_esr_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esr_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                         _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_esr_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_esr_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                    _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_esr_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_esr_saved_masks": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_sr_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int]),
    "cid_sr_destroy": (None, [_c.c_void_p]),
    "cid_sr_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_sr_param_key": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_sr_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_sr_set_bn_eps": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_double]),
    "cid_sr_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_sr_packed_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_sr_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_sr_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_sr_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_sr_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                     _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_sr_train_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_sr_forward_train": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_uint, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_sr_train_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t),
                                           _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_sr_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_sr_forward_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_uint,
                                        _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_sr_backward_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_sr_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p,
                                   _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_sr_pack_weights_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_sr_saved_masks": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_cg_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int]),
    "cid_cg_destroy": (None, [_c.c_void_p]),
    "cid_cg_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_cg_param_key": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_cg_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_cg_set_bn_eps": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_double]),
    "cid_cg_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_cg_packed_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_cg_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_cg_workspace_bytes": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_cg_latent": (_c.c_int, [_c.c_uint64, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "cid_cg_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p,
                                  _c.c_size_t, _c.c_void_p]),
    "cid_cg_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                     _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_lpips_create": (_c.c_int, [_c.POINTER(_c.c_void_p)]),
    "cid_lpips_destroy": (None, [_c.c_void_p]),
    "cid_lpips_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_lpips_param_key": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_lpips_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_lpips_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_lpips_packed_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_lpips_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_lpips_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_lpips_stage_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                        _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_lpips": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_uint,
                             _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_vgg_create": (_c.c_int, [_c.POINTER(_c.c_void_p)]),
    "cid_vgg_destroy": (None, [_c.c_void_p]),
    "cid_vgg_last_error": (_c.c_char_p, [_c.c_void_p]),
    "cid_vgg_param_key": (_c.c_char_p, [_c.c_void_p, _c.c_int]),
    "cid_vgg_set_weight": (_c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_void_p, _c.POINTER(_c.c_int64), _c.c_int]),
    "cid_vgg_missing_weights": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int)]),
    "cid_vgg_packed_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_vgg_upload_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_vgg_workspace_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_vgg_stage_view": (_c.c_int, [_c.c_int, _c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                      _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_vgg_lpips": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_uint,
                                 _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_vgg_content_loss": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_uint,
                                        _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_vgg_saved_bytes": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t)]),
    "cid_vgg_saved_view": (_c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_int),
                                      _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "cid_vgg_content_loss_saved": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_uint, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "cid_vgg_backward_weights_bytes": (_c.c_size_t, [_c.c_void_p]),
    "cid_vgg_upload_backward_weights": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "cid_vgg_content_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_uint, _c.c_void_p,
                                            _c.c_size_t, _c.c_void_p]),
}

_lib = None


class CidError(RuntimeError):
    """A cid_* call returned a non-zero status."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def lib() -> ctypes.CDLL:
    """Load libcid.so (built by `python -c 'import __graft_entry__ as g; g.build()'` or csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is not built. This package has no CPU or PyTorch "
                "fallback; build it with `make -C celebrity_image_denoiser_amd/csrc` (needs hipcc)."
            )
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so (same SONAME as
        # /opt/rocm's).  Load torch's copy first so libcid.so binds to the runtime that owns the
        # tensors and streams it is handed; two runtimes in one process do not see each other's devices.
        import torch

        hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(hip_rt):
            ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError here = header and library out of sync
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(handle, code: int):
    if code != CID_OK:
        msg = lib().cid_last_error(handle)
        raise CidError(code, (msg.decode() if msg else "") or f"cid error {code}")


def check_abi(abi: str, handle, code: int):
    """check() for the handle of the family cid_<abi>_*: "esr", "sr", "cg", "lpips", "vgg", "disc", "srd" or "esd"."""
    if code != CID_OK:
        msg = getattr(lib(), f"cid_{abi}_last_error")(handle) if handle else None
        raise CidError(code, (msg.decode() if msg else "") or f"cid error {code}")


def check_disc(handle, code: int):
    """check() for a cid_disc_t handle."""
    check_abi("disc", handle, code)


def check_srd(handle, code: int):
    """check() for a cid_srd_t handle."""
    check_abi("srd", handle, code)


def check_lpips(handle, code: int):
    """check() for a cid_lpips_t handle (the tests call it)."""
    check_abi("lpips", handle, code)


def check_vgg(handle, code: int):
    """check() for a cid_vgg_t handle (the tests call it)."""
    check_abi("vgg", handle, code)
