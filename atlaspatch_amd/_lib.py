"""ctypes binding of libatlaspatch_hip.so (the C ABI declared in include/atlaspatch_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C atlaspatch_amd/csrc``.
There is NO fallback: if the library is missing or a call fails, the product raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

AP_F32, AP_F16, AP_BF16 = 0, 1, 2
AP_OK = 0
PROF_KINDS = ("preproc", "gemm_patch_embed", "gemm_qkv", "gemm_proj", "gemm_fc1", "gemm_fc2",
              "attention", "layernorm", "cls_tail")
AP_ERR_CAPACITY = -6
AP_ERR_UNSUPPORTED = -4
AP_ERR_INVALID = -1
AP_JPEG_GRAY, AP_JPEG_444, AP_JPEG_422, AP_JPEG_420 = 0, 1, 2, 3     # sampling of a JPEG coefficient slot
AP_JPEG_RGB = 4                  # three 1 x 1 components coded as R, G, B (no colour transform); device side: the *_ex entries take it

# Stream capture (the SAM2 hipGraph) must not overlap synchronous HIP calls on the legacy stream from other threads (the
# encoder built on a side thread uploads weights with hipMemcpy): both sides hold this lock for their critical section.
HIP_CAPTURE_LOCK = threading.RLock()

_LIB_NAME = "libatlaspatch_hip.so"
_lock = threading.Lock()
_lib = None


class HipLibraryError(RuntimeError):
    pass


AP_JPEG_STREAM_RESTART = 1       # flag of the *_streams_ex stagers: admit restart intervals (decoded by ap_jpeg_entropy_decode_tiles_rst)


def jpeg_restart_table_bound(side: int, sampling: int) -> int:
    """Arena bytes the restart table of one ``side`` x ``side`` tile can take: 4 per MCU (an interval of one MCU), rounded up to 16."""
    hmax, vmax = (2 if sampling in (AP_JPEG_422, AP_JPEG_420) else 1), (2 if sampling == AP_JPEG_420 else 1)
    mcus = -(-int(side) // (8 * hmax)) * -(-int(side) // (8 * vmax))
    return (4 * mcus + 15) // 16 * 16


ABI_VERSION = 20               # include/atlaspatch_hip.h: AP_ABI_VERSION; load() refuses a library that reports another


class VitConfig(C.Structure):
    """``ap_vit_config`` (ABI v20).  ``struct_size`` is filled in here, so positional construction starts at
    ``image_size`` as it did before the field existed."""
    _fields_ = [("struct_size", C.c_uint32), ("image_size", C.c_int), ("patch_size", C.c_int), ("dim", C.c_int),
                ("depth", C.c_int), ("heads", C.c_int), ("mlp_dim", C.c_int),
                ("ln_eps", C.c_float), ("layer_scale", C.c_int), ("compute_dtype", C.c_int),
                ("pool", C.c_int), ("pool_dim", C.c_int), ("pool_heads", C.c_int), ("pool_ln_eps", C.c_float),
                ("reg_tokens", C.c_int), ("no_embed_class", C.c_int), ("mlp_type", C.c_int), ("head_dim", C.c_int),
                ("attn_scale", C.c_float), ("pre_norm", C.c_int), ("act", C.c_int), ("proj_dim", C.c_int), ("rope", C.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


class VitConfigEx(VitConfig):
    """``ap_vit_config_ex``: the same bytes followed by the fields appended since ABI v20 (zero = the behaviour before the field
    existed).  ``struct_size`` records the longer size; ``ap_vit_create`` takes either."""
    _fields_ = [("no_class_token", C.c_int)]


class VitConfigEx2(VitConfigEx):
    """``ap_vit_config_ex2``: ``ap_vit_config_ex`` followed by the attentional pooler's fields of the CoCa / CONCH v1.5 towers
    (112 bytes; all four zero = ``VitConfigEx``)."""
    _fields_ = [("pool_head_dim", C.c_int), ("pool_skip_final_norm", C.c_int), ("pool_proj_dim", C.c_int),
                ("out_normalize", C.c_int)]


class ResnetConfig(C.Structure):
    """``ap_resnet_config`` (additive to ABI v20); ``struct_size`` is filled in here."""
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_int), ("depths", C.c_int * 4), ("stem_width", C.c_int),
                ("compute_dtype", C.c_int), ("image_size", C.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


RESNET_PROF_KINDS = ("stem", "conv1x1", "conv3x3", "pool")


class ConvnextConfig(C.Structure):
    """``ap_convnext_config`` (additive to ABI v20); ``struct_size`` is filled in here."""
    _fields_ = [("struct_size", C.c_uint32), ("depths", C.c_int * 4), ("widths", C.c_int * 4), ("compute_dtype", C.c_int),
                ("image_size", C.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


CONVNEXT_PROF_KINDS = ("stem", "dwconv_ln", "fc1", "fc2", "downsample", "pool")


class SwinConfig(C.Structure):
    """``ap_swin_config`` (additive to ABI v20); ``struct_size`` is filled in here."""
    _fields_ = [("struct_size", C.c_uint32), ("depths", C.c_int * 4), ("heads", C.c_int * 4), ("embed_dim", C.c_int),
                ("window", C.c_int), ("compute_dtype", C.c_int), ("image_size", C.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


SWIN_PROF_KINDS = ("stem", "ln", "qkv", "window_attn", "proj", "fc1", "fc2", "merge", "pool")


class ClipResnetConfig(C.Structure):
    """``ap_clip_resnet_config`` (additive to ABI v20); ``struct_size`` is filled in here."""
    _fields_ = [("struct_size", C.c_uint32), ("depths", C.c_int * 4), ("width", C.c_int), ("image_size", C.c_int),
                ("output_dim", C.c_int), ("compute_dtype", C.c_int)]

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(type(self)), *args, **kw)


CLIP_RESNET_PROF_KINDS = ("stem", "conv1x1", "conv3x3", "avgpool", "head")


# name -> (restype, argtypes); every symbol include/atlaspatch_hip.h declares
SIGNATURES = {
    "ap_abi_version": (C.c_int, []),
    "ap_last_error": (C.c_char_p, []),
    "ap_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ap_preproc_u8hwc_to_chw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                          C.c_int, C.c_void_p]),
    "ap_preproc_u8hwc_to_chw_any": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                              C.c_int, C.c_void_p]),
    "ap_preproc_u8hwc_to_patchrows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                                C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ap_host_inflate_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_size_t]),
    "ap_host_decode_jpeg_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int]),
    "ap_jpeg_slot_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ap_jpeg_slot_bytes_ex": (C.c_size_t, [C.c_int, C.c_int]),
    "ap_host_jpeg_probe": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ap_host_jpeg_coefficients": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "ap_jpeg_decode_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_jpeg_decode_tiles_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_jpeg_stream_header_bytes": (C.c_size_t, []),
    "ap_host_jpeg_stream_bound": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_size_t)]),
    "ap_host_jpeg_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                       C.c_int]),
    "ap_jpeg_entropy_decode_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p]),
    "ap_jpeg_entropy_decode_tiles_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p]),
    "ap_host_jpeg_streams_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                          C.c_int, C.c_int]),
    "ap_jpeg_entropy_decode_tiles_rst": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                   C.c_int, C.c_void_p]),
    "ap_host_format_passports": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int]),
    "ap_host_gather_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_size_t]),
    "ap_host_synth_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                      C.c_uint32, C.c_void_p, C.c_int]),
    "ap_resample_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_cv2_resize_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p]),
    "ap_tile_content_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "ap_sizeof_vit_config": (C.c_size_t, []),
    "ap_vit_config_init": (C.c_int, [C.POINTER(VitConfig), C.c_size_t]),
    "ap_vit_create": (C.c_int, [C.POINTER(VitConfig), C.POINTER(C.c_void_p)]),
    "ap_vit_destroy": (None, [C.c_void_p]),
    "ap_vit_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ap_vit_set_params": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]),
    "ap_vit_finalize": (C.c_int, [C.c_void_p]),
    "ap_vit_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ap_vit_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_vit_embed_dim": (C.c_int, [C.c_void_p]),
    "ap_vit_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_vit_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]),
    "ap_vit_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_vit_forward_chw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "ap_sizeof_resnet_config": (C.c_size_t, []),
    "ap_resnet_config_init": (C.c_int, [C.POINTER(ResnetConfig), C.c_size_t]),
    "ap_resnet_create": (C.c_int, [C.POINTER(ResnetConfig), C.POINTER(C.c_void_p)]),
    "ap_resnet_destroy": (None, [C.c_void_p]),
    "ap_resnet_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ap_resnet_finalize": (C.c_int, [C.c_void_p]),
    "ap_resnet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_resnet_embed_dim": (C.c_int, [C.c_void_p]),
    "ap_resnet_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_resnet_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]),
    "ap_resnet_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_conv2d_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_maxpool3x3s2_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_avgpool_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_sizeof_convnext_config": (C.c_size_t, []),
    "ap_convnext_config_init": (C.c_int, [C.POINTER(ConvnextConfig), C.c_size_t]),
    "ap_convnext_create": (C.c_int, [C.POINTER(ConvnextConfig), C.POINTER(C.c_void_p)]),
    "ap_convnext_destroy": (None, [C.c_void_p]),
    "ap_convnext_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ap_convnext_finalize": (C.c_int, [C.c_void_p]),
    "ap_convnext_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_convnext_embed_dim": (C.c_int, [C.c_void_p]),
    "ap_convnext_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_convnext_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]),
    "ap_convnext_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_conv2d_nhwc_ex": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_dwconv7_ln_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "ap_layernorm_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                    C.c_void_p]),
    "ap_sizeof_swin_config": (C.c_size_t, []),
    "ap_swin_config_init": (C.c_int, [C.POINTER(SwinConfig), C.c_size_t]),
    "ap_swin_create": (C.c_int, [C.POINTER(SwinConfig), C.POINTER(C.c_void_p)]),
    "ap_swin_destroy": (None, [C.c_void_p]),
    "ap_swin_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ap_swin_finalize": (C.c_int, [C.c_void_p]),
    "ap_swin_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_swin_embed_dim": (C.c_int, [C.c_void_p]),
    "ap_swin_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_swin_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]),
    "ap_swin_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_swin_window_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "ap_patch_merge_ln": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_void_p]),
    "ap_sizeof_clip_resnet_config": (C.c_size_t, []),
    "ap_clip_resnet_config_init": (C.c_int, [C.POINTER(ClipResnetConfig), C.c_size_t]),
    "ap_clip_resnet_create": (C.c_int, [C.POINTER(ClipResnetConfig), C.POINTER(C.c_void_p)]),
    "ap_clip_resnet_destroy": (None, [C.c_void_p]),
    "ap_clip_resnet_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ap_clip_resnet_finalize": (C.c_int, [C.c_void_p]),
    "ap_clip_resnet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_clip_resnet_embed_dim": (C.c_int, [C.c_void_p]),
    "ap_clip_resnet_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_clip_resnet_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]),
    "ap_clip_resnet_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_avgpool2x2_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_clip_attnpool_tokens": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "ap_gemm": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_gemm_fused": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ap_stream_init": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ap_rowstats_finalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ap_gemm_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_split_f16_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_gemm_split_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_void_p]),
    "ap_gemm_split_f16_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_layernorm": (C.c_int, [C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_float, C.c_void_p, C.c_void_p]),
    "ap_attention": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # engine building blocks: the kernels ap_vit_forward_* chains, one export each
    "ap_attention_scaled": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "ap_attention_cls": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_void_p]),
    "ap_attn_pool": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_attention_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_float, C.c_void_p]),
    "ap_rope": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                          C.c_void_p]),
    "ap_swiglu": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_add2_layernorm": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long,
                                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "ap_fold_ln": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ap_fold_ls": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "ap_cls_mean_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_l2_normalize_rows": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ap_stream_to_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_chw_to_patchrows": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ap_cls_stream": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ap_cls_exact_update": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ap_rowstats_finalize_cls": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ap_sgemm": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int,
                           C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_long,
                           C.c_void_p, C.c_long, C.c_long, C.c_void_p]),
    "ap_sgemm_stacked": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]),
    "ap_softmax_rows": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "ap_sattention_f32": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_long, C.c_void_p]),
    "ap_sattention_split_f16": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_long, C.c_void_p]),
    "ap_sam2_patchify": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p,
                                   C.c_void_p]),
    "ap_window_partition": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_window_unpartition": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_window_unpartition_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    "ap_maxpool2x2": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_add_rowvec": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "ap_gelu": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "ap_upsample2x_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_convt2x2_shuffle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p]),
    "ap_bilinear_up4_threshold": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "ap_contours_from_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.POINTER(C.c_void_p), C.c_void_p]),
    "ap_contours_destroy": (None, [C.c_void_p]),
    "ap_contours_count": (C.c_int, [C.c_void_p]),
    "ap_contours_num_holes": (C.c_int, [C.c_void_p, C.c_int]),
    "ap_contours_points": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "ap_grid_coords": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]),
    "ap_clock_probe": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ap_synth_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                 C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_gather2d_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_synth_region": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_uint32,
                                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ap_pillow_reduce_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    "ap_host_openslide_available": (C.c_int, []),
    "ap_host_openslide_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "ap_host_openslide_read_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_host_openslide_close": (None, [C.c_void_p]),
    "ap_host_tiff_open": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "ap_host_tiff_close": (None, [C.c_void_p]),
    "ap_host_tiff_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "ap_host_tiff_level": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "ap_host_tiff_tile_present": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "ap_host_tiff_read_patches": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ap_host_tiff_tile_coefficients": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ap_host_tiff_max_tile_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "ap_host_tiff_tile_streams": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "ap_host_tiff_tile_streams_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_size_t), C.c_int]),
    "ap_gather_patches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
}


def library_path() -> str:
    """The in-tree product library; ATLASPATCH_HIP_LIB names another build of the same ABI (tools only: the debug
    library with the GEMM A/B twin, `make -C atlaspatch_amd/csrc twin`)."""
    override = os.environ.get("ATLASPATCH_HIP_LIB")
    if override:
        return override
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load():
    """Load (once) and return the ctypes handle.  Raises HipLibraryError when the .so is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise HipLibraryError(
                f"{path} not found: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C atlaspatch_amd/csrc`. "
                "There is no CPU fallback.")
        try:
            # torch bundles its own libamdhip64.so.7; import it first so both share ONE HIP runtime
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for symbol checks
            pass
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        # the ABI question first, on the two symbols it needs: a stale library must be refused with "rebuild", not fail
        # on the first symbol it lacks
        rebuild = "Rebuild the library (`make -C atlaspatch_amd/csrc`)."
        try:
            lib.ap_abi_version.restype, lib.ap_abi_version.argtypes = SIGNATURES["ap_abi_version"]
            got = lib.ap_abi_version()
        except AttributeError as exc:
            raise HipLibraryError(f"{path} does not export ap_abi_version: not a build of include/atlaspatch_hip.h. {rebuild}") from exc
        size = None
        if hasattr(lib, "ap_sizeof_vit_config"):
            lib.ap_sizeof_vit_config.restype, lib.ap_sizeof_vit_config.argtypes = SIGNATURES["ap_sizeof_vit_config"]
            size = lib.ap_sizeof_vit_config()
        if got != ABI_VERSION or size != C.sizeof(VitConfig):
            raise HipLibraryError(
                f"{path} reports ABI {got} with a {size}-byte ap_vit_config; this binding is written "
                f"for ABI {ABI_VERSION} / {C.sizeof(VitConfig)} bytes (include/atlaspatch_hip.h). {rebuild}")
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:
                raise HipLibraryError(f"{path} (ABI {got}) does not export {name}, which include/atlaspatch_hip.h declares: "
                                      f"the library is older than this binding. {rebuild}") from exc
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return _lib


def check(code: int, what: str = "") -> None:
    if code != AP_OK:
        msg = load().ap_last_error()
        raise HipLibraryError(f"{what or 'libatlaspatch_hip'} failed with code {code}: "
                              f"{msg.decode(errors='replace') if msg else ''}")


def f3(values):
    arr = (C.c_float * 3)(*[float(v) for v in values])
    return arr


def torch_dtype_code(dtype) -> int:
    import torch
    table = {torch.float32: AP_F32, torch.float16: AP_F16, torch.bfloat16: AP_BF16}
    if dtype not in table:
        raise ValueError(f"unsupported compute dtype {dtype}")
    return table[dtype]


def current_stream_ptr(device=None) -> int:
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)
