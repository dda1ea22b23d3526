"""ctypes binding of libltk_hip.so (include/ltk.h).

The HIP library IS the product path: importing this module without the built
shared object raises, there is no CPU/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LTK_LIB") or os.path.join(_HERE, "libltk_hip.so")      # LTK_LIB: A/B runs against another build


class LtkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ltk error {code}: {msg}")
        self.code = code


class NamedTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("ndim", C.c_int),
                ("shape", C.POINTER(C.c_int64))]


class W2lReq(C.Structure):
    _fields_ = [("avatar", C.c_int), ("index", C.c_int), ("batch", C.c_int), ("d_mel", C.c_void_p),
                ("d_pred", C.c_void_p)]


class MtReq(C.Structure):
    _fields_ = [("avatar", C.c_int), ("index", C.c_int), ("batch", C.c_int), ("d_feat", C.c_void_p), ("d_pred", C.c_void_p)]


class UlReq(C.Structure):
    _fields_ = [("avatar", C.c_int), ("index", C.c_int), ("batch", C.c_int), ("d_feat", C.c_void_p), ("d_pred", C.c_void_p)]


UL_MERGE_MAX_PASSES = 64     # include/ltk.h LTK_UL_MERGE_MAX_PASSES
UL_PATH_PER_AVATAR, UL_PATH_GROUPED = 0, 1


class UlMergeReport(C.Structure):
    _fields_ = [("n_passes", C.c_int), ("n_avatars", C.c_int), ("grouped", C.c_int), ("frames", C.c_int),
                ("path", C.c_int * UL_MERGE_MAX_PASSES), ("nf", C.c_int * UL_MERGE_MAX_PASSES), ("avatar", C.c_int * UL_MERGE_MAX_PASSES)]


class HubertReq(C.Structure):
    _fields_ = [("pcm", C.c_void_p), ("n_samples", C.c_int), ("batch", C.c_int), ("first_row", C.c_int), ("row_step", C.c_int),
                ("rows", C.c_int), ("d_out", C.c_void_p)]


class WhisperReq(C.Structure):
    _fields_ = [("pcm", C.c_void_p), ("n_samples", C.c_int), ("batch", C.c_int), ("first_row", C.c_int), ("row_step", C.c_int),
                ("rows", C.c_int), ("d_out", C.c_void_p)]


class EgressReq(C.Structure):
    _fields_ = [("source", C.c_int), ("avatar", C.c_int), ("idx", C.c_int), ("d_pred", C.c_void_p), ("h_frame", C.c_void_p),
                ("speaking", C.c_int), ("alpha", C.c_double), ("keep", C.c_int), ("format", C.c_int), ("chroma", C.c_int)]


class ConvOpts(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("x_ld", "x_coff", "y_ld", "y_coff", "res_ld", "res_coff", "act", "ups", "force_pxw", "force_nbt",
                                       "force_ksplit", "family")]


class ConvReport(C.Structure):
    _fields_ = [("kernel", C.c_char * 64)] + [(n, C.c_int) for n in ("family", "G", "NBT", "PXW", "NC8", "T", "S", "ksplit", "items", "grid",
                                                                     "FT", "UB", "l2w", "l2h", "NB", "s2half", "phases", "lds", "args_hash")]


class UlIrReport(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("reason", C.c_char * 160)] + [(n, C.c_int) for n in (
        "accepted", "Ho", "Wo", "TH", "TW", "MC", "chunks", "hidden_px", "lds_bytes", "lds_limit", "grid_x", "grid_y", "grid_z", "blocks",
        "threads")]


class UlOpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64)] + [(n, C.c_int) for n in (
        "type", "in_buf", "in_ld", "in_coff", "H", "W", "out_buf", "out_ld", "out_coff", "Ho", "Wo", "res_buf", "res_ld", "res_coff",
        "C", "Creal", "cin", "k", "stride", "pad", "relu")]


class FpOpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64)] + [(n, C.c_int) for n in ("type", "cin", "cout", "k", "stride", "pad", "relu", "ups", "has_res", "plus1",
                                                                     "H", "W", "Ho", "Wo")]


class FpView(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("buf", "ld", "coff", "C", "H", "W")]


class FpBind(C.Structure):
    _fields_ = [("name", C.c_char * 64)] + [(n, FpView) for n in ("x", "y", "r", "a", "b")]


class FdOpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64)] + [(n, C.c_int) for n in ("type", "cin", "cout", "k", "stride", "pad", "relu", "maxout", "level",
                                                                     "H", "W", "Ho", "Wo")]


class FdBind(C.Structure):
    _fields_ = [("name", C.c_char * 64)] + [(n, FpView) for n in ("x", "y")]


class NormOpts(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("x_ld", "x_coff", "y_ld", "y_coff")]


class NormReport(C.Structure):
    _fields_ = [("kernel", C.c_char * 64)] + [(n, C.c_int) for n in ("impl", "segs", "members", "grid")]


class HealthOp(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("type", C.c_int), ("observed", C.c_int), ("q8", C.c_int), ("elements", C.c_ulonglong),
                ("at_limit", C.c_ulonglong), ("near_limit", C.c_ulonglong), ("nonfinite", C.c_ulonglong), ("max_abs", C.c_float),
                ("limit", C.c_float)]


# include/ltk.h LTK_HEALTH_*: the programs a headroom watch can be armed for
HEALTH_WAV2LIP, HEALTH_MUSETALK, HEALTH_ULTRALIGHT, HEALTH_WHISPER, HEALTH_HUBERT = range(5)
HEALTH_FACEPARSE = 6         # (5 stays unassigned)
HEALTH_FACEDET = 7
HEALTH_PROGRAMS = {"wav2lip": HEALTH_WAV2LIP, "musetalk": HEALTH_MUSETALK, "ultralight": HEALTH_ULTRALIGHT, "whisper": HEALTH_WHISPER,
                   "hubert": HEALTH_HUBERT, "faceparse": HEALTH_FACEPARSE, "facedet": HEALTH_FACEDET}

DEFER_SYNC = 2      # flag of ltk_wav2lip_infer_deferred

# every symbol include/ltk.h declares: (restype, argtypes)
SYMBOLS = {
    "ltk_last_error": (C.c_char_p, []),
    "ltk_version": (C.c_char_p, []),
    "ltk_engine_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "ltk_engine_destroy": (None, [C.c_void_p]),
    "ltk_engine_sync": (C.c_int, [C.c_void_p]),
    "ltk_wav2lip_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.c_int]),
    "ltk_avatar_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_int)]),
    "ltk_avatar_release": (C.c_int, [C.c_void_p, C.c_int]),
    "ltk_mel_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ltk_wav2lip_infer": (C.c_int, [C.c_void_p, C.POINTER(W2lReq), C.c_int, C.c_void_p]),
    "ltk_wav2lip_infer_deferred": (C.c_int, [C.c_void_p, C.POINTER(W2lReq), C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "ltk_wav2lip_order_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ltk_wav2lip_defer_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "ltk_paste_back": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_paste_back_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ltk_musetalk_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.POINTER(NamedTensor), C.c_int, C.c_int]),
    "ltk_musetalk_set_fp8": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "ltk_musetalk_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ltk_musetalk_avatar_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ltk_musetalk_infer": (C.c_int, [C.c_void_p, C.POINTER(MtReq), C.c_int, C.c_void_p]),
    "ltk_paste_blend": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_ultralight_avatar_register": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ltk_ultralight_infer": (C.c_int, [C.c_void_p, C.POINTER(UlReq), C.c_int, C.c_void_p]),
    "ltk_ultralight_infer_merged": (C.c_int, [C.c_void_p, C.POINTER(UlReq), C.c_int, C.c_int, C.c_void_p, C.POINTER(UlMergeReport)]),
    "ltk_ultralight_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "ltk_debug_ul_merge_plan": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.c_int, C.POINTER(C.c_int)]),
    "ltk_ul_gconv_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ConvOpts),
                                   C.POINTER(ConvReport)]),
    "ltk_debug_ul_ir_plan": (C.c_int, [C.c_int] * 9 + [C.POINTER(ConvOpts), C.POINTER(UlIrReport)]),
    "ltk_ul_ir_f16": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 11 + [C.POINTER(ConvOpts), C.c_void_p, C.c_void_p,
                                C.POINTER(UlIrReport)]),
    "ltk_ultralight_paste_back": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_ultralight_paste_back_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ltk_ultralight_forward_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_ultralight_time": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "ltk_dwconv3x3_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_upsample2x_cat_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]),
    "ltk_parse_stem_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(ConvOpts)]),
    "ltk_maxpool3x3s2_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_global_avgpool_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_chan_gate_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.POINTER(ConvOpts)]),
    "ltk_seg_argmax_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ltk_debug_face_parse_program": (C.c_int, [C.c_int, C.POINTER(FpOpInfo), C.c_int, C.POINTER(C.c_int)]),
    "ltk_debug_face_parse_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(FpBind), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.c_int,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ltk_face_parse_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.c_int, C.c_int]),
    "ltk_face_parse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_face_parse_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_debug_face_parse_time": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "ltk_s3fd_stem_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_maxpool2x2s2_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_l2norm_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_s3fd_detect_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                      C.c_void_p, C.POINTER(ConvOpts)]),
    "ltk_face_detect_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.c_int]),
    "ltk_face_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_face_detect_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_debug_face_detect_time": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "ltk_debug_face_detect_program": (C.c_int, [C.c_int, C.c_int, C.POINTER(FdOpInfo), C.c_int, C.POINTER(C.c_int)]),
    "ltk_debug_face_detect_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(FdBind), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                             C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    "ltk_egress_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "ltk_egress_close": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ltk_egress_watermark": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ltk_egress_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(EgressReq), C.c_void_p, C.c_void_p]),
    "ltk_egress_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p]),
    "ltk_musetalk_forward_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ltk_musetalk_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_musetalk_debug_get_q8": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_musetalk_time": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "ltk_health_watch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "ltk_health_report": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(HealthOp), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int)]),
    "ltk_health_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.POINTER(HealthOp)]),
    "ltk_whisper_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int]),
    "ltk_whisper_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ltk_whisper_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ltk_whisper_step_batch": (C.c_int, [C.c_void_p, C.POINTER(WhisperReq), C.c_int]),
    "ltk_whisper_debug_get_clip": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_whisper_batch_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ltk_debug_whisper_batch_plan": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ltk_hubert_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int]),
    "ltk_hubert_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "ltk_hubert_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ltk_hubert_step_batch": (C.c_int, [C.c_void_p, C.POINTER(HubertReq), C.c_int]),
    "ltk_hubert_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ltk_hubert_debug_get_clip": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "ltk_hubert_batch_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ltk_debug_hubert_batch_plan": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ltk_ultralight_op_count": (C.c_int, [C.c_void_p, C.c_int]),
    "ltk_ultralight_op_name": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "ltk_debug_ultralight_program": (C.c_int, [C.c_int, C.POINTER(UlOpInfo), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_int,
                                               C.POINTER(C.c_int)]),
    "ltk_hubert_op_count": (C.c_int, [C.c_void_p]),
    "ltk_hubert_op_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "ltk_hubert_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "ltk_hubert_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "ltk_hubert_layer0_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ltk_hubert_ln_gelu_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ltk_hubert_posconv_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ltk_hubert_chunks_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ltk_vae_encoder_load": (C.c_int, [C.c_void_p, C.POINTER(NamedTensor), C.c_int, C.c_int]),
    "ltk_vae_encode_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ltk_wav2lip_forward_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ltk_debug_capture": (C.c_int, [C.c_void_p, C.c_int]),
    "ltk_debug_set_knob": (C.c_int, [C.c_char_p, C.c_int]),
    "ltk_debug_tile_table_check": (C.c_int, [C.c_char_p, C.c_int]),
    "ltk_debug_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "ltk_wav2lip_time_convs": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "ltk_wav2lip_graph_count": (C.c_int, [C.c_void_p]),
    "ltk_program_graph_count": (C.c_int, [C.c_void_p]),
    "ltk_wav2lip_prefetch_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "ltk_debug_solo_walk": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ltk_avatar_face_cache_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "ltk_musetalk_op_count": (C.c_int, [C.c_void_p]),
    "ltk_musetalk_op_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "ltk_musetalk_time_ops": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "ltk_wav2lip_layer_count": (C.c_int, [C.c_void_p]),
    "ltk_wav2lip_layer_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    "ltk_wav2lip_set_layer_tile": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ltk_wav2lip_time_layers": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "ltk_conv2d_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_float)]),
    "ltk_conv2d_f16_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ConvOpts), C.POINTER(ConvReport)]),
    "ltk_debug_conv_plan": (C.c_int, [C.c_int] * 15 + [C.POINTER(ConvOpts), C.POINTER(ConvReport)]),
    "ltk_debug_conv3_variants": (C.c_int, [C.c_char_p, C.c_int]),
    "ltk_debug_conv1_variants": (C.c_int, [C.c_char_p, C.c_int]),
    "ltk_w2l_head_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.POINTER(NormOpts)]),
    "ltk_groupnorm_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_float, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "ltk_groupnorm_f16_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_float, C.c_void_p, C.POINTER(NormOpts), C.POINTER(NormReport)]),
    "ltk_pointwise_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                    C.POINTER(NormOpts)]),
    "ltk_attention_f16": (C.c_int, [C.c_void_p] + [C.c_void_p, C.c_int, C.c_int] * 4 + [C.c_int] * 6),
    "ltk_f32_to_e4m3": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "ltk_conv2d_fp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "ltk_conv2d_fp8_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ConvOpts), C.POINTER(ConvReport)]),
    "ltk_debug_conv_fp8_plan": (C.c_int, [C.c_int] * 15 + [C.POINTER(ConvOpts), C.POINTER(ConvReport)]),
    "ltk_debug_conv3_fp8_variants": (C.c_int, [C.c_char_p, C.c_int]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library (once) and bind every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C livetalking_amd/csrc`). livetalking_amd has no CPU fallback.")
    # PyTorch-ROCm first: it ships its own libamdhip64.so.7 / HSA runtime, the engine links against the system's by the same soname, and
    # whichever is mapped first serves both.  With the system's mapped first (this library loaded before `import torch`, e.g. build() and
    # smoke() in one process) the second runtime finds no device ("no ROCm-capable device is detected"); with torch's first everything -
    # torch's allocator and the engine's streams - shares one runtime.  The plugin needs torch for its device buffers anyway.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    other_build = bool(os.environ.get("LTK_LIB"))
    for name, (res, args) in SYMBOLS.items():
        if other_build and not hasattr(lib, name):      # an A/B against an older build: it lacks the hooks added since, bind what it has
            continue
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().ltk_last_error()
        raise LtkError(rc, msg.decode("utf-8", "replace") if msg else "")
