"""ctypes binding of libsdv_hip.so (C ABI: include/sdv_hip.h).

PyTorch is used for device memory and streams only: every wrapper takes torch tensors, checks
dtype/device/contiguity, and passes ``data_ptr()`` + the current HIP stream to the C entry point.
There is NO fallback: if the library is missing or a tensor is not on the GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

import torch

# SDV_HIP_LIB: developer knob - load an alternative build of the SAME C ABI (tools/ubench/build_whatif.py timing variants)
_LIB_PATH = Path(os.environ["SDV_HIP_LIB"]) if os.environ.get("SDV_HIP_LIB") else Path(__file__).resolve().parent / "lib" / "libsdv_hip.so"
_lib = None


class SdvHipError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("X2", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p),
        ("C", C.c_void_p), ("step_ptr", C.c_void_p), ("zero_page", C.c_void_p),
        ("sX", C.c_int64), ("sW", C.c_int64), ("sC", C.c_int64), ("sR", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("ldx", C.c_int32), ("ldx2", C.c_int32), ("C1", C.c_int32), ("ldw", C.c_int32), ("ldc", C.c_int32),
        ("ldr", C.c_int32),
        ("mode", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32),
        ("circular", C.c_int32),
        ("epi", C.c_int32), ("bias_mode", C.c_int32), ("bias_step_stride", C.c_int32),
        ("batch", C.c_int32), ("tile", C.c_int32), ("alpha", C.c_float),
        ("div_hw_mul", C.c_uint32), ("div_hw_shr", C.c_uint32), ("div_w_mul", C.c_uint32), ("div_w_shr", C.c_uint32),
        ("alpha_cols", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_s", C.c_void_p), ("stats_out", C.c_void_p), ("ln_side", C.c_int32), ("stats_p", C.c_int32),
        ("fp8", C.c_int32), ("out_mode", C.c_int32), ("out_f32", C.c_void_p), ("out_u8", C.c_void_p),
        ("gn_out", C.c_void_p), ("gn_ld", C.c_int32), ("split_k", C.c_int32),
    ]


ABI_VERSION = 12    # sdv_abi_version() of the library this binding (struct layouts, signatures) was written against


_SIGNATURES = {
    "sdv_last_error": (C.c_char_p, []),
    "sdv_abi_version": (C.c_int, []),
    "sdv_gemm_bf16": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "sdv_gemm_stats_slots": (C.c_int, [C.POINTER(GemmArgs)]),
    "sdv_gemm_split_k": (C.c_int, [C.POINTER(GemmArgs)]),
    "sdv_gemm_set_persistent": (C.c_int, [C.c_int]),
    "sdv_gemm_set_grid_limit": (C.c_int, [C.c_int]),
    "sdv_rowstats_finalize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "sdv_ffn_geglu_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]),
    "sdv_linear320_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_linear640_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_float, C.c_void_p]),
    "sdv_attention_bf16": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 9 + [C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_softmax_rows_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_softmax_rows_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_groupnorm_finalize": (C.c_int, ([C.c_void_p] + [C.c_int32] * 4 + [C.c_int64]) * 2 + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p]),
    "sdv_groupnorm_stats": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p]),
    "sdv_groupnorm_apply": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 3 +
                            [C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdv_groupnorm_apply_fp8": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 3 +
                                [C.c_float, C.c_int32, C.c_void_p, C.c_float, C.c_void_p]),
    "sdv_groupnorm_fp8_set_saturation_counter": (C.c_int, [C.c_void_p]),
    "sdv_layernorm_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdv_conv3x3_cin_small": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 6 + [C.c_void_p]),
    "sdv_im2col3x3_c4": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]),
    "sdv_latent_affine": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "sdv_slerp_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sdv_slerp_batch": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_float, C.c_void_p, C.c_void_p]),
    "sdv_lerp_batch": (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdv_cfg_ddim_step": (C.c_int, [C.c_void_p] * 6 + [C.c_float, C.c_int32, C.c_int64, C.c_void_p]),
    "sdv_cfg_multistep_step": (C.c_int, [C.c_void_p] * 8 + [C.c_float, C.c_int32, C.c_int64, C.c_void_p]),
    "sdv_latents_to_unet_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "sdv_step_counter_add": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "sdv_timestep_embedding": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                         C.c_void_p]),
    "sdv_linear_small": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]),
    "sdv_nchw_to_nhwc_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_nhwc_to_nchw_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_embed_tokens": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "sdv_rgb_u8_to_bf16_c4": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "sdv_axpby_bf16": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                 C.c_float, C.c_float, C.c_void_p]),
    "sdv_clip_preprocess_patches": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3 +
                                    [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]),
    "sdv_safety_screen": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdv_jpeg_transform_u8": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.c_void_p, C.c_void_p]),
    "sdv_jpeg_entropy_pack": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdv_png_filter_u8": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdv_png_deflate_pack": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sdv_png_deflate_lz_pack": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "sdv_png_crc32": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "sdv_h264_planes_u8": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 4),
    "sdv_h264_encode_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_encode_gops": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "sdv_h264_pack": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_int32] * 3 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sdv_h264_vlc_tables": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.c_int32]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
# include/sdv_hip_ext.h: additive codec extensions of ABI 12, exported by the same library and bound by load() with the table above
_EXT_SIGNATURES = {
    "sdv_h264_motion_search": (C.c_int, [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p] * 3),
    "sdv_h264_encode_gop_step": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 8 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
}
EXTENSION_SYMBOLS = tuple(_EXT_SIGNATURES)
# include/sdv_hip_h264_sub.h: the same pair with quarter-sample vectors (one more int32, ``subpel``, after ``search``)
_H264_SUB_SIGNATURES = {
    "sdv_h264_motion_search_sub": (C.c_int, [C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p] * 3),
    "sdv_h264_encode_gop_step_sub": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
}
H264_SUB_SYMBOLS = tuple(_H264_SUB_SIGNATURES)
# include/sdv_hip_h264_i4.h: the IDR pictures of a call with Intra4x4 prediction (the arguments of sdv_h264_encode_gops)
_H264_I4_SIGNATURES = {
    "sdv_h264_encode_idr4": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
}
H264_I4_SYMBOLS = tuple(_H264_I4_SIGNATURES)
# include/sdv_hip_h264_lf.h: the in-loop deblocking filter, and the three per-position entry points with (mbinfo, mbinfo_count) before the stream
_H264_LF_SIGNATURES = {
    "sdv_h264_encode_gop_step_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 8 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_encode_gop_step_sub_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_encode_idr4_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_deblock": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 7 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
}
H264_LF_SYMBOLS = tuple(_H264_LF_SIGNATURES)
# include/sdv_hip_h264_part.h: four vectors per macroblock (P_8x8): the search, the per-position pair and the filter, each with the element
# count of ``mv`` (and of ``sad`` / ``mbinfo``) after its pointer
_H264_PART_SIGNATURES = {
    "sdv_h264_motion_search_part": (C.c_int, [C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_encode_gop_step_part": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]),
    "sdv_h264_encode_gop_step_part_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 +
                                         [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "sdv_h264_deblock_part": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
}
H264_PART_SYMBOLS = tuple(_H264_PART_SIGNATURES)
# include/sdv_hip_h264_seg.h: several slices per macroblock row: the four-vector per-position pair and the Intra4x4 pair, each with ``segs``
# before the stream
_H264_SEG_SIGNATURES = {
    "sdv_h264_encode_gop_step_seg": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 +
                                     [C.c_int64, C.c_int32, C.c_void_p]),
    "sdv_h264_encode_gop_step_seg_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 9 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 +
                                        [C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "sdv_h264_encode_idr4_seg": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_void_p]),
    "sdv_h264_encode_idr4_seg_lf": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4 +
                                    [C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
}
H264_SEG_SYMBOLS = tuple(_H264_SEG_SIGNATURES)


def lib_path() -> Path:
    return _LIB_PATH


def load(build_if_missing: bool = False):
    """dlopen libsdv_hip.so and bind every symbol of include/sdv_hip.h.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        if build_if_missing:
            from . import build as _build
            _build.build()
        else:
            raise SdvHipError(
                f"{_LIB_PATH} is missing - build it with `python -m stable_diffusion_videos_amd.build` "
                "(there is no CPU / eager fallback for the hot path)")
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in {**_SIGNATURES, **_EXT_SIGNATURES, **_H264_SUB_SIGNATURES, **_H264_I4_SIGNATURES, **_H264_LF_SIGNATURES,
                              **_H264_PART_SIGNATURES, **_H264_SEG_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.sdv_abi_version() != ABI_VERSION:
        raise SdvHipError(f"{_LIB_PATH} reports ABI version {lib.sdv_abi_version()}, this binding needs {ABI_VERSION}: "
                          "rebuild it with `python -m stable_diffusion_videos_amd.build --force`")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.sdv_last_error().decode(errors="replace") if _lib is not None else ""
        raise SdvHipError(f"{what} failed (rc={rc}): {msg}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor], dtype=None, name="tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise SdvHipError(f"{name} must live in GPU memory (got device {t.device}); the HIP path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise SdvHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


BF16 = torch.bfloat16
F32 = torch.float32
FP8 = torch.float8_e4m3fn      # OCP e4m3, what gfx950's fp8 MFMA and converters use
FP8_MAX = 448.0

_zero_pages = {}
FP8_MX = int(os.environ.get("SDV_FP8_MX", "1"))            # developer knob for A/B: 0 = fp8 operands on the plain (bf16-rate) fp8 MFMA
# Test / tools knob: launches that leave the tile to the cost model (tile=0) are forced onto this tile where it exists for them
# (6 = the persistent 256 x 320 tile).  With it - and sdv_gemm_set_grid_limit - a 2-sample forward runs the SAME tile code paths as
# the 256-sample benchmark forward, so they can be put under the oracle's block-wise absolute gate (tests/test_blockwise_gpu.py).
FORCE_TILE = int(os.environ.get("SDV_FORCE_TILE", "0"))

# Optional launch observer used by bench.py's roofline pass: called as hook(kind, info_dict, launch_fn).  The
# hook must call launch_fn() itself (it may bracket it with HIP events).  None = no overhead.
LAUNCH_HOOK = None


def _launch(kind: str, info: dict, fn):
    if LAUNCH_HOOK is None:
        fn()
    else:
        LAUNCH_HOOK(kind, info, fn)


# ------------------------------------------------------------------------------------------------
# torch.ops.sdv.k_* : every launch on the hot path is a PyTorch custom op
# ------------------------------------------------------------------------------------------------
# BASELINE.json's north_star: "Python host code calling hand-written CDNA4 HIP kernels through PyTorch-ROCm custom ops".  The public
# wrappers below (gemm / linear / conv3x3 / attention / groupnorm / cfg_*_step / lerp / slerp ...) - which is what engine.py and
# pipeline.py call - do not touch ctypes themselves: they pack their arguments and call ``torch.ops.sdv.k_<name>``, a dispatcher
# op registered here with a schema (mutated outputs annotated), an implementation that hands ``data_ptr()`` + the current HIP
# stream to the C ABI, and a Meta (fake) kernel.  Registered through ``torch.library.Library`` rather than
# ``torch.library.custom_op``: 6 us per call instead of 31 us (measured), which matters for the ~400 launches of an eager UNet
# forward and not at all once a step is a hipGraph replay.  There is still no CPU kernel: the one implementation raises
# ``SdvHipError`` for a tensor that is not in GPU memory.
_OPLIB = torch.library.Library("sdv", "FRAGMENT")
KERNEL_OPS = []


def _defop(schema: str, impl, fake=None):
    name = schema[:schema.index("(")]
    _OPLIB.define(schema)
    _OPLIB.impl(name, impl, "CompositeExplicitAutograd")
    _OPLIB.impl(name, fake if fake is not None else (lambda *a, **k: None), "Meta")
    KERNEL_OPS.append(name)
    return getattr(torch.ops.sdv, name)


def zero_page(device) -> torch.Tensor:
    key = str(device)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(256, dtype=torch.uint8, device=device)
    return _zero_pages[key]


# ------------------------------------------------------------------------------------------------
# GEMM / conv
# ------------------------------------------------------------------------------------------------
_GEMM_INTS = ("M", "N", "K", "ldx", "ldw", "ldc", "ldr", "C1", "ldx2", "epi", "mode", "Hin", "Win", "Hout", "Wout", "circular", "batch",
              "sX", "sW", "sC", "sR", "bias_mode", "bias_step_stride", "tile", "x_off", "w_off", "out_off", "alpha_cols", "out_mode")


GN_EPILOGUE = os.environ.get("SDV_GN_EPILOGUE", "1") != "0"     # A/B knob: 0 = every GroupNorm runs its own statistics pass
SPLIT_K = os.environ.get("SDV_SPLIT_K", "1") != "0"             # A/B knob: 0 = no split-K launches (small-batch regime)
LAST_SPLIT_K = 1


class GnStats:
    """GroupNorm statistics that left the producing igemm's epilogue (sdv_gemm_args.gn_out): ``p`` fp32 [blocks, 2, C] of
    (sum, sumsq) per 32-row block and channel of a tensor of ``nimg`` images with ``HW`` pixels each; ``nrep`` repetitions
    ``rep_stride`` blocks apart (the four phases of a phase-form up-conv).  Travels as ``tensor._sdv_gn`` with the tensor the
    producer returned; ``groupnorm`` uses it instead of a statistics pass when it matches what it is asked to normalise - same
    geometry AND the tensor's version counter still where it was when the statistics were attached (``ver``): any in-place torch
    writer since (``copy_``, ``add_``, an ``out=`` op) makes ``groupnorm`` fall back to its own statistics pass."""
    __slots__ = ("p", "C", "nimg", "HW", "bpi", "nrep", "rep_stride", "ver")

    def __init__(self, p, C, nimg, HW, bpi, nrep, rep_stride, ver=-1):
        self.p, self.C, self.nimg, self.HW, self.bpi, self.nrep, self.rep_stride, self.ver = p, C, nimg, HW, bpi, nrep, rep_stride, ver


def _ver(t: torch.Tensor) -> int:
    try:
        return t._version
    except RuntimeError:          # inference tensors do not track versions: nothing to compare, the geometry check stands alone
        return -1


def gn_repeat(t_src: torch.Tensor, t_dst: torch.Tensor, times: int):
    """``t_dst`` holds ``times`` copies of ``t_src``'s images back to back (the CFG-shared skip tensor): its statistics are the
    source's, repeated."""
    g = getattr(t_src, "_sdv_gn", None)
    if g is not None and g.nrep == 1:
        t_dst._sdv_gn = GnStats(torch.cat([g.p] * times), g.C, g.nimg * times, g.HW, g.bpi, 1, 0, _ver(t_dst))


def gn_slice(t: torch.Tensor, first_img: int, n_img: int, HW: int) -> torch.Tensor:
    """Rows of images [first_img, first_img + n_img) of ``t`` - with the matching slice of its epilogue statistics, so that a
    forward that walks the batch in chunks of images normalises with exactly the numbers the whole-batch forward uses."""
    out = t[first_img * HW:(first_img + n_img) * HW]
    g = getattr(t, "_sdv_gn", None)
    if g is not None and g.HW == HW:
        if g.nrep == 1:
            p = g.p[first_img * g.bpi:(first_img + n_img) * g.bpi]
            out._sdv_gn = GnStats(p, g.C, n_img, HW, g.bpi, 1, 0, g.ver)
        else:
            p = g.p.view(g.nrep, g.rep_stride, 2, g.C)[:, first_img * g.bpi:(first_img + n_img) * g.bpi].contiguous()
            out._sdv_gn = GnStats(p.view(-1, 2, g.C), g.C, n_img, HW, g.bpi, g.nrep, n_img * g.bpi, g.ver)
    return out


def gn_join(parts, whole: torch.Tensor):
    """The statistics of ``whole`` from those of its consecutive image chunks ``parts`` (all produced with nrep == 1)."""
    gs = [getattr(t, "_sdv_gn", None) for t in parts]
    if gs and all(g is not None and g.nrep == 1 for g in gs):
        whole._sdv_gn = GnStats(torch.cat([g.p for g in gs]), gs[0].C, sum(g.nimg for g in gs), gs[0].HW, gs[0].bpi, 1, 0, _ver(whole))


def gn_epilogue_ok(*, M, N, epi, mode, ldc, ldr, out, bias, residual, fp8, ln, want_stats, out_mode, HW_out, batch, sC, sR) -> bool:
    """Can this igemm launch emit the GroupNorm statistics of its output (sdv_hip.h gn_out)?  ``HW_out``: pixels per image of the
    OUTPUT tensor.  Mirrors the checks of sdv_gemm_bf16."""
    if not GN_EPILOGUE or epi != 0 or out_mode or fp8 or ln is not None or want_stats or out is None:
        return False
    rows_per_image = HW_out // 4 if mode == 4 else HW_out           # rows of ONE launch phase that belong to one image
    if M % 32 or rows_per_image % 32 or N % 8 or ldc % 8 or (residual is not None and ldr % 8) or (sC | sR) % 8:
        return False
    ptrs = out.data_ptr() | (bias.data_ptr() if bias is not None else 0) | (residual.data_ptr() if residual is not None else 0)
    return ptrs % 16 == 0


def _igemm_impl(x, w, out, bias, residual, x2, ln_stats, ln_s, step_ptr, out_f32, out_u8, gn_out, ints, alpha, ln_eps, want_stats):
    """sdv::k_igemm - the launch of ``sdv_gemm_bf16`` (+ ``sdv_rowstats_finalize`` when the row statistics are wanted)."""
    g = dict(zip(_GEMM_INTS, ints))
    M, N, K, batch, mode, epi = g["M"], g["N"], g["K"], g["batch"], g["mode"], g["epi"]
    lib = load()
    a = GemmArgs()
    fp8 = x.dtype == FP8
    if fp8:
        if w.dtype != FP8 or (x2 is not None and x2.dtype != FP8) or g["x_off"] or g["w_off"]:
            raise SdvHipError("gemm: fp8 activations need fp8 weights (and no operand offsets)")
        # 2 = the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 form (twice the MFMA rate; sdv_hip.h), 1 = v_mfma_f32_32x32x16_fp8_fp8
        a.fp8 = 2 if FP8_MX else 1
        a.X, a.X2, a.W = _ptr(x, FP8, "X"), _ptr(x2, FP8, "X2"), _ptr(w, FP8, "W")
    else:
        a.X = _ptr(x, BF16, "X") + 2 * g["x_off"]
        a.X2 = _ptr(x2, BF16, "X2")
        a.W = _ptr(w, BF16, "W") + 2 * g["w_off"]
    a.bias = _ptr(bias, F32, "bias")
    a.R = _ptr(residual, BF16, "R")
    a.C = _ptr(out, BF16, "C") + 2 * g["out_off"] if out is not None else None
    a.out_mode, a.out_f32, a.out_u8 = g["out_mode"], _ptr(out_f32, F32, "out_f32"), _ptr(out_u8, torch.uint8, "out_u8")
    a.step_ptr = _ptr(step_ptr, torch.int32, "step_ptr")
    a.zero_page = zero_page(x.device).data_ptr()
    a.sX, a.sW, a.sC, a.sR = g["sX"], g["sW"], g["sC"], g["sR"]
    a.M, a.N, a.K = M, N, K
    a.ldx, a.ldx2, a.C1, a.ldw, a.ldc, a.ldr = g["ldx"], g["ldx2"], g["C1"], g["ldw"], g["ldc"], g["ldr"]
    a.mode, a.Hin, a.Win, a.Hout, a.Wout, a.circular = mode, g["Hin"], g["Win"], g["Hout"], g["Wout"], g["circular"]
    a.epi, a.bias_mode, a.bias_step_stride = epi, (g["bias_mode"] if bias is not None else 0), g["bias_step_stride"]
    a.batch, a.tile, a.alpha, a.alpha_cols = batch, g["tile"], alpha, g["alpha_cols"]
    if FORCE_TILE and not g["tile"] and not g["out_mode"] and epi < 3:
        a.tile = FORCE_TILE
    if ln_stats is not None:
        a.ln_stats, a.ln_s, a.ln_side = _ptr(ln_stats, F32, "ln_stats"), _ptr(ln_s, F32, "ln_s"), 1
    if gn_out is not None:
        a.gn_out, a.gn_ld = _ptr(gn_out, F32, "gn_out"), gn_out.shape[-1]
    split_used = False
    # Split-K for the small-batch regime (sdv_hip.h split_k): plain launches with few rows and a long K ask the library how many
    # splits it would take and hand it the workspace (the GroupNorm statistics, if asked for, then come out of the second pass).
    # (alpha_cols - alpha on the leading columns only - is not something the second pass knows: such launches stay unsplit)
    if (SPLIT_K and not fp8 and ln_stats is None and not want_stats and not g["out_mode"] and epi == 0 and batch <= 1 and mode != 4
            and out_f32 is None and not g["alpha_cols"] and M <= 4096 and K * (1 if mode == 0 else 9) >= 2048):
        a.split_k = 8
        S = lib.sdv_gemm_split_k(C.byref(a))
        if S > 1:
            ws = torch.empty((S, M, N), dtype=F32, device=x.device)
            a.out_f32, a.split_k = ws.data_ptr(), S
            split_used = True
        else:
            a.split_k = 0
    global LAST_SPLIT_K
    LAST_SPLIT_K = a.split_k if split_used else 1    # (tests / tools: how the last igemm launch was split)
    partials = None
    if want_stats:
        a.stats_out = 16          # (non-null while planning: the tile choice depends on it)
        slots = lib.sdv_gemm_stats_slots(C.byref(a))
        if slots <= 0:
            _check(-1, "sdv_gemm_stats_slots")
        partials = torch.empty((max(batch, 1) * M, slots, 2), dtype=F32, device=x.device)
        a.stats_out = partials.data_ptr()
    taps = 1 if mode == 0 else 9
    # algorithmic work: the phase form (mode 4) is a nearest-2x upsample + conv3x3 on 4*M output pixels (9 taps each);
    # it EXECUTES 4 taps per output pixel
    flops = 2.0 * M * N * K * taps * (4 if mode == 4 else batch)
    _launch("gemm" if mode == 0 else "conv3x3",
            dict(M=M * (4 if mode == 4 else 1), N=N, K=K * taps, batch=batch, flops=flops, mode=mode, epi=epi),
            lambda: _check(lib.sdv_gemm_bf16(C.byref(a), _stream()), "sdv_gemm_bf16"))
    if want_stats:
        nout = N // 2 if epi == 1 else N
        stats = torch.empty((max(batch, 1) * M, 2), dtype=F32, device=x.device)
        _launch("ln_stats", dict(bytes=8.0 * partials.shape[0] * (partials.shape[1] + 1)),
                lambda: _check(lib.sdv_rowstats_finalize(partials.data_ptr(), partials.shape[0], partials.shape[1], nout, ln_eps,
                                                         stats.data_ptr(), _stream()), "sdv_rowstats_finalize"))
        return stats
    return torch.empty(0, dtype=F32, device=x.device)


def _igemm_fake(x, w, out, bias, residual, x2, ln_stats, ln_s, step_ptr, out_f32, out_u8, gn_out, ints, alpha, ln_eps, want_stats):
    g = dict(zip(_GEMM_INTS, ints))
    return x.new_empty((max(g["batch"], 1) * g["M"], 2) if want_stats else (0,), dtype=F32)


_k_igemm = _defop("k_igemm(Tensor x, Tensor w, Tensor(a!)? out, Tensor? bias, Tensor? residual, Tensor? x2, Tensor? ln_stats, "
                  "Tensor? ln_s, Tensor? step_ptr, Tensor(b!)? out_f32, Tensor(c!)? out_u8, Tensor(d!)? gn_out, int[] ints, float alpha, "
                  "float ln_eps, bool want_stats) -> Tensor", _igemm_impl, _igemm_fake)


def gemm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int, ldx: int, ldw: int,
         ldc: int, bias: Optional[torch.Tensor] = None, bias_mode: int = 1, residual: Optional[torch.Tensor] = None,
         ldr: int = 0, x2: Optional[torch.Tensor] = None, C1: int = 0, ldx2: int = 0, alpha: float = 1.0,
         epi: int = 0, mode: int = 0, Hin: int = 0, Win: int = 0, Hout: int = 0, Wout: int = 0,
         circular: bool = False, batch: int = 1, sX: int = 0, sW: int = 0, sC: int = 0, sR: int = 0,
         step_ptr: Optional[torch.Tensor] = None, bias_step_stride: int = 0, tile: int = 0,
         x_off: int = 0, w_off: int = 0, out_off: int = 0, alpha_cols: int = 0, ln=None,
         want_stats: bool = False, ln_eps: float = 1e-5, out_mode: int = 0, out_f32: Optional[torch.Tensor] = None,
         out_u8: Optional[torch.Tensor] = None, gn_hw: int = 0):
    """``sdv_gemm_bf16`` through ``torch.ops.sdv.k_igemm`` (element offsets x_off / w_off / out_off select sub-matrices).
    ``out`` / ``residual`` may be windows of wider buffers; what alignment they need follows from ldc / ldr (sdv_hip.h "C / R":
    ``sdv_gemm_bf16`` refuses a launch that breaks it - ``SdvHipError``, nothing launched).
    ``out_mode`` 1 / 2: fp32 output / image epilogue into ``out_f32`` / ``out_u8`` (``out`` may be None), see sdv_hip.h.
    ``ln=(stats, s)``: LayerNorm folded into this GEMM (sdv_hip.h): ``stats`` fp32 [rows, 2] = (mean, rstd) from
    ``want_stats`` of the producer, ``s`` fp32 row sums of the gamma-scaled weights.  ``want_stats=True`` returns the
    (mean, rstd) [batch*M, 2] of this GEMM's OUTPUT rows over its N columns (for the next LayerNorm).
    ``gn_hw`` > 0: the output is an NHWC image tensor with ``gn_hw`` pixels per image whose next consumer is a GroupNorm - where the
    launch qualifies (``gn_epilogue_ok``) the epilogue also emits the per-channel statistics and ``out._sdv_gn`` carries them."""
    ints = [M, N, K, ldx, ldw, ldc, ldr, C1, ldx2, epi, mode, Hin, Win, Hout, Wout, int(circular), batch, sX, sW, sC, sR, bias_mode,
            bias_step_stride, tile, x_off, w_off, out_off, alpha_cols, out_mode]
    gn_out = None
    nb = max(batch, 1)
    if gn_hw and out_off == 0 and gn_epilogue_ok(M=M, N=N, epi=epi, mode=mode, ldc=ldc, ldr=ldr, out=out, bias=bias, residual=residual,
                                                 fp8=x.dtype == FP8, ln=ln, want_stats=want_stats, out_mode=out_mode, HW_out=gn_hw,
                                                 batch=batch, sC=sC, sR=sR):
        nrep = 4 if mode == 4 else 1
        rows = nb * M if mode != 4 else M                       # rows of one repetition
        gn_out = torch.empty((nrep * rows // 32, 2, N), dtype=F32, device=x.device)
    st = _k_igemm(x, w, out, bias, residual, x2, ln[0] if ln is not None else None, ln[1] if ln is not None else None, step_ptr,
                  out_f32, out_u8, gn_out, ints, float(alpha), float(ln_eps), bool(want_stats))
    if gn_out is not None:
        rows_per_image = gn_hw // 4 if mode == 4 else gn_hw
        nimg = (M if mode == 4 else nb * M) // rows_per_image
        out._sdv_gn = GnStats(gn_out, N, nimg, gn_hw, rows_per_image // 32, 4 if mode == 4 else 1, (M // 32) if mode == 4 else 0, _ver(out))
    elif out is not None and hasattr(out, "_sdv_gn"):
        del out._sdv_gn
    return st if want_stats else None


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, residual=None, out=None,
           epi: int = 0, x2: Optional[torch.Tensor] = None, alpha: float = 1.0, tile: int = 0, alpha_cols: int = 0, ln=None,
           want_stats: bool = False, ln_eps: float = 1e-5, gn_hw: int = 0):
    """y[M,N] = epi(x[M,K] @ w[N,K]^T + bias) (+ residual); x2 = optional second K-source (concat).
    ``ln`` / ``want_stats``: see ``gemm`` (with want_stats the return value is ``(y, stats)``)."""
    M, K1 = x.shape
    K2 = x2.shape[1] if x2 is not None else 0
    N, K = w.shape
    if K != K1 + K2:
        raise SdvHipError(f"linear: K mismatch {K} vs {K1}+{K2}")
    n_out = N // 2 if epi == 1 else N
    if out is None:
        out = torch.empty((M, n_out), dtype=BF16, device=x.device)
    st = gemm(x, w, out, M=M, N=N, K=K, ldx=x.stride(0), ldw=w.stride(0), ldc=out.stride(0), bias=bias,
              residual=residual, ldr=residual.stride(0) if residual is not None else 0, x2=x2, C1=K1 if x2 is not None else 0,
              ldx2=x2.stride(0) if x2 is not None else 0, alpha=alpha, epi=epi, tile=tile, alpha_cols=alpha_cols, ln=ln,
              want_stats=want_stats, ln_eps=ln_eps, gn_hw=gn_hw)
    return (out, st) if want_stats else out


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, nimg: int, H: int, W: int,
            mode: int = 1, x2: Optional[torch.Tensor] = None, residual=None, circular: bool = False,
            step_ptr=None, bias_step_stride: int = 0, out=None, tile: int = 0, epi: int = 0,
            alpha: float = 1.0, out_mode: int = 0, out_f32=None, out_u8=None, gn: bool = False) -> torch.Tensor:
    """NHWC conv3x3 pad 1.  x: [nimg*H*W, C1] (+ x2 [.., C2]); w: [Cout, 9*(C1+C2)] (OHWI).
    mode 1: stride 1; 2: stride 2; 3: nearest-2x upsample then conv.  x / out / residual may be column
    slices of wider row-major buffers (row stride = .stride(0)): dense-block concat without copies.
    ``out_mode`` 1: fp32 result in ``out_f32`` [M, Cout]; 2: image epilogue (clamp(v/2+0.5), fp32 in ``out_f32`` and / or
    uint8 in ``out_u8``) - the Cout <= 4 output convolutions of the UNet / VAE on the matrix cores; nothing is returned."""
    C1 = x.shape[1]
    C2 = x2.shape[1] if x2 is not None else 0
    Cout = w.shape[0]
    if w.shape[1] != 9 * (C1 + C2):
        raise SdvHipError(f"conv3x3: weight K {w.shape[1]} != 9*{C1 + C2}")
    if mode == 4:
        return upconv3x3_phase(x, w, bias, nimg=nimg, H=H, W=W, circular=circular, out=out, tile=tile, gn=gn)
    if mode == 1:
        Ho, Wo = H, W
    elif mode == 2:
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
    else:
        Ho, Wo = 2 * H, 2 * W
    M = nimg * Ho * Wo
    if out_mode:
        if (out_f32 is None and out_u8 is None) or out is not None or residual is not None:
            raise SdvHipError("conv3x3: out_mode needs out_f32 / out_u8 (and takes no bf16 output / residual)")
        ldc = Cout
    else:
        if out is None:
            out = torch.empty((M, Cout), dtype=BF16, device=x.device)
        ldc = out.stride(0)
    gemm(x, w, out, M=M, N=Cout, K=C1 + C2, ldx=x.stride(0), ldw=w.stride(0), ldc=ldc, bias=bias,
         residual=residual, ldr=residual.stride(0) if residual is not None else 0, x2=x2,
         C1=C1 if x2 is not None else 0, ldx2=x2.stride(0) if x2 is not None else 0, mode=mode, Hin=H, Win=W,
         Hout=Ho, Wout=Wo, circular=circular, step_ptr=step_ptr, bias_step_stride=bias_step_stride, tile=tile,
         epi=epi, alpha=alpha, out_mode=out_mode, out_f32=out_f32, out_u8=out_u8, gn_hw=Ho * Wo if gn else 0)
    return out


def upconv3x3_phase(x: torch.Tensor, w4: torch.Tensor, bias: Optional[torch.Tensor], *, nimg: int, H: int, W: int,
                    circular: bool = False, out=None, tile: int = 0, gn: bool = False) -> torch.Tensor:
    """Upsample2D (nearest 2x, then conv3x3 pad 1) in phase form: x [nimg*H*W, Cin] -> [nimg*2H*2W, Cout].
    ``w4``: [4*Cout, 4*Cin] from ``weights.upconv_phase_w`` (phase-major; 2x2 taps with the coincident 3x3 taps summed)."""
    Cin = x.shape[1]
    if w4.shape[0] % 4 or w4.shape[1] != 4 * Cin:
        raise SdvHipError(f"upconv3x3_phase: weight shape {tuple(w4.shape)} does not match Cin={Cin}")
    Cout = w4.shape[0] // 4
    if out is None:
        out = torch.empty((nimg * 4 * H * W, Cout), dtype=BF16, device=x.device)
    gemm(x, w4, out, M=nimg * H * W, N=Cout, K=Cin, ldx=x.stride(0), ldw=w4.stride(0), ldc=out.stride(0), bias=bias, mode=4,
         Hin=H, Win=W, Hout=H, Wout=W, circular=circular, tile=tile, gn_hw=4 * H * W if gn else 0)
    return out


# ------------------------------------------------------------------------------------------------
# attention / norms
# ------------------------------------------------------------------------------------------------
def _attention_impl(q, k, vt, out, ints, scale, causal, q_prescaled, v_rowmajor):
    B, H, Lq, Lk, dh, ldq, ldk, ldv, ldo, q_off, k_off, v_off = ints
    lib = load()
    qp, kp, op = _ptr(q, BF16, "Q") + 2 * q_off, _ptr(k, BF16, "K") + 2 * k_off, _ptr(out, BF16, "O")
    vp = _ptr(vt, BF16, "V") + 2 * v_off
    _launch("attention", dict(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, flops=4.0 * B * H * Lq * Lk * dh),
            lambda: _check(lib.sdv_attention_bf16(qp, kp, vp, op, B, H, Lq, Lk, dh, ldq, ldk, ldv, ldo, scale, int(causal),
                                                  int(q_prescaled), int(v_rowmajor), _stream()),
                           "sdv_attention_bf16"))


_k_attention = _defop("k_attention(Tensor q, Tensor k, Tensor vt, Tensor(a!) out, int[] ints, float scale, bool causal, "
                      "bool q_prescaled, bool v_rowmajor) -> ()", _attention_impl)


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, *, B: int, H: int, Lq: int,
              Lk: int, dh: int, ldq: int, ldk: int, ldv: int, ldo: int, scale: float, q_off: int = 0, k_off: int = 0,
              v_off: int = 0, causal: bool = False, q_prescaled: bool = False, v_rowmajor: bool = False):
    """softmax(Q K^T scale) V (``torch.ops.sdv.k_attention``).  ``q_prescaled``: Q already holds q * scale * log2(e)
    (``LOG2E_SCALE(dh)`` applied as the ``alpha`` of its projection GEMM, one bf16 rounding in total) and ``scale`` is ignored.
    ``vt``: V transposed [B][H*dh][ldv] (the text context's V^T) or, with ``v_rowmajor``, V as a projection wrote it -
    [B*Lk][ldv] rows, head h at columns v_off + [h*dh, (h+1)*dh): the V third of a fused [Q | K | V] projection."""
    _k_attention(q, k, vt, out, [B, H, Lq, Lk, dh, ldq, ldk, ldv, ldo, q_off, k_off, v_off], float(scale), bool(causal),
                 bool(q_prescaled), bool(v_rowmajor))


def _ffn_geglu_impl(x, ln_stats, w1, w1x, w2p, bias2, out):
    lib = load()
    M, C = x.shape
    if tuple(w1.shape) != (8 * C, C) or tuple(w1x.shape) != (8 * C, 16) or tuple(w2p.shape) != (C, 4 * C) or not (
            w1.is_contiguous() and w1x.is_contiguous() and w2p.is_contiguous()):
        raise SdvHipError(f"ffn_geglu: weights must be contiguous [8C, C] / [8C, 16] / [C, 4C] for C = {C}, got {tuple(w1.shape)} / "
                          f"{tuple(w1x.shape)} / {tuple(w2p.shape)}")
    if ln_stats.numel() != 2 * M or bias2.numel() != C or out.shape != x.shape:
        raise SdvHipError("ffn_geglu: vector / output sizes do not match the activation")
    args = (_ptr(x, BF16, "X"), _ptr(ln_stats, F32, "ln_stats"), M, C, x.stride(0), _ptr(w1, BF16, "W1"), _ptr(w1x, BF16, "W1x"),
            _ptr(w2p, BF16, "W2p"), _ptr(bias2, F32, "bias2"), _ptr(out, BF16, "out"), out.stride(0))
    # algorithmic work: both projections (2 M (8C C + C 4C)); bytes: x in, out back (the hidden activations never touch HBM)
    _launch("ffn_geglu", dict(M=M, N=8 * C, K=C, flops=2.0 * M * 12 * C * C, bytes=4.0 * M * C),
            lambda: _check(lib.sdv_ffn_geglu_bf16(*args, _stream()), "sdv_ffn_geglu_bf16"))


_k_ffn_geglu = _defop("k_ffn_geglu(Tensor x, Tensor ln_stats, Tensor w1, Tensor w1x, Tensor w2p, Tensor bias2, Tensor(a!) out) -> ()", _ffn_geglu_impl)
FFN_FUSED = os.environ.get("SDV_FFN_FUSED", "1") != "0"     # A/B knob: 0 = the C = 320 feed-forward as two igemm launches (round 5)


def ffn_geglu(x: torch.Tensor, ln_stats: torch.Tensor, w1: torch.Tensor, w1x: torch.Tensor, w2p: torch.Tensor, bias2: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x + ff.net.2(GEGLU(ff.net.0(LayerNorm(x)))) in ONE launch (``torch.ops.sdv.k_ffn_geglu`` -> sdv_ffn_geglu_bf16, C = 320 only).
    ``w1``: the gamma-folded, GEGLU-interleaved ff.net.0 weight of ``weights.ln_fold(weights.geglu_interleave(...))``; ``w1x``:
    ``weights.ffn_fold_columns(s, t)`` of the same call; ``w2p``: ``weights.ffn_w2_permute(ff.net.2.weight)``; ``ln_stats`` [M, 2]:
    (mean, rstd) of the rows of ``x`` (the producer's ``want_stats``)."""
    if out is None:
        out = torch.empty_like(x)
    _k_ffn_geglu(x, ln_stats, w1, w1x, w2p, bias2, out)
    return out


def _linear320_impl(x, w, wx, ln_stats, alpha, residual, out, stats_out, eps, vt, hw):
    lib = load()
    M, N = x.shape[0], w.shape[0]
    if x.shape[1] != 320 or w.shape[1] != 320 or tuple(wx.shape) != (N, 16) or not (w.is_contiguous() and wx.is_contiguous()):
        raise SdvHipError(f"linear320: x [M, 320], w [N, 320], wx [N, 16] contiguous expected, got {tuple(x.shape)} / {tuple(w.shape)} / {tuple(wx.shape)}")
    if alpha is not None and alpha.numel() != N // 320:
        raise SdvHipError("linear320: alpha holds one factor per block of 320 output columns")
    args = (_ptr(x, BF16, "X"), M, x.stride(0), _ptr(w, BF16, "W"), _ptr(wx, BF16, "Wx"), N, _ptr(ln_stats, F32, "ln_stats"), _ptr(alpha, F32, "alpha"),
            _ptr(residual, BF16, "R"), residual.stride(0) if residual is not None else 0, _ptr(out, BF16, "out"), out.stride(0),
            _ptr(stats_out, F32, "stats_out"), float(eps), _ptr(vt, BF16, "Vt"), vt.stride(1) if vt is not None else 0, int(hw))
    if vt is not None and (vt.dim() != 3 or vt.shape[0] * hw != M or vt.shape[1] != 320 or vt.stride(2) != 1 or vt.stride(0) != 320 * vt.stride(1)):
        raise SdvHipError(f"linear320: vt must be [M / hw, 320, ldv] with unit token stride, got {tuple(vt.shape)} / strides {vt.stride()}")
    nbytes = 2.0 * M * (320 + N + (320 if residual is not None else 0))
    _launch("linear320", dict(M=M, N=N, K=320, flops=2.0 * M * N * 320, bytes=nbytes),
            lambda: _check(lib.sdv_linear320_bf16(*args, _stream()), "sdv_linear320_bf16"))


_k_linear320 = _defop("k_linear320(Tensor x, Tensor w, Tensor wx, Tensor? ln_stats, Tensor? alpha, Tensor? residual, Tensor(a!) out, Tensor(b!)? stats_out, "
                      "float eps, Tensor(c!)? vt, int hw) -> ()", _linear320_impl)
def _linear640_impl(x, w, wx, ln_stats, alpha, out, stats_out, eps):
    lib = load()
    M, N = x.shape[0], w.shape[0]
    if x.shape[1] != 640 or w.shape[1] != 640 or tuple(wx.shape) != (N, 16) or not (w.is_contiguous() and wx.is_contiguous()):
        raise SdvHipError(f"linear640: x [M, 640], w [N, 640], wx [N, 16] contiguous expected, got {tuple(x.shape)} / {tuple(w.shape)} / {tuple(wx.shape)}")
    if alpha is not None and alpha.numel() != N // 320:
        raise SdvHipError("linear640: alpha holds one factor per block of 320 output columns")
    args = (_ptr(x, BF16, "X"), M, x.stride(0), _ptr(w, BF16, "W"), _ptr(wx, BF16, "Wx"), N, _ptr(ln_stats, F32, "ln_stats"), _ptr(alpha, F32, "alpha"),
            _ptr(out, BF16, "out"), out.stride(0), _ptr(stats_out, F32, "stats_out"), float(eps))
    _launch("linear320", dict(M=M, N=N, K=640, flops=2.0 * M * N * 640, bytes=2.0 * M * (640 + N)),
            lambda: _check(lib.sdv_linear640_bf16(*args, _stream()), "sdv_linear640_bf16"))


_k_linear640 = _defop("k_linear640(Tensor x, Tensor w, Tensor wx, Tensor? ln_stats, Tensor? alpha, Tensor(a!) out, Tensor(b!)? stats_out, float eps) -> ()",
                      _linear640_impl)
LINEAR640 = os.environ.get("SDV_LINEAR640", "1") != "0"     # A/B knob: 0 = the residual-free C = 640 projections stay on the igemm tiles
# Rows (of the WHOLE call: samples x pixels of the level, so that the CFG-shared prefix and the unshared forward choose alike) below which
# a persistent panel kernel leaves most CUs idle and the igemm's small tiles win (tools/r6_small.sh, profiles/round6_small_batches.txt):
# the fused feed-forward, the C = 640 fused Q K V projection, the other C = 640 projections.  hip.FORCE_TILE - "run what the big batch
# runs" (bench.py's parity check, the forced-tile tests) - overrides them: a forced forward takes the panel kernels at any size.
PANEL_MIN_ROWS_FFN = int(os.environ.get("SDV_PANEL_MIN_ROWS_FFN", "16384"))
PANEL_MIN_ROWS_QKV640 = int(os.environ.get("SDV_PANEL_MIN_ROWS_QKV640", "32768"))
PANEL_MIN_ROWS_LIN640 = int(os.environ.get("SDV_PANEL_MIN_ROWS_LIN640", "8192"))
LINEAR320 = os.environ.get("SDV_LINEAR320", "1") != "0"     # A/B knob: 0 = the C = 320 projections on the igemm tiles (round 5)
QKV_VT = os.environ.get("SDV_QKV_VT", "1") != "0"           # A/B knob: 0 = V stays row-major in the fused [Q | K | V] buffer


def linear320(x: torch.Tensor, w: torch.Tensor, wx: torch.Tensor, *, ln_stats=None, alpha=None, residual=None, out=None, want_stats: bool = False,
              eps: float = 1e-5, stats_out=None, vt=None, hw: int = 0):
    """A C = 320 (or, residual-free, C = 640: ``k_linear640`` -> sdv_linear640_bf16, N = 640 / 1920) projection on the panel kernel
    (``torch.ops.sdv.k_linear320`` -> sdv_linear320_bf16): N = 320 or 960 output
    columns, bias / LayerNorm fold in ``wx`` (``weights.ffn_fold_columns(s, t)``), optional per-320-column ``alpha``, residual and the
    LayerNorm statistics of the stored rows (returned as ``(y, stats [M, 2])`` with ``want_stats``).  ``vt`` [M / hw, 320, ldv]
    (N = 960): the V third is stored transposed per sample of ``hw`` tokens and ``out`` [M, 640] holds only [Q | K]."""
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, w.shape[0] if vt is None else 640), dtype=BF16, device=x.device)
    st = (stats_out if stats_out is not None else torch.empty((M, 2), dtype=F32, device=x.device)) if want_stats else None
    if w.shape[1] == 640:      # the C = 640 form (sdv_linear640_bf16): N = 640 or 1920, no residual, no transposed V
        if residual is not None or vt is not None:
            raise SdvHipError("linear320: the K = 640 form takes neither a residual nor a transposed V output")
        _k_linear640(x, w, wx, ln_stats, alpha, out, st, float(eps))
    else:
        _k_linear320(x, w, wx, ln_stats, alpha, residual, out, st, float(eps), vt, int(hw))
    return (out, st) if want_stats else out


_fp8_sat_ref: Optional[torch.Tensor] = None


def _fp8_saturation_counter_impl(counter: Optional[torch.Tensor]):
    if counter is not None and (counter.dtype != torch.int32 or not counter.is_cuda or counter.numel() != 1):
        raise SdvHipError("fp8 saturation counter: one int32 element in GPU memory")
    _check(load().sdv_groupnorm_fp8_set_saturation_counter(counter.data_ptr() if counter is not None else None),
           "sdv_groupnorm_fp8_set_saturation_counter")
    global _fp8_sat_ref
    _fp8_sat_ref = counter      # the library holds a raw device pointer: keep the tensor alive for as long as it is registered


def set_fp8_saturation_counter(counter: Optional[torch.Tensor]):
    """Debug aid of the fp8 path: while a one-element int32 device tensor is registered, every e4m3 GroupNorm apply adds the number
    of elements it had to clamp at +-448 to it (None switches it off).  Register it before a step is captured into a hipGraph."""
    _fp8_saturation_counter_impl(counter)


def q_prescale(dh: int) -> float:
    """softmax scale * log2(e): what the attention kernels want Q multiplied by (they exponentiate in base 2)."""
    return dh ** -0.5 * 1.4426950408889634


def _softmax_rows_impl(s, rows, cols, ld):
    lib = load()
    _check(lib.sdv_softmax_rows_bf16(_ptr(s, BF16, "S"), rows, cols, ld, _stream()), "sdv_softmax_rows_bf16")


_k_softmax_rows = _defop("k_softmax_rows_(Tensor(a!) s, int rows, int cols, int ld) -> ()", _softmax_rows_impl)


def softmax_rows_(s: torch.Tensor, rows: int, cols: int, ld: int):
    _k_softmax_rows(s, rows, cols, ld)


def _softmax_rows_f32_impl(s, p, rows, cols, lds, ldp):
    lib = load()
    _launch("softmax_rows", dict(bytes=(2 * 4.0 + 2.0) * rows * cols),
            lambda: _check(lib.sdv_softmax_rows_f32(_ptr(s, F32, "S"), _ptr(p, BF16, "P"), rows, cols, lds, ldp, _stream()),
                           "sdv_softmax_rows_f32"))


_k_softmax_rows_f32 = _defop("k_softmax_rows_f32(Tensor s, Tensor(a!) p, int rows, int cols, int lds, int ldp) -> ()", _softmax_rows_f32_impl)


def softmax_rows_f32(s: torch.Tensor, p: torch.Tensor, rows: int, cols: int, lds: int, ldp: int):
    """bf16 probabilities ``p`` = softmax over each fp32 row of ``s`` (``torch.ops.sdv.k_softmax_rows_f32``)."""
    _k_softmax_rows_f32(s, p, rows, cols, lds, ldp)


def gn_splits(HW: int) -> int:
    """Pixel ranges the statistics pass cuts an image into.  The apply pass re-reduces the partials in every block, so it
    wants few of them, the statistics pass wants enough blocks to fill the chip: 256 pixels per split at the 64 x 64 level
    and above, 128 at 32 x 32, 64 below (tools/gn_bench.py at 128 samples: apply 152 -> 114 us on 64^2 x 320 channels)."""
    pix = 256 if HW >= 4096 else (128 if HW >= 1024 else 64)
    return max(1, min(64, HW // pix))


def _groupnorm_impl(x, gamma, beta, x2, out, p1, p2, ints, eps, fp8_scale):
    nimg, HW, groups, silu, bpi1, nrep1, rs1, bpi2, nrep2, rs2 = ints
    lib = load()
    C1 = x.shape[1]
    C2 = x2.shape[1] if x2 is not None else 0
    if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
        raise SdvHipError("groupnorm: inputs must be contiguous")
    fp8 = fp8_scale > 0.0
    nbytes = 2.0 * nimg * HW * (C1 + C2)
    if p1 is not None:
        # statistics from the producers' epilogues (sdv_gemm_args.gn_out): only their per-block partials are read
        splits = max(1, min(64, (bpi1 * nrep1) // 16))          # 16 of an image's 32-row blocks per finalize workgroup
        partials = torch.empty((nimg, splits, groups, 2), dtype=F32, device=x.device)
        pp = _ptr(partials)
        q1, q2 = _ptr(p1, F32, "gn partials"), _ptr(p2, F32, "gn partials 2")
        ld1, ld2 = p1.shape[-1], (p2.shape[-1] if p2 is not None else 0)
        fbytes = 4.0 * (p1.numel() + (p2.numel() if p2 is not None else 0))
        _launch("gn_finalize", dict(bytes=fbytes),
                lambda: _check(lib.sdv_groupnorm_finalize(q1, C1, ld1, bpi1, nrep1, rs1, q2, C2, ld2, bpi2, nrep2, rs2, nimg, groups, splits,
                                                          pp, _stream()), "sdv_groupnorm_finalize"))
    else:
        splits = gn_splits(HW)
        partials = torch.empty((nimg, splits, groups, 2), dtype=F32, device=x.device)
        pp = _ptr(partials)
    xp, x2p, op = _ptr(x, BF16, "X"), _ptr(x2, BF16, "X2"), _ptr(out, FP8 if fp8 else BF16, "Y")
    gp, bp = _ptr(gamma, F32, "gamma"), _ptr(beta, F32, "beta")
    if p1 is None:
        _launch("gn_stats", dict(bytes=nbytes),
                lambda: _check(lib.sdv_groupnorm_stats(xp, x2p, C1, C2, nimg, HW, groups, splits, pp, _stream()),
                               "sdv_groupnorm_stats"))
    if fp8:
        _launch("gn_apply", dict(bytes=1.5 * nbytes),
                lambda: _check(lib.sdv_groupnorm_apply_fp8(xp, x2p, C1, C2, nimg, HW, groups, splits, pp, gp, bp, eps, int(silu),
                                                           op, 1.0 / fp8_scale, _stream()), "sdv_groupnorm_apply_fp8"))
        return
    _launch("gn_apply", dict(bytes=2 * nbytes),
            lambda: _check(lib.sdv_groupnorm_apply(xp, x2p, C1, C2, nimg, HW, groups, splits, pp, gp, bp, eps, int(silu),
                                                   op, _stream()), "sdv_groupnorm_apply"))


_k_groupnorm = _defop("k_groupnorm(Tensor x, Tensor gamma, Tensor beta, Tensor? x2, Tensor(a!) out, Tensor? gn1, Tensor? gn2, int[] ints, "
                      "float eps, float fp8_scale) -> ()", _groupnorm_impl)


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, nimg: int, HW: int, groups: int,
              eps: float, silu: bool, x2: Optional[torch.Tensor] = None, out=None, fp8_scale: Optional[float] = None) -> torch.Tensor:
    """GroupNorm(+SiLU) over NHWC [nimg*HW, C1] (++ [.., C2] concatenated on channels) -> bf16 [.., C1+C2]
    (``torch.ops.sdv.k_groupnorm``: statistics pass + apply pass).  When ``x`` (and ``x2``) carry the statistics their producer's
    epilogue emitted (``tensor._sdv_gn``, see ``gemm(gn_hw=)``) and those describe exactly this tensor, the statistics pass is
    replaced by ``sdv_groupnorm_finalize`` over the per-block partials.
    ``fp8_scale`` s: the result is written as OCP e4m3 bytes q = sat(y / s) instead (y ~ q * s), the fp8 conv's operand."""
    C1 = x.shape[1]
    C2 = x2.shape[1] if x2 is not None else 0
    if out is None:
        out = torch.empty((nimg * HW, C1 + C2), dtype=BF16 if fp8_scale is None else FP8, device=x.device)
    g1 = getattr(x, "_sdv_gn", None) if GN_EPILOGUE else None
    g2 = getattr(x2, "_sdv_gn", None) if (x2 is not None and GN_EPILOGUE) else None

    def fits(g, t):
        return (g is not None and g.nimg == nimg and g.HW == HW and g.C == t.shape[1] and t.shape[0] == nimg * HW
                and g.ver == _ver(t))

    geo = [0, 1, 0, 0, 1, 0]
    p1 = p2 = None
    if fits(g1, x) and (x2 is None or fits(g2, x2)):
        p1, geo[0:3] = g1.p, [g1.bpi, g1.nrep, g1.rep_stride]
        if x2 is not None:
            p2, geo[3:6] = g2.p, [g2.bpi, g2.nrep, g2.rep_stride]
    _k_groupnorm(x, gamma, beta, x2, out, p1, p2, [nimg, HW, groups, int(silu)] + geo, float(eps),
                 float(fp8_scale) if fp8_scale is not None else 0.0)
    return out


def _layernorm_impl(x, gamma, beta, eps, out):
    lib = load()
    rows, Cn = x.shape
    if not x.is_contiguous():
        raise SdvHipError("layernorm: input must be contiguous")
    xp, gp, bp, op = _ptr(x, BF16, "X"), _ptr(gamma, F32), _ptr(beta, F32), _ptr(out, BF16)
    _launch("layernorm", dict(bytes=4.0 * rows * Cn),
            lambda: _check(lib.sdv_layernorm_bf16(xp, gp, bp, eps, rows, Cn, op, _stream()), "sdv_layernorm_bf16"))


_k_layernorm = _defop("k_layernorm(Tensor x, Tensor gamma, Tensor beta, float eps, Tensor(a!) out) -> ()", _layernorm_impl)


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, out=None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(x)
    _k_layernorm(x, gamma, beta, float(eps), out)
    return out


# ------------------------------------------------------------------------------------------------
# small convs / latents
# ------------------------------------------------------------------------------------------------
def _conv3x3_cin_small_impl(x, w, bias, out, nimg, H, W, circular):
    lib = load()
    Cin, Cout = x.shape[1], w.shape[0]
    xp, wp, bp, op = _ptr(x, BF16, "X"), _ptr(w, BF16, "W"), _ptr(bias, F32), _ptr(out, BF16)
    _launch("conv_cin_small", dict(flops=18.0 * nimg * H * W * Cin * Cout, bytes=2.0 * nimg * H * W * (Cin + Cout)),
            lambda: _check(lib.sdv_conv3x3_cin_small(xp, wp, bp, op, nimg, H, W, Cin, Cout, int(circular), _stream()),
                           "sdv_conv3x3_cin_small"))


_k_conv3x3_cin_small = _defop("k_conv3x3_cin_small(Tensor x, Tensor w, Tensor? bias, Tensor(a!) out, int nimg, int H, int W, "
                              "bool circular) -> ()", _conv3x3_cin_small_impl)


def conv3x3_cin_small(x, w, bias, *, nimg, H, W, circular=False, out=None):
    if out is None:
        out = torch.empty((nimg * H * W, w.shape[0]), dtype=BF16, device=x.device)
    _k_conv3x3_cin_small(x, w, bias, out, nimg, H, W, bool(circular))
    return out


def _im2col3x3_c4_impl(x, cols, nimg, H, W, circular):
    lib = load()
    xp, cp = _ptr(x, BF16, "X"), _ptr(cols, BF16)
    _launch("im2col_c4", dict(bytes=2.0 * nimg * H * W * (4 + 64)),
            lambda: _check(lib.sdv_im2col3x3_c4(xp, cp, nimg, H, W, int(circular), _stream()), "sdv_im2col3x3_c4"))


_k_im2col3x3_c4 = _defop("k_im2col3x3_c4(Tensor x, Tensor(a!) cols, int nimg, int H, int W, bool circular) -> ()", _im2col3x3_c4_impl)


def conv3x3_c4(x, w_pad, bias, *, nimg, H, W, circular=False, out=None, gn: bool = False):
    """3x3 pad-1 conv of a 4-channel NHWC tensor on the matrix cores: im2col to 64-wide rows + K = 64 GEMM.
    ``w_pad``: [Cout, 64] = OHWI weights [Cout, 36] zero-padded (see ``weights.conv_w_c4``)."""
    if x.shape[1] != 4:
        raise SdvHipError(f"conv3x3_c4: expected 4 input channels, got {x.shape[1]}")
    cols = torch.empty((nimg * H * W, 64), dtype=BF16, device=x.device)
    _k_im2col3x3_c4(x, cols, nimg, H, W, bool(circular))
    return linear(cols, w_pad, bias, out=out, gn_hw=H * W if gn else 0)


def embed_tokens(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """CLIP input embeddings: ids int64 [B, L] -> bf16 [B*L, D] = tok[ids] + pos[position]."""
    if ids.dtype != torch.int64 or ids.ndim != 2:
        raise SdvHipError("embed_tokens: ids must be int64 [B, L]")
    B, L = ids.shape
    V, D = tok.shape
    if L > pos.shape[0] or pos.shape[1] != D:
        raise SdvHipError(f"embed_tokens: {L} positions / width {D} do not fit the position table {tuple(pos.shape)}")
    return _k_embed_tokens(ids.contiguous(), tok, pos)


def _embed_tokens_impl(ids, tok, pos):
    lib = load()
    B, L = ids.shape
    V, D = tok.shape
    out = torch.empty((B * L, D), dtype=BF16, device=ids.device)
    _check(lib.sdv_embed_tokens(_ptr(ids, torch.int64, "ids"), _ptr(tok, F32, "tok"), _ptr(pos, F32, "pos"), _ptr(out, BF16),
                                B * L, L, D, V, _stream()), "sdv_embed_tokens")
    return out


_k_embed_tokens = _defop("k_embed_tokens(Tensor ids, Tensor tok, Tensor pos) -> Tensor", _embed_tokens_impl,
                         lambda ids, tok, pos: tok.new_empty((ids.shape[0] * ids.shape[1], tok.shape[1]), dtype=BF16))


def rgb_u8_to_bf16_c4(img_u8: torch.Tensor, scale: float = 1.0 / 255.0) -> torch.Tensor:
    """uint8 RGB NHWC [..., 3] -> bf16 rows [npix, 4] = {r, g, b, 0} * scale."""
    if img_u8.shape[-1] != 3 or not img_u8.is_contiguous():
        raise SdvHipError("rgb_u8_to_bf16_c4: expected a contiguous [..., 3] uint8 tensor")
    return _k_rgb_u8_to_bf16_c4(img_u8, float(scale))


def _rgb_u8_to_bf16_c4_impl(img_u8, scale):
    lib = load()
    npix = img_u8.numel() // 3
    out = torch.empty((npix, 4), dtype=BF16, device=img_u8.device)
    _check(lib.sdv_rgb_u8_to_bf16_c4(_ptr(img_u8, torch.uint8, "img"), _ptr(out, BF16), npix, scale, _stream()),
           "sdv_rgb_u8_to_bf16_c4")
    return out


_k_rgb_u8_to_bf16_c4 = _defop("k_rgb_u8_to_bf16_c4(Tensor img_u8, float scale) -> Tensor", _rgb_u8_to_bf16_c4_impl,
                              lambda img, scale: img.new_empty((img.numel() // 3, 4), dtype=BF16))


def axpby(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, alpha: float, beta: float):
    """out = alpha*a + beta*b over [rows, cols] bf16 (column slices of wider buffers allowed)."""
    if b.shape != a.shape or out.shape != a.shape:
        raise SdvHipError("axpby: shape mismatch")
    for t in (a, b, out):
        if t.stride(1) != 1:
            raise SdvHipError("axpby: rows must be contiguous")
    _k_axpby(a, b, out, float(alpha), float(beta))


def _axpby_impl(a, b, out, alpha, beta):
    lib = load()
    rows, cols = a.shape
    _launch("axpby", dict(bytes=6.0 * rows * cols),
            lambda: _check(lib.sdv_axpby_bf16(_ptr(a, BF16, "a"), a.stride(0), _ptr(b, BF16, "b"), b.stride(0),
                                              _ptr(out, BF16, "out"), out.stride(0), rows, cols, alpha, beta, _stream()),
                           "sdv_axpby_bf16"))


_k_axpby = _defop("k_axpby(Tensor a, Tensor b, Tensor(a!) out, float alpha, float beta) -> ()", _axpby_impl)




def _latent_affine_impl(x, wpq, bias, in_scale, out, npix, Cn):
    lib = load()
    _check(lib.sdv_latent_affine(_ptr(x, F32), _ptr(wpq, F32), _ptr(bias, F32), in_scale, _ptr(out, BF16), npix, Cn,
                                 _stream()), "sdv_latent_affine")


_k_latent_affine = _defop("k_latent_affine(Tensor x, Tensor wpq, Tensor bias, float in_scale, Tensor(a!) out, int npix, int Cn) -> ()",
                          _latent_affine_impl)


def latent_affine(x, wpq, bias, in_scale, out, npix, Cn):
    _k_latent_affine(x, wpq, bias, float(in_scale), out, npix, Cn)


# ------------------------------------------------------------------------------------------------
# interpolation / scheduler step
# ------------------------------------------------------------------------------------------------
def _slerp_stats_impl(v0, v1):
    lib = load()
    stats = torch.empty(3, dtype=torch.float64, device=v0.device)
    _check(lib.sdv_slerp_stats(_ptr(v0, F32, "v0"), _ptr(v1, F32, "v1"), v0.numel(), _ptr(stats), _stream()),
           "sdv_slerp_stats")
    return stats


_k_slerp_stats = _defop("k_slerp_stats(Tensor v0, Tensor v1) -> Tensor", _slerp_stats_impl,
                        lambda v0, v1: v0.new_empty((3,), dtype=torch.float64))


def slerp_stats(v0, v1) -> torch.Tensor:
    return _k_slerp_stats(v0, v1)


def _slerp_batch_impl(v0, v1, stats, T, out, C_, HW, to_hwc, dot_threshold):
    lib = load()
    _check(lib.sdv_slerp_batch(_ptr(v0, F32), _ptr(v1, F32), _ptr(stats, torch.float64), _ptr(T, F32), T.numel(), C_, HW,
                               int(to_hwc), dot_threshold, _ptr(out, F32), _stream()), "sdv_slerp_batch")


_k_slerp_batch = _defop("k_slerp_batch(Tensor v0, Tensor v1, Tensor stats, Tensor T, Tensor(a!) out, int C_, int HW, bool to_hwc, "
                        "float dot_threshold) -> ()", _slerp_batch_impl)


def slerp_batch(v0, v1, stats, T, *, C_: int, HW: int, to_hwc: bool, dot_threshold: float = 0.9995, out=None):
    if out is None:
        out = torch.empty((T.numel(), C_ * HW), dtype=F32, device=v0.device)
    _k_slerp_batch(v0, v1, stats, T, out, C_, HW, bool(to_hwc), float(dot_threshold))
    return out


def _lerp_batch_impl(a, b, T, out_f32, out_bf16):
    lib = load()
    _check(lib.sdv_lerp_batch(_ptr(a, F32), _ptr(b, F32), _ptr(T, F32), T.numel(), a.numel(), _ptr(out_f32, F32),
                              _ptr(out_bf16, BF16), _stream()), "sdv_lerp_batch")


_k_lerp_batch = _defop("k_lerp_batch(Tensor a, Tensor b, Tensor T, Tensor(a!)? out_f32, Tensor(b!)? out_bf16) -> ()", _lerp_batch_impl)


def lerp_batch(a, b, T, *, out_f32=None, out_bf16=None):
    _k_lerp_batch(a, b, T, out_f32, out_bf16)


def _cfg_ddim_step_impl(eps, latents, x2, coefs, step_ptr, noise, guidance, cfg, n):
    lib = load()
    _check(lib.sdv_cfg_ddim_step(_ptr(eps, F32), _ptr(latents, F32), _ptr(x2, BF16), _ptr(coefs, F32),
                                 _ptr(step_ptr, torch.int32), _ptr(noise, F32), guidance, int(cfg), n, _stream()),
           "sdv_cfg_ddim_step")


_k_cfg_ddim_step = _defop("k_cfg_ddim_step(Tensor eps, Tensor(a!) latents, Tensor(b!) x2, Tensor coefs, Tensor? step_ptr, Tensor? noise, "
                          "float guidance, bool cfg, int n) -> ()", _cfg_ddim_step_impl)


def cfg_ddim_step(eps, latents, x2, coefs, step_ptr, noise, guidance: float, cfg: bool, n: int):
    _k_cfg_ddim_step(eps, latents, x2, coefs, step_ptr, noise, float(guidance), bool(cfg), n)


def _cfg_multistep_step_impl(eps, latents, x2, hist, xsave, table, step_ptr, noise, guidance, cfg, n):
    lib = load()
    _check(lib.sdv_cfg_multistep_step(_ptr(eps, F32), _ptr(latents, F32), _ptr(x2, BF16), _ptr(hist, F32), _ptr(xsave, F32),
                                      _ptr(table, F32), _ptr(step_ptr, torch.int32), _ptr(noise, F32), guidance, int(cfg), n,
                                      _stream()), "sdv_cfg_multistep_step")


_k_cfg_multistep_step = _defop("k_cfg_multistep_step(Tensor eps, Tensor(a!) latents, Tensor(b!) x2, Tensor(c!) hist, Tensor(d!) xsave, "
                               "Tensor table, Tensor? step_ptr, Tensor? noise, float guidance, bool cfg, int n) -> ()",
                               _cfg_multistep_step_impl)


def cfg_multistep_step(eps, latents, x2, hist, xsave, table, step_ptr, noise, guidance: float, cfg: bool, n: int):
    """One fused guidance + linear-multistep scheduler update (sdv_hip.h: every scheduler besides DDIM)."""
    _k_cfg_multistep_step(eps, latents, x2, hist, xsave, table, step_ptr, noise, float(guidance), bool(cfg), n)


def _latents_to_unet_input_impl(latents, x2, cfg, n):
    lib = load()
    _check(lib.sdv_latents_to_unet_input(_ptr(latents, F32), _ptr(x2, BF16), int(cfg), n, _stream()),
           "sdv_latents_to_unet_input")


_k_latents_to_unet_input = _defop("k_latents_to_unet_input(Tensor latents, Tensor(a!) x2, bool cfg, int n) -> ()",
                                  _latents_to_unet_input_impl)


def latents_to_unet_input(latents, x2, cfg: bool, n: int):
    _k_latents_to_unet_input(latents, x2, bool(cfg), n)


def _step_counter_add_impl(step_ptr, inc):
    lib = load()
    _check(lib.sdv_step_counter_add(_ptr(step_ptr, torch.int32), inc, _stream()), "sdv_step_counter_add")


_k_step_counter_add = _defop("k_step_counter_add(Tensor(a!) step_ptr, int inc) -> ()", _step_counter_add_impl)


def step_counter_add(step_ptr, inc: int = 1):
    _k_step_counter_add(step_ptr, inc)


def _timestep_embedding_impl(ts, dim, flip, freq_shift):
    lib = load()
    out = torch.empty((ts.numel(), dim), dtype=F32, device=ts.device)
    _check(lib.sdv_timestep_embedding(_ptr(ts, F32), ts.numel(), dim, int(flip), freq_shift, _ptr(out), _stream()),
           "sdv_timestep_embedding")
    return out


_k_timestep_embedding = _defop("k_timestep_embedding(Tensor ts, int dim, bool flip, float freq_shift) -> Tensor", _timestep_embedding_impl,
                               lambda ts, dim, flip, fs: ts.new_empty((ts.numel(), dim), dtype=F32))


def timestep_embedding(ts, dim: int, flip: bool, freq_shift: float):
    return _k_timestep_embedding(ts, dim, bool(flip), float(freq_shift))


def _linear_small_impl(x, w, b, add, silu_in):
    lib = load()
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=F32, device=x.device)
    _check(lib.sdv_linear_small(_ptr(x, F32), _ptr(w, BF16), _ptr(b, F32), _ptr(add, F32), _ptr(out), M, N, K,
                                int(silu_in), _stream()), "sdv_linear_small")
    return out


_k_linear_small = _defop("k_linear_small(Tensor x, Tensor w, Tensor? b, Tensor? add, bool silu_in) -> Tensor", _linear_small_impl,
                         lambda x, w, b, add, silu_in: x.new_empty((x.shape[0], w.shape[0]), dtype=F32))


def linear_small(x, w, b=None, add=None, silu_in=False):
    return _k_linear_small(x, w, b, add, bool(silu_in))


def _permute_f32_impl(x, to_nhwc):
    lib = load()
    if to_nhwc:
        n, c, h, w = x.shape
        out = torch.empty((n, h, w, c), dtype=F32, device=x.device)
        _check(lib.sdv_nchw_to_nhwc_f32(_ptr(x.contiguous(), F32), _ptr(out), n, c, h * w, _stream()), "sdv_nchw_to_nhwc_f32")
    else:
        n, h, w, c = x.shape
        out = torch.empty((n, c, h, w), dtype=F32, device=x.device)
        _check(lib.sdv_nhwc_to_nchw_f32(_ptr(x.contiguous(), F32), _ptr(out), n, c, h * w, _stream()), "sdv_nhwc_to_nchw_f32")
    return out


_k_permute_f32 = _defop("k_permute_f32(Tensor x, bool to_nhwc) -> Tensor", _permute_f32_impl,
                        lambda x, to_nhwc: x.new_empty((x.shape[0], x.shape[2], x.shape[3], x.shape[1]) if to_nhwc else
                                                       (x.shape[0], x.shape[3], x.shape[1], x.shape[2]), dtype=F32))


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return _k_permute_f32(x, True)


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return _k_permute_f32(x, False)


def _f32_to_bf16_impl(x):
    lib = load()
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _check(lib.sdv_f32_to_bf16(_ptr(x.contiguous(), F32), _ptr(out), x.numel(), _stream()), "sdv_f32_to_bf16")
    return out


_k_f32_to_bf16 = _defop("k_f32_to_bf16(Tensor x) -> Tensor", _f32_to_bf16_impl, lambda x: x.new_empty(x.shape, dtype=BF16))


def f32_to_bf16(x: torch.Tensor) -> torch.Tensor:
    return _k_f32_to_bf16(x)


# ------------------------------------------------------------------------------------------------
# safety checker glue (csrc/sdv_vision.hip): frames -> patch rows, cosine head + black-out
# ------------------------------------------------------------------------------------------------
def patch_kpad(P: int) -> int:
    """K = 3 * P * P of the patch-embedding GEMM rounded up to sdv_gemm_bf16's K granularity (588 -> 640 for P = 14)."""
    return (3 * P * P + 63) // 64 * 64


def _clip_preprocess_impl(frames, patches, x_off, x_cnt, x_w, y_off, y_cnt, y_w, S, P, mean, std):
    # every check comes before the first pointer is taken
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise SdvHipError(f"clip_preprocess: frames must be a contiguous uint8 [n, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)} "
                          f"strides {frames.stride()}")
    n, H, W, _ = frames.shape
    if n < 1 or S < 1 or P < 1 or S % P:
        raise SdvHipError(f"clip_preprocess: bad geometry n={n} S={S} P={P} (S % P == 0)")
    G, Kpad = S // P, patch_kpad(P)
    if patches.dtype != BF16 or patches.dim() != 2 or patches.shape[1] != Kpad or patches.stride(1) != 1 or patches.stride(0) != Kpad:
        raise SdvHipError(f"clip_preprocess: patches must be dense bf16 rows of Kpad = {Kpad} columns, got {patches.dtype} {tuple(patches.shape)} "
                          f"strides {patches.stride()}")
    if patches.shape[0] != n * G * G:
        raise SdvHipError(f"clip_preprocess: patches has {patches.shape[0]} rows, {n} frames x {G} x {G} patches need {n * G * G}")
    if patches.data_ptr() % 16:
        raise SdvHipError("clip_preprocess: patches must be 16-byte aligned")
    for name, off, cnt, w, size in (("x", x_off, x_cnt, x_w, W), ("y", y_off, y_cnt, y_w, H)):
        if off.dtype != torch.int32 or cnt.dtype != torch.int32 or w.dtype != F32 or not (off.is_contiguous() and cnt.is_contiguous() and w.is_contiguous()):
            raise SdvHipError(f"clip_preprocess: {name} tap tables must be contiguous int32 / int32 / fp32")
        if off.numel() != S or cnt.numel() != S or w.dim() != 2 or w.shape[0] != S or not 1 <= w.shape[1] <= size:
            raise SdvHipError(f"clip_preprocess: {name} tap tables must hold S = {S} entries ([S], [S], [S, taps <= {size}]), got {off.numel()} / "
                              f"{cnt.numel()} / {tuple(w.shape)}")
    if len(mean) != 3 or len(std) != 3:
        raise SdvHipError("clip_preprocess: image_mean / image_std hold one value per RGB channel")
    lib = load()
    args = (_ptr(frames, torch.uint8, "frames"), _ptr(patches, BF16, "patches"), n, H, W, S, P, Kpad,
            _ptr(x_off, torch.int32, "x_off"), _ptr(x_cnt, torch.int32, "x_cnt"), _ptr(x_w, F32, "x_w"), x_w.shape[1],
            _ptr(y_off, torch.int32, "y_off"), _ptr(y_cnt, torch.int32, "y_cnt"), _ptr(y_w, F32, "y_w"), y_w.shape[1],
            (C.c_float * 3)(*mean), (C.c_float * 3)(*std))
    _launch("clip_preprocess", dict(bytes=3.0 * n * H * W + 2.0 * patches.numel()),
            lambda: _check(lib.sdv_clip_preprocess_patches(*args, _stream()), "sdv_clip_preprocess_patches"))


_k_clip_preprocess = _defop("k_clip_preprocess(Tensor frames, Tensor(a!) patches, Tensor x_off, Tensor x_cnt, Tensor x_w, Tensor y_off, Tensor y_cnt, "
                            "Tensor y_w, int S, int P, float[] mean, float[] std) -> ()", _clip_preprocess_impl)


def clip_preprocess_patches(frames: torch.Tensor, taps_x, taps_y, *, S: int, P: int, mean, std, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB NHWC frames [n, H, W, 3] -> bf16 patch rows [n * (S/P)^2, Kpad] of the CLIP patch-embedding GEMM
    (``torch.ops.sdv.k_clip_preprocess`` -> sdv_clip_preprocess_patches): PIL-bicubic resize of the shortest edge to ``S``, centre
    crop, / 255, (x - mean) / std, im2col in (c, py, px) order.  ``taps_x`` / ``taps_y``: (off int32 [S], cnt int32 [S], w fp32
    [S, taps]) on the device, from ``vision.resample_taps``."""
    if out is None:
        out = torch.empty((frames.shape[0] * (S // P) ** 2, patch_kpad(P)), dtype=BF16, device=frames.device)
    _k_clip_preprocess(frames, out, *taps_x, *taps_y, int(S), int(P), [float(v) for v in mean], [float(v) for v in std])
    return out


def _safety_screen_impl(image_embeds, concept, special, thr_c, thr_s, frames, flags, scores):
    if image_embeds.dtype != F32 or image_embeds.dim() != 2 or not image_embeds.is_contiguous():
        raise SdvHipError(f"safety_screen: image_embeds must be contiguous fp32 [n, D], got {image_embeds.dtype} {tuple(image_embeds.shape)}")
    n, D = image_embeds.shape
    for name, t in (("concept_embeds", concept), ("special_care_embeds", special)):
        if t.dtype != F32 or t.dim() != 2 or t.shape[1] != D or not t.is_contiguous():
            raise SdvHipError(f"safety_screen: {name} must be contiguous fp32 [rows, D = {D}], got {t.dtype} {tuple(t.shape)}")
    nc, ns = concept.shape[0], special.shape[0]
    if nc < 1 or nc + ns > 64:
        raise SdvHipError(f"safety_screen: at most 64 concept + special-care rows, got {nc} + {ns}")
    if thr_c.dtype != F32 or thr_s.dtype != F32 or thr_c.numel() != nc or thr_s.numel() != ns or not (thr_c.is_contiguous() and thr_s.is_contiguous()):
        raise SdvHipError(f"safety_screen: thresholds must be contiguous fp32 vectors of {nc} / {ns} elements, got {thr_c.numel()} / {thr_s.numel()}")
    if flags.dtype != torch.int32 or flags.numel() != n or not flags.is_contiguous():
        raise SdvHipError(f"safety_screen: flags must be a contiguous int32 vector of n = {n} elements, got {flags.dtype} x {flags.numel()}")
    if scores.dtype != F32 or tuple(scores.shape) != (n, ns + nc) or not scores.is_contiguous():
        raise SdvHipError(f"safety_screen: scores must be contiguous fp32 [{n}, {ns + nc}], got {scores.dtype} {tuple(scores.shape)}")
    frame_bytes = 0
    if frames is not None:
        if frames.dtype != torch.uint8 or frames.dim() < 2 or frames.shape[0] != n or not frames.is_contiguous() or frames.numel() == 0:
            raise SdvHipError(f"safety_screen: frames must be a contiguous uint8 tensor of n = {n} frames, got {frames.dtype} {tuple(frames.shape)} "
                              f"strides {frames.stride()}")
        if frames.data_ptr() % 16:
            raise SdvHipError("safety_screen: frames must be 16-byte aligned")
        frame_bytes = frames.numel() // n
    lib = load()
    args = (_ptr(image_embeds, F32, "image_embeds"), _ptr(concept, F32, "concept_embeds"), _ptr(special, F32, "special_care_embeds"),
            _ptr(thr_c, F32, "concept_thr"), _ptr(thr_s, F32, "special_thr"), n, D, nc, ns, _ptr(frames, torch.uint8, "frames"), frame_bytes,
            _ptr(flags, torch.int32, "flags"), _ptr(scores, F32, "scores"))
    _launch("safety_screen", dict(bytes=4.0 * D * (n + nc + ns)),
            lambda: _check(lib.sdv_safety_screen(*args, _stream()), "sdv_safety_screen"))


_k_safety_screen = _defop("k_safety_screen(Tensor image_embeds, Tensor concept, Tensor special, Tensor thr_c, Tensor thr_s, Tensor(a!)? frames, "
                          "Tensor(b!) flags, Tensor(c!) scores) -> ()", _safety_screen_impl)


def safety_screen(image_embeds: torch.Tensor, concept: torch.Tensor, special: torch.Tensor, thr_c: torch.Tensor, thr_s: torch.Tensor,
                  frames: Optional[torch.Tensor] = None):
    """The head of diffusers' ``StableDiffusionSafetyChecker`` and the black-out of the flagged frames
    (``torch.ops.sdv.k_safety_screen`` -> sdv_safety_screen): returns (flags int32 [n], scores fp32 [n, special + concept]), both on
    the device; flagged ``frames`` (uint8, n leading) are zeroed in place."""
    n = image_embeds.shape[0]
    flags = torch.empty((n,), dtype=torch.int32, device=image_embeds.device)
    scores = torch.empty((n, special.shape[0] + concept.shape[0]), dtype=F32, device=image_embeds.device)
    _k_safety_screen(image_embeds, concept, special, thr_c, thr_s, frames, flags, scores)
    return flags, scores


# ------------------------------------------------------------------------------------------------
# JPEG encoder (csrc/sdv_jpeg.hip; jpeg.py builds the tables, the header and the workspaces)
# ------------------------------------------------------------------------------------------------
def jpeg_mcu_grid(H: int, W: int):
    return (H + 15) // 16, (W + 15) // 16


def jpeg_scratch_bytes(n: int, H: int) -> int:
    """sdv_jpeg_entropy_pack's scratch: an int64 position and an int32 length per restart interval (one per MCU row and frame)."""
    return 12 * n * ((H + 15) // 16)


def _jpeg_transform_impl(frames, qtab_luma, qtab_chroma, coef):
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise SdvHipError(f"jpeg_transform: frames must be a contiguous uint8 [n, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)} "
                          f"contiguous={frames.is_contiguous()}")
    n, H, W, _ = frames.shape
    rows, cols = jpeg_mcu_grid(H, W)
    if coef.dtype != torch.int16 or tuple(coef.shape) != (n, rows, cols, 6, 64) or not coef.is_contiguous():
        raise SdvHipError(f"jpeg_transform: coef must be a contiguous int16 [{n}, {rows}, {cols}, 6, 64] tensor, got {coef.dtype} {tuple(coef.shape)}")
    if len(qtab_luma) != 64 or len(qtab_chroma) != 64:
        raise SdvHipError(f"jpeg_transform: quantisation tables hold 64 entries, got {len(qtab_luma)} / {len(qtab_chroma)}")
    if any(not 0 <= int(v) <= 65535 for v in list(qtab_luma) + list(qtab_chroma)):
        raise SdvHipError("jpeg_transform: quantisation table entry outside 1 .. 255")
    lib = load()
    ql, qc = (C.c_uint16 * 64)(*[int(v) for v in qtab_luma]), (C.c_uint16 * 64)(*[int(v) for v in qtab_chroma])
    args = (_ptr(frames, name="frames"), n, H, W, ql, qc, _ptr(coef, name="coef"))
    _launch("jpeg_transform", dict(bytes=3.0 * n * H * W + 2.0 * coef.numel()),
            lambda: _check(lib.sdv_jpeg_transform_u8(*args, _stream()), "sdv_jpeg_transform_u8"))


_k_jpeg_transform = _defop("k_jpeg_transform(Tensor frames, int[] qtab_luma, int[] qtab_chroma, Tensor(a!) coef) -> ()", _jpeg_transform_impl)


def jpeg_transform(frames: torch.Tensor, qtab_luma, qtab_chroma, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB frames [n, H, W, 3] in HBM -> quantised DCT coefficients int16 [n, ceil(H/16), ceil(W/16), 6, 64], zigzag order, MCU
    block order Y00 Y01 Y10 Y11 Cb Cr (``torch.ops.sdv.k_jpeg_transform`` -> sdv_jpeg_transform_u8).  Tables: 64 entries, natural order."""
    if out is None:
        rows, cols = jpeg_mcu_grid(frames.shape[1], frames.shape[2])
        out = torch.empty((frames.shape[0], rows, cols, 6, 64), dtype=torch.int16, device=frames.device)
    _k_jpeg_transform(frames, [int(v) for v in qtab_luma], [int(v) for v in qtab_chroma], out)
    return out


def _jpeg_entropy_pack_impl(coef, H, W, header, scratch, out, offsets, needed):
    rows, cols = jpeg_mcu_grid(H, W)
    if coef.dtype != torch.int16 or coef.ndim != 5 or tuple(coef.shape[1:]) != (rows, cols, 6, 64) or not coef.is_contiguous():
        raise SdvHipError(f"jpeg_entropy_pack: coef must be a contiguous int16 [n, {rows}, {cols}, 6, 64] tensor for {H} x {W} frames, got "
                          f"{coef.dtype} {tuple(coef.shape)}")
    n = coef.shape[0]
    for name, t in (("header", header), ("scratch", scratch), ("out", out)):
        if t.dtype != torch.uint8 or t.ndim != 1 or not t.is_contiguous():
            raise SdvHipError(f"jpeg_entropy_pack: {name} must be a contiguous 1-D uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    if scratch.numel() < jpeg_scratch_bytes(n, H):
        raise SdvHipError(f"jpeg_entropy_pack: scratch holds {scratch.numel()} bytes, {n} frames of {rows} MCU rows need {jpeg_scratch_bytes(n, H)}")
    if offsets.dtype != torch.int64 or offsets.numel() != n + 1 or not offsets.is_contiguous():
        raise SdvHipError(f"jpeg_entropy_pack: offsets must be a contiguous int64 vector of n + 1 = {n + 1} elements, got {offsets.dtype} x {offsets.numel()}")
    if needed.dtype != torch.int64 or needed.numel() != 1:
        raise SdvHipError(f"jpeg_entropy_pack: needed must be one int64 element, got {needed.dtype} x {needed.numel()}")
    lib = load()
    args = (_ptr(coef, name="coef"), n, H, W, _ptr(header, name="header"), header.numel(), _ptr(scratch, name="scratch"), scratch.numel(),
            _ptr(out, name="out"), out.numel(), _ptr(offsets, name="offsets"), _ptr(needed, name="needed"))
    _launch("jpeg_entropy_pack", dict(bytes=2.0 * 2 * coef.numel()),
            lambda: _check(lib.sdv_jpeg_entropy_pack(*args, _stream()), "sdv_jpeg_entropy_pack"))


_k_jpeg_entropy_pack = _defop("k_jpeg_entropy_pack(Tensor coef, int H, int W, Tensor header, Tensor(a!) scratch, Tensor(b!) out, Tensor(c!) offsets, "
                              "Tensor(d!) needed) -> ()", _jpeg_entropy_pack_impl)


def jpeg_entropy_pack(coef: torch.Tensor, H: int, W: int, header: torch.Tensor, scratch: torch.Tensor, out: torch.Tensor,
                      offsets: torch.Tensor, needed: torch.Tensor):
    """Huffman-code the coefficient blocks and pack complete files into ``out`` (``torch.ops.sdv.k_jpeg_entropy_pack`` ->
    sdv_jpeg_entropy_pack): ``out[offsets[k]:offsets[k + 1]]`` is file k.  When ``needed`` (= offsets[n]) exceeds ``out.numel()``
    nothing was written to ``out``: call again with a buffer of that size."""
    _k_jpeg_entropy_pack(coef, int(H), int(W), header, scratch, out, offsets, needed)


# ------------------------------------------------------------------------------------------------
# PNG encoder (csrc/sdv_png.hip; png.py builds the header and the workspaces and fills the IDAT CRC)
# ------------------------------------------------------------------------------------------------
PNG_MAX_DIM = 16384


def png_stripes(H: int, W: int, stripe_rows: Optional[int] = None) -> int:
    """Deflate blocks per frame: the filtered rows are cut into stripes of ``stripe_rows`` rows (default: as many rows as fit 32 KiB)."""
    if stripe_rows is None:
        stripe_rows = max(1, min(H, 32768 // (1 + 3 * W)))
    if not 1 <= stripe_rows <= H:
        raise SdvHipError(f"png: stripe_rows must be 1 .. H = {H}, got {stripe_rows}")
    return (H + stripe_rows - 1) // stripe_rows


def png_scratch_bytes(n: int, H: int, stripe_rows: int) -> int:
    """sdv_png_deflate_pack's scratch: an int64 position and an int64 length per stripe, an Adler-32 per frame, 260 code words per stripe."""
    S = n * png_stripes(H, 1, stripe_rows)
    return 16 * S + 8 * ((n + 1) // 2) + 1040 * S


def _png_frame_shape(what, frames):
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise SdvHipError(f"{what}: frames must be a contiguous uint8 [n, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)} "
                          f"contiguous={frames.is_contiguous()}")
    n, H, W, _ = frames.shape
    if n < 1 or not (1 <= H <= PNG_MAX_DIM and 1 <= W <= PNG_MAX_DIM):
        raise SdvHipError(f"{what}: frame size must be 1 .. {PNG_MAX_DIM} and n >= 1, got n={n} H={H} W={W}")
    return n, H, W


def _png_filter_impl(frames, filtered, adler_rows):
    n, H, W = _png_frame_shape("png_filter", frames)
    if filtered.dtype != torch.uint8 or tuple(filtered.shape) != (n, H, 1 + 3 * W) or not filtered.is_contiguous():
        raise SdvHipError(f"png_filter: filtered must be a contiguous uint8 [{n}, {H}, {1 + 3 * W}] tensor, got {filtered.dtype} {tuple(filtered.shape)}")
    if adler_rows.dtype != torch.int32 or tuple(adler_rows.shape) != (n, H, 2) or not adler_rows.is_contiguous():
        raise SdvHipError(f"png_filter: adler_rows must be a contiguous int32 [{n}, {H}, 2] tensor, got {adler_rows.dtype} {tuple(adler_rows.shape)}")
    lib = load()
    args = (_ptr(frames, name="frames"), n, H, W, _ptr(filtered, name="filtered"), _ptr(adler_rows, name="adler_rows"))
    _launch("png_filter", dict(bytes=2.0 * 3 * n * H * W), lambda: _check(lib.sdv_png_filter_u8(*args, _stream()), "sdv_png_filter_u8"))


_k_png_filter = _defop("k_png_filter(Tensor frames, Tensor(a!) filtered, Tensor(b!) adler_rows) -> ()", _png_filter_impl)


def png_filter(frames: torch.Tensor, filtered: Optional[torch.Tensor] = None, adler_rows: Optional[torch.Tensor] = None):
    """uint8 RGB frames [n, H, W, 3] in HBM -> (filtered rows uint8 [n, H, 1 + 3W], Adler-32 partials int32 [n, H, 2])
    (``torch.ops.sdv.k_png_filter`` -> sdv_png_filter_u8): per row the filter type libpng's heuristic picks among all five."""
    n, H, W = _png_frame_shape("png_filter", frames)
    if filtered is None:
        filtered = torch.empty((n, H, 1 + 3 * W), dtype=torch.uint8, device=frames.device)
    if adler_rows is None:
        adler_rows = torch.empty((n, H, 2), dtype=torch.int32, device=frames.device)
    _k_png_filter(frames, filtered, adler_rows)
    return filtered, adler_rows


def _png_pack_args(what, filtered, adler_rows, stripe_rows, header, scratch, out, offsets, needed, lengths):
    """The checks both packers share -> (n, H, W, stripes, the C arguments up to ``lengths``)."""
    if filtered.dtype != torch.uint8 or filtered.ndim != 3 or filtered.shape[2] % 3 != 1 or filtered.shape[2] < 4 or not filtered.is_contiguous():
        raise SdvHipError(f"{what}: filtered must be a contiguous uint8 [n, H, 1 + 3W] tensor, got {filtered.dtype} {tuple(filtered.shape)}")
    n, H, R = filtered.shape
    W = (R - 1) // 3
    if n < 1 or not (1 <= H <= PNG_MAX_DIM and 1 <= W <= PNG_MAX_DIM):
        raise SdvHipError(f"{what}: frame size must be 1 .. {PNG_MAX_DIM} and n >= 1, got n={n} H={H} W={W}")
    if adler_rows.dtype != torch.int32 or tuple(adler_rows.shape) != (n, H, 2) or not adler_rows.is_contiguous():
        raise SdvHipError(f"{what}: adler_rows must be a contiguous int32 [{n}, {H}, 2] tensor, got {adler_rows.dtype} {tuple(adler_rows.shape)}")
    stripes = png_stripes(H, W, stripe_rows)
    for name, t in (("header", header), ("scratch", scratch), ("out", out)):
        if t.dtype != torch.uint8 or t.ndim != 1 or not t.is_contiguous():
            raise SdvHipError(f"{what}: {name} must be a contiguous 1-D uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    if header.numel() != 33:
        raise SdvHipError(f"{what}: header must hold the 33 bytes signature + IHDR chunk, got {header.numel()}")
    if scratch.numel() < png_scratch_bytes(n, H, stripe_rows):
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n} frames of {stripes} stripes need "
                          f"{png_scratch_bytes(n, H, stripe_rows)}")
    if offsets.dtype != torch.int64 or offsets.numel() != n + 1 or not offsets.is_contiguous():
        raise SdvHipError(f"{what}: offsets must be a contiguous int64 vector of n + 1 = {n + 1} elements, got {offsets.dtype} x {offsets.numel()}")
    if needed.dtype != torch.int64 or needed.numel() != 1:
        raise SdvHipError(f"{what}: needed must be one int64 element, got {needed.dtype} x {needed.numel()}")
    if lengths is not None and (lengths.dtype != torch.uint8 or tuple(lengths.shape) != (n, stripes, 257) or not lengths.is_contiguous()):
        raise SdvHipError(f"{what}: lengths must be a contiguous uint8 [{n}, {stripes}, 257] tensor, got {lengths.dtype} {tuple(lengths.shape)}")
    return n, H, W, stripes


def _png_pack_pointers(filtered, adler_rows, n, H, W, stripe_rows, header, scratch, out, offsets, needed, lengths):
    return (_ptr(filtered, name="filtered"), _ptr(adler_rows, name="adler_rows"), n, H, W, stripe_rows, _ptr(header, name="header"), header.numel(),
            _ptr(scratch, name="scratch"), scratch.numel(), _ptr(out, name="out"), out.numel(), _ptr(offsets, name="offsets"),
            _ptr(needed, name="needed"), _ptr(lengths, name="lengths"))


def _png_deflate_pack_impl(filtered, adler_rows, stripe_rows, header, scratch, out, offsets, needed, lengths):
    n, H, W, _ = _png_pack_args("png_deflate_pack", filtered, adler_rows, stripe_rows, header, scratch, out, offsets, needed, lengths)
    lib = load()
    args = _png_pack_pointers(filtered, adler_rows, n, H, W, stripe_rows, header, scratch, out, offsets, needed, lengths)
    _launch("png_deflate_pack", dict(bytes=3.0 * filtered.numel()),
            lambda: _check(lib.sdv_png_deflate_pack(*args, _stream()), "sdv_png_deflate_pack"))


_k_png_deflate_pack = _defop("k_png_deflate_pack(Tensor filtered, Tensor adler_rows, int stripe_rows, Tensor header, Tensor(a!) scratch, Tensor(b!) out, "
                             "Tensor(c!) offsets, Tensor(d!) needed, Tensor(e!)? lengths) -> ()", _png_deflate_pack_impl)


def png_deflate_pack(filtered: torch.Tensor, adler_rows: torch.Tensor, stripe_rows: int, header: torch.Tensor, scratch: torch.Tensor,
                     out: torch.Tensor, offsets: torch.Tensor, needed: torch.Tensor, lengths: Optional[torch.Tensor] = None):
    """Huffman-code the filtered rows, one dynamic block per stripe, and pack complete PNG files into ``out``
    (``torch.ops.sdv.k_png_deflate_pack`` -> sdv_png_deflate_pack): ``out[offsets[k]:offsets[k + 1]]`` is file k with four zero bytes
    where the IDAT CRC goes.  When ``needed`` (= offsets[n]) exceeds ``out.numel()`` nothing was written to ``out``: call again with
    a buffer of that size.  ``lengths`` (uint8 [n, stripes, 257]) receives the code lengths of every stripe."""
    _k_png_deflate_pack(filtered, adler_rows, int(stripe_rows), header, scratch, out, offsets, needed, lengths)


def png_lz_scratch_bytes(n: int, H: int, W: int, stripe_rows: int) -> int:
    """sdv_png_deflate_lz_pack's token scratch: a uint32 token per filtered byte, a uint32 count per stripe, 320 code words per stripe."""
    S = n * png_stripes(H, 1, stripe_rows)
    return 4 * n * H * (1 + 3 * W) + 8 * ((S + 1) // 2) + 1280 * S


def _png_deflate_lz_pack_impl(filtered, adler_rows, stripe_rows, header, scratch, out, offsets, needed, lz_scratch, lengths, ll_lengths, d_lengths):
    what = "png_deflate_lz_pack"
    n, H, W, stripes = _png_pack_args(what, filtered, adler_rows, stripe_rows, header, scratch, out, offsets, needed, lengths)
    if lz_scratch.dtype != torch.uint8 or lz_scratch.ndim != 1 or not lz_scratch.is_contiguous():
        raise SdvHipError(f"{what}: lz_scratch must be a contiguous 1-D uint8 tensor, got {lz_scratch.dtype} {tuple(lz_scratch.shape)}")
    if lz_scratch.numel() < png_lz_scratch_bytes(n, H, W, stripe_rows):
        raise SdvHipError(f"{what}: lz_scratch holds {lz_scratch.numel()} bytes, {n * H * (1 + 3 * W)} filtered bytes in {n * stripes} stripes need "
                          f"{png_lz_scratch_bytes(n, H, W, stripe_rows)}")
    for name, t, syms in (("ll_lengths", ll_lengths, 286), ("d_lengths", d_lengths, 30)):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != (n, stripes, syms) or not t.is_contiguous()):
            raise SdvHipError(f"{what}: {name} must be a contiguous uint8 [{n}, {stripes}, {syms}] tensor, got {t.dtype} {tuple(t.shape)}")
    lib = load()
    args = _png_pack_pointers(filtered, adler_rows, n, H, W, stripe_rows, header, scratch, out, offsets, needed, lengths) + (
        _ptr(lz_scratch, name="lz_scratch"), lz_scratch.numel(), _ptr(ll_lengths, name="ll_lengths"), _ptr(d_lengths, name="d_lengths"))
    _launch(what, dict(bytes=11.0 * filtered.numel()), lambda: _check(lib.sdv_png_deflate_lz_pack(*args, _stream()), "sdv_png_deflate_lz_pack"))


_k_png_deflate_lz_pack = _defop("k_png_deflate_lz_pack(Tensor filtered, Tensor adler_rows, int stripe_rows, Tensor header, Tensor(a!) scratch, "
                                "Tensor(b!) out, Tensor(c!) offsets, Tensor(d!) needed, Tensor(e!) lz_scratch, Tensor(f!)? lengths, "
                                "Tensor(g!)? ll_lengths, Tensor(h!)? d_lengths) -> ()", _png_deflate_lz_pack_impl)


def png_deflate_lz_pack(filtered: torch.Tensor, adler_rows: torch.Tensor, stripe_rows: int, header: torch.Tensor, scratch: torch.Tensor,
                        out: torch.Tensor, offsets: torch.Tensor, needed: torch.Tensor, lz_scratch: torch.Tensor,
                        lengths: Optional[torch.Tensor] = None, ll_lengths: Optional[torch.Tensor] = None,
                        d_lengths: Optional[torch.Tensor] = None):
    """``png_deflate_pack`` with LZ77 matches (``torch.ops.sdv.k_png_deflate_lz_pack`` -> sdv_png_deflate_lz_pack; the stream rule is in
    sdv_hip.h "Matching mode").  ``lz_scratch`` (``png_lz_scratch_bytes``) holds the tokens afterwards: as int32, the first n H R
    words are the tokens (a stripe's from the index of its first filtered byte), the next n * stripes the token counts.  ``lengths``
    receives the literal prices, ``ll_lengths`` [n, stripes, 286] / ``d_lengths`` [n, stripes, 30] the final code lengths."""
    _k_png_deflate_lz_pack(filtered, adler_rows, int(stripe_rows), header, scratch, out, offsets, needed, lz_scratch, lengths, ll_lengths, d_lengths)


def _png_crc32_impl(out, offsets, needed, acc):
    if out.dtype != torch.uint8 or out.ndim != 1 or not out.is_contiguous():
        raise SdvHipError(f"png_crc32: out must be a contiguous 1-D uint8 tensor, got {out.dtype} {tuple(out.shape)}")
    if offsets.dtype != torch.int64 or offsets.ndim != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
        raise SdvHipError(f"png_crc32: offsets must be a contiguous int64 vector of n + 1 >= 2 elements, got {offsets.dtype} {tuple(offsets.shape)}")
    n = offsets.numel() - 1
    if needed.dtype != torch.int64 or needed.numel() != 1:
        raise SdvHipError(f"png_crc32: needed must be one int64 element, got {needed.dtype} x {needed.numel()}")
    if acc.dtype != torch.int32 or acc.numel() != n or not acc.is_contiguous():
        raise SdvHipError(f"png_crc32: acc must be a contiguous int32 vector of n = {n} elements, got {acc.dtype} x {acc.numel()}")
    lib = load()
    args = (_ptr(out, name="out"), out.numel(), _ptr(offsets, name="offsets"), _ptr(needed, name="needed"), n, _ptr(acc, name="acc"))
    _launch("png_crc32", dict(bytes=1.0 * out.numel()), lambda: _check(lib.sdv_png_crc32(*args, _stream()), "sdv_png_crc32"))


_k_png_crc32 = _defop("k_png_crc32(Tensor(a!) out, Tensor offsets, Tensor needed, Tensor(b!) acc) -> ()", _png_crc32_impl)


def png_crc32(out: torch.Tensor, offsets: torch.Tensor, needed: torch.Tensor, acc: torch.Tensor):
    """Fill the IDAT CRC-32 of every file a packer left in ``out`` (``torch.ops.sdv.k_png_crc32`` -> sdv_png_crc32), in place; nothing
    happens when ``needed`` exceeds ``out.numel()``.  ``acc``: int32 [n] workspace."""
    _k_png_crc32(out, offsets, needed, acc)


# ------------------------------------------------------------------------------------------------
# H.264 CAVLC intra encoder (csrc/sdv_h264.hip; h264_cavlc.py holds the workspaces and cuts the samples)
# ------------------------------------------------------------------------------------------------
H264_MAX_DIM = 16384
H264_VLC_WORDS = 656


def h264_mb_grid(H: int, W: int):
    return (int(H) + 15) // 16, (int(W) + 15) // 16


def h264_slice_bytes(mbw: int) -> int:
    """The most one slice of ``mbw`` macroblocks takes in a sample (sdv_hip.h "Capacity"): 4-byte length + NAL header + an RBSP of at
    most 400 bytes per macroblock and 8 of header and stop bit, with an emulation-prevention byte behind every second byte."""
    rbsp = 400 * int(mbw) + 8
    return 5 + rbsp + rbsp // 2


def h264_out_bytes(n: int, mbh: int, mbw: int) -> int:
    """The capacity sdv_h264_pack demands of ``out``."""
    return int(n) * int(mbh) * h264_slice_bytes(mbw)


def h264_scratch_bytes(n: int, mbh: int, mbw: int) -> int:
    """One slot per slice at an 8-byte stride, then an int64 start and an int32 length per slice."""
    return int(n) * int(mbh) * (((h264_slice_bytes(mbw) + 7) & ~7) + 12)


def _h264_u8(what, name, t, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "1-D" if shape is None else list(shape)
        raise SdvHipError(f"{what}: {name} must be a contiguous uint8 {want} tensor, got {getattr(t, 'dtype', type(t))} "
                          f"{tuple(getattr(t, 'shape', ()))}")


def _h264_planes_impl(frames, y, cb, cr):
    what = "h264_planes"
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise SdvHipError(f"{what}: frames must be a contiguous uint8 [n, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    n, H, W, _ = frames.shape
    if n < 1 or H % 2 or W % 2 or not (2 <= H <= H264_MAX_DIM and 2 <= W <= H264_MAX_DIM):
        raise SdvHipError(f"{what}: frame size must be even, 2 .. {H264_MAX_DIM}, and n >= 1, got n={n} H={H} W={W}")
    mbh, mbw = h264_mb_grid(H, W)
    _h264_u8(what, "y", y, (n, 16 * mbh, 16 * mbw))
    _h264_u8(what, "cb", cb, (n, 8 * mbh, 8 * mbw))
    _h264_u8(what, "cr", cr, (n, 8 * mbh, 8 * mbw))
    lib = load()
    args = (_ptr(frames, name="frames"), n, H, W, _ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"))
    _launch("h264_planes", dict(bytes=3.0 * n * H * W + 1.5 * y.numel()), lambda: _check(lib.sdv_h264_planes_u8(*args, _stream()), "sdv_h264_planes_u8"))


_k_h264_planes = _defop("k_h264_planes(Tensor frames, Tensor(a!) y, Tensor(b!) cb, Tensor(c!) cr) -> ()", _h264_planes_impl)


def h264_planes(frames: torch.Tensor, y: Optional[torch.Tensor] = None, cb: Optional[torch.Tensor] = None, cr: Optional[torch.Tensor] = None):
    """uint8 RGB ``[n, H, W, 3]`` -> padded studio-range BT.601 planes ``y [n, 16 mbh, 16 mbw]``, ``cb`` / ``cr [n, 8 mbh, 8 mbw]`` by the
    integer rule of sdv_hip.h (``torch.ops.sdv.k_h264_planes`` -> sdv_h264_planes_u8)."""
    if frames.ndim == 4 and y is None:
        mbh, mbw = h264_mb_grid(frames.shape[1], frames.shape[2])
        y = torch.empty((frames.shape[0], 16 * mbh, 16 * mbw), dtype=torch.uint8, device=frames.device)
        cb = torch.empty((frames.shape[0], 8 * mbh, 8 * mbw), dtype=torch.uint8, device=frames.device)
        cr = torch.empty_like(cb)
    _k_h264_planes(frames, y, cb, cr)
    return y, cb, cr


def _h264_plane_grid(what, y, cb, cr):
    if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.ndim != 3 or not y.is_contiguous() or y.shape[0] < 1 \
            or y.shape[1] % 16 or y.shape[2] % 16 or not y.shape[1] or not y.shape[2]:
        raise SdvHipError(f"{what}: y must be a contiguous uint8 [n, 16 mbh, 16 mbw] tensor, got {getattr(y, 'dtype', type(y))} "
                          f"{tuple(getattr(y, 'shape', ()))}")
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    _h264_u8(what, "cb", cb, (n, 8 * mbh, 8 * mbw))
    _h264_u8(what, "cr", cr, (n, 8 * mbh, 8 * mbw))
    return n, mbh, mbw


def _h264_encode_rows_impl(y, cb, cr, qp, first_index, scratch):
    what = "h264_encode_rows"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    _h264_u8(what, "scratch", scratch)
    if scratch.ndim != 1 or scratch.numel() < h264_scratch_bytes(n, mbh, mbw):
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {h264_scratch_bytes(n, mbh, mbw)}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(first_index) & 0x7fffffff,
            _ptr(scratch, name="scratch"), scratch.numel())
    _launch("h264_encode_rows", dict(bytes=1.5 * y.numel()), lambda: _check(lib.sdv_h264_encode_rows(*args, _stream()), "sdv_h264_encode_rows"))


_k_h264_encode_rows = _defop("k_h264_encode_rows(Tensor y, Tensor cb, Tensor cr, int qp, int first_index, Tensor(a!) scratch) -> ()",
                             _h264_encode_rows_impl)


def h264_encode_rows(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, first_index: int, scratch: torch.Tensor):
    """Code every macroblock row of every picture as one IDR slice into its slot of ``scratch`` (``h264_scratch_bytes``), by the stream
    rule of sdv_hip.h (``torch.ops.sdv.k_h264_encode_rows`` -> sdv_h264_encode_rows).  Picture k carries idr_pic_id (first_index + k) & 1."""
    _k_h264_encode_rows(y, cb, cr, int(qp), int(first_index), scratch)


H264_GOP_MAX = 256
H264_GOP_MAX_MBW = 1008


def h264_gop_slot_mbw(mbw: int) -> int:
    """The GOP path keeps a slice in the slot of a picture this many macroblocks wide (sdv_hip.h "Capacity of the GOP path"): a P slice
    carries an mb_skip_run per macroblock on top of the 3200 bits, and its header is not bounded by 8 bytes."""
    return int(mbw) + 1 + int(mbw) // 64


def h264_gop_out_bytes(n: int, mbh: int, mbw: int) -> int:
    """The capacity sdv_h264_pack demands of ``out`` behind ``h264_encode_gops``."""
    return h264_out_bytes(n, mbh, h264_gop_slot_mbw(mbw))


def h264_gop_scratch_bytes(n: int, mbh: int, mbw: int) -> int:
    return h264_scratch_bytes(n, mbh, h264_gop_slot_mbw(mbw))


def _h264_encode_gops_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch):
    what = "h264_encode_gops"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded with P pictures, got mbw={mbw}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_gop_scratch_bytes(n, mbh, mbw)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {need}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(first_index) & 0x7fffffff,
            _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"), _ptr(scratch, name="scratch"), scratch.numel())
    _launch("h264_encode_gops", dict(bytes=3.0 * y.numel()), lambda: _check(lib.sdv_h264_encode_gops(*args, _stream()), "sdv_h264_encode_gops"))


_k_h264_encode_gops = _defop("k_h264_encode_gops(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int first_index, Tensor(a!) ry, Tensor(b!) rcb, "
                             "Tensor(c!) rcr, Tensor(d!) scratch) -> ()", _h264_encode_gops_impl)


def h264_encode_gops(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, first_index: int, ry: torch.Tensor,
                     rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor):
    """Code the pictures in groups of ``gop``: picture k an IDR picture when ``k % gop == 0``, else a P picture predicted (zero motion)
    from the reconstruction of picture k - 1, by the stream rule of sdv_hip.h (``torch.ops.sdv.k_h264_encode_gops`` ->
    sdv_h264_encode_gops).  Slices go to the slots of ``scratch`` (``h264_gop_scratch_bytes``; pack with ``h264_gop_slot_mbw(mbw)``), the
    reconstruction of every picture to ``ry`` / ``rcb`` / ``rcr``."""
    _k_h264_encode_gops(y, cb, cr, int(qp), int(gop), int(first_index), ry, rcb, rcr, scratch)


H264_SEARCH_MAX = 16


def _h264_search_range(what, search):
    if not 2 <= search <= H264_SEARCH_MAX or search % 2:
        raise SdvHipError(f"{what}: search must be even, 2 .. {H264_SEARCH_MAX}, got {search} (0 is sdv_h264_encode_gops and never comes here)")


def _h264_motion_search_impl(y, qp, gop, search, mv, sad):
    what = "h264_motion_search"
    if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.ndim != 3 or not y.is_contiguous() or y.shape[0] < 1 \
            or y.shape[1] % 16 or y.shape[2] % 16 or not y.shape[1] or not y.shape[2]:
        raise SdvHipError(f"{what}: y must be a contiguous uint8 [n, 16 mbh, 16 mbw] tensor, got {getattr(y, 'dtype', type(y))} "
                          f"{tuple(getattr(y, 'shape', ()))}")
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    _h264_search_range(what, search)
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    if sad is not None and (sad.dtype != torch.int32 or not sad.is_contiguous() or tuple(sad.shape) != (n, mbh, mbw)):
        raise SdvHipError(f"{what}: sad must be a contiguous int32 {[n, mbh, mbw]} tensor, got {sad.dtype} {tuple(sad.shape)}")
    lib = load()
    args = (_ptr(y, name="y"), n, mbh, mbw, int(qp), int(gop), int(search), _ptr(mv, name="mv"), _ptr(sad, name="sad"))
    _launch("h264_motion_search", dict(bytes=2.0 * y.numel()), lambda: _check(lib.sdv_h264_motion_search(*args, _stream()), "sdv_h264_motion_search"))


_k_h264_motion_search = _defop("k_h264_motion_search(Tensor y, int qp, int gop, int search, Tensor(a!) mv, Tensor(b!)? sad) -> ()",
                               _h264_motion_search_impl)


def h264_motion_search(y: torch.Tensor, qp: int, gop: int, search: int, mv: torch.Tensor, sad: Optional[torch.Tensor] = None):
    """One even whole-sample vector per macroblock of every P picture (``k % gop != 0``) of the call: exhaustive search of source picture
    k against source picture k - 1 within ``search`` luma samples by the rule of sdv_hip_ext.h (``torch.ops.sdv.k_h264_motion_search`` ->
    sdv_h264_motion_search).  ``mv``: int16 ``[n, mbh, mbw, 2]`` (vx, vy), zeros for IDR pictures; ``sad``: int32 ``[n, mbh, mbw]``, the
    winner's source SAD (optional)."""
    _k_h264_motion_search(y, int(qp), int(gop), int(search), mv, sad)


def _h264_mbinfo_check(what, mbinfo, n, mbh, mbw):
    """The side information tensor of sdv_hip_h264_lf.h: int32 [n, mbh, mbw], contiguous."""
    if not isinstance(mbinfo, torch.Tensor) or mbinfo.dtype != torch.int32 or not mbinfo.is_contiguous() or tuple(mbinfo.shape) != (n, mbh, mbw):
        raise SdvHipError(f"{what}: mbinfo must be a contiguous int32 {[n, mbh, mbw]} tensor, got {getattr(mbinfo, 'dtype', type(mbinfo))} "
                          f"{tuple(getattr(mbinfo, 'shape', ()))}")


def _h264_mbinfo_args(what, mbinfo, n, mbh, mbw):
    _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    return _ptr(mbinfo, name="mbinfo"), mbinfo.numel()


def _h264_encode_gop_step_impl(y, cb, cr, qp, gop, k, search, first_index, mv, ry, rcb, rcr, scratch, mbinfo=None):
    what = "h264_encode_gop_step" if mbinfo is None else "h264_encode_gop_step_lf"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if mbinfo is not None:
        _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    _h264_search_range(what, search)
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded with P pictures, got mbw={mbw}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_gop_scratch_bytes(n, mbh, mbw)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {need}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(k), int(search),
            int(first_index) & 0x7fffffff, _ptr(mv, name="mv"), _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"),
            _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_gop_step_lf", dict(bytes=3.0 * y.numel() / min(gop, n)),
                lambda: _check(lib.sdv_h264_encode_gop_step_lf(*args, *lf, _stream()), "sdv_h264_encode_gop_step_lf"))
        return
    _launch("h264_encode_gop_step", dict(bytes=3.0 * y.numel() / min(gop, n)),
            lambda: _check(lib.sdv_h264_encode_gop_step(*args, _stream()), "sdv_h264_encode_gop_step"))


_k_h264_encode_gop_step = _defop("k_h264_encode_gop_step(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int first_index, "
                                 "Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch) -> ()", _h264_encode_gop_step_impl)


def h264_encode_gop_step(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, first_index: int,
                         mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor):
    """``h264_encode_gops`` for the pictures at position ``k`` of every GOP of the call, motion-compensated with the vectors ``mv`` (rule of
    sdv_hip_ext.h; ``torch.ops.sdv.k_h264_encode_gop_step`` -> sdv_h264_encode_gop_step).  Call it for k = 0 .. min(gop, n) - 1 in order on
    one stream: picture k predicts from the reconstruction the launch before it left in ``ry`` / ``rcb`` / ``rcr``."""
    _k_h264_encode_gop_step(y, cb, cr, int(qp), int(gop), int(k), int(search), int(first_index), mv, ry, rcb, rcr, scratch)


H264_SUBPELS = (1, 2, 4)


def _h264_subpel_value(what, subpel):
    if subpel not in H264_SUBPELS:
        raise SdvHipError(f"{what}: subpel must be 1, 2 or 4, got {subpel} (0 is sdv_h264_motion_search / sdv_h264_encode_gop_step and never comes here)")


def _h264_motion_search_sub_impl(y, qp, gop, search, subpel, mv, sad):
    what = "h264_motion_search_sub"
    if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.ndim != 3 or not y.is_contiguous() or y.shape[0] < 1 \
            or y.shape[1] % 16 or y.shape[2] % 16 or not y.shape[1] or not y.shape[2]:
        raise SdvHipError(f"{what}: y must be a contiguous uint8 [n, 16 mbh, 16 mbw] tensor, got {getattr(y, 'dtype', type(y))} "
                          f"{tuple(getattr(y, 'shape', ()))}")
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    _h264_search_range(what, search)
    _h264_subpel_value(what, subpel)
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    if sad is not None and (sad.dtype != torch.int32 or not sad.is_contiguous() or tuple(sad.shape) != (n, mbh, mbw)):
        raise SdvHipError(f"{what}: sad must be a contiguous int32 {[n, mbh, mbw]} tensor, got {sad.dtype} {tuple(sad.shape)}")
    lib = load()
    args = (_ptr(y, name="y"), n, mbh, mbw, int(qp), int(gop), int(search), int(subpel), _ptr(mv, name="mv"), _ptr(sad, name="sad"))
    _launch("h264_motion_search_sub", dict(bytes=2.0 * y.numel()),
            lambda: _check(lib.sdv_h264_motion_search_sub(*args, _stream()), "sdv_h264_motion_search_sub"))


_k_h264_motion_search_sub = _defop("k_h264_motion_search_sub(Tensor y, int qp, int gop, int search, int subpel, Tensor(a!) mv, Tensor(b!)? sad) -> ()",
                                   _h264_motion_search_sub_impl)


def h264_motion_search_sub(y: torch.Tensor, qp: int, gop: int, search: int, subpel: int, mv: torch.Tensor, sad: Optional[torch.Tensor] = None):
    """``h264_motion_search`` on the grid of 1 / ``subpel`` samples (``subpel`` 1, 2 or 4): every whole-sample vector, then a half- and a
    quarter-sample refinement by the rule of sdv_hip_h264_sub.h (``torch.ops.sdv.k_h264_motion_search_sub`` -> sdv_h264_motion_search_sub).
    ``mv``: int16 ``[n, mbh, mbw, 2]`` (vx, vy) in QUARTER samples, zeros for IDR pictures; ``sad``: int32 ``[n, mbh, mbw]`` (optional)."""
    _k_h264_motion_search_sub(y, int(qp), int(gop), int(search), int(subpel), mv, sad)


def _h264_encode_gop_step_sub_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, mbinfo=None):
    what = "h264_encode_gop_step_sub" if mbinfo is None else "h264_encode_gop_step_sub_lf"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if mbinfo is not None:
        _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    _h264_search_range(what, search)
    _h264_subpel_value(what, subpel)
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded with P pictures, got mbw={mbw}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_gop_scratch_bytes(n, mbh, mbw)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {need}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(k), int(search), int(subpel),
            int(first_index) & 0x7fffffff, _ptr(mv, name="mv"), _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"),
            _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_gop_step_sub_lf", dict(bytes=3.0 * y.numel() / min(gop, n)),
                lambda: _check(lib.sdv_h264_encode_gop_step_sub_lf(*args, *lf, _stream()), "sdv_h264_encode_gop_step_sub_lf"))
        return
    _launch("h264_encode_gop_step_sub", dict(bytes=3.0 * y.numel() / min(gop, n)),
            lambda: _check(lib.sdv_h264_encode_gop_step_sub(*args, _stream()), "sdv_h264_encode_gop_step_sub"))


_k_h264_encode_gop_step_sub = _defop("k_h264_encode_gop_step_sub(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                     "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch) -> ()",
                                     _h264_encode_gop_step_sub_impl)


def h264_encode_gop_step_sub(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                             first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor):
    """``h264_encode_gop_step`` with the quarter-sample vectors ``mv`` of ``h264_motion_search_sub``: interpolated luma and chroma
    prediction (rule of sdv_hip_h264_sub.h; ``torch.ops.sdv.k_h264_encode_gop_step_sub`` -> sdv_h264_encode_gop_step_sub).  Call it for
    k = 0 .. min(gop, n) - 1 in order on one stream."""
    _k_h264_encode_gop_step_sub(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch)


def _h264_encode_idr4_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo=None):
    what = "h264_encode_idr4" if mbinfo is None else "h264_encode_idr4_lf"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if mbinfo is not None:
        _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded in the GOP path's slots, got mbw={mbw}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_gop_scratch_bytes(n, mbh, mbw)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {need}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(first_index) & 0x7fffffff,
            _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"), _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_idr4_lf", dict(bytes=3.0 * y.numel() / gop),
                lambda: _check(lib.sdv_h264_encode_idr4_lf(*args, *lf, _stream()), "sdv_h264_encode_idr4_lf"))
        return
    _launch("h264_encode_idr4", dict(bytes=3.0 * y.numel() / gop), lambda: _check(lib.sdv_h264_encode_idr4(*args, _stream()), "sdv_h264_encode_idr4"))


_k_h264_encode_idr4 = _defop("k_h264_encode_idr4(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int first_index, Tensor(a!) ry, Tensor(b!) rcb, "
                             "Tensor(c!) rcr, Tensor(d!) scratch) -> ()", _h264_encode_idr4_impl)


def h264_encode_idr4(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, first_index: int, ry: torch.Tensor,
                     rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor):
    """Code the IDR pictures of a call (positions ``k % gop == 0``; every picture at ``gop`` 1) with Intra4x4 prediction: per macroblock
    ``I_NxN`` against Intra16x16 DC by the stream rule of sdv_hip_h264_i4.h (``torch.ops.sdv.k_h264_encode_idr4`` ->
    sdv_h264_encode_idr4).  Slices go to the GOP slots of ``scratch`` (``h264_gop_scratch_bytes``; pack with ``h264_gop_slot_mbw(mbw)``), all
    their reconstructed samples to ``ry`` / ``rcb`` / ``rcr``; the P pictures follow through ``h264_encode_gop_step`` / ``_sub`` for
    k = 1 .. min(gop, n) - 1."""
    _k_h264_encode_idr4(y, cb, cr, int(qp), int(gop), int(first_index), ry, rcb, rcr, scratch)


def _h264_encode_gop_step_lf_impl(y, cb, cr, qp, gop, k, search, first_index, mv, ry, rcb, rcr, scratch, mbinfo):
    _h264_encode_gop_step_impl(y, cb, cr, qp, gop, k, search, first_index, mv, ry, rcb, rcr, scratch, _h264_mbinfo_given("h264_encode_gop_step_lf", mbinfo))


def _h264_encode_gop_step_sub_lf_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, mbinfo):
    _h264_encode_gop_step_sub_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch,
                                   _h264_mbinfo_given("h264_encode_gop_step_sub_lf", mbinfo))


def _h264_encode_idr4_lf_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo):
    _h264_encode_idr4_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, _h264_mbinfo_given("h264_encode_idr4_lf", mbinfo))


def _h264_mbinfo_given(what, mbinfo):
    if mbinfo is None:
        raise SdvHipError(f"{what}: mbinfo is missing")
    return mbinfo


H264_LF_WAVES_MAX = 16


def _h264_deblock_impl(ry, rcb, rcr, qp, gop, k, subpel, mbinfo, mv, waves):
    what = "h264_deblock"
    n, mbh, mbw = _h264_plane_grid(what, ry, rcb, rcr)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    if subpel not in (0,) + H264_SUBPELS:
        raise SdvHipError(f"{what}: subpel must be 0, 1, 2 or 4, got {subpel}")
    if not 0 <= waves <= H264_LF_WAVES_MAX:
        raise SdvHipError(f"{what}: waves must be 0 (the default) .. {H264_LF_WAVES_MAX}, got {waves}")
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    lib = load()
    lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
    args = (_ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"), n, mbh, mbw, int(qp), int(gop), int(k), int(subpel), *lf,
            _ptr(mv, name="mv"), int(waves))
    _launch("h264_deblock", dict(bytes=3.0 * ry.numel() / min(gop, n)), lambda: _check(lib.sdv_h264_deblock(*args, _stream()), "sdv_h264_deblock"))


_k_h264_encode_gop_step_lf = _defop("k_h264_encode_gop_step_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int first_index, "
                                    "Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, Tensor(e!) mbinfo) -> ()",
                                    _h264_encode_gop_step_lf_impl)
_k_h264_encode_gop_step_sub_lf = _defop("k_h264_encode_gop_step_sub_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                        "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, "
                                        "Tensor(e!) mbinfo) -> ()", _h264_encode_gop_step_sub_lf_impl)
_k_h264_encode_idr4_lf = _defop("k_h264_encode_idr4_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int first_index, Tensor(a!) ry, Tensor(b!) rcb, "
                                "Tensor(c!) rcr, Tensor(d!) scratch, Tensor(e!) mbinfo) -> ()", _h264_encode_idr4_lf_impl)
_k_h264_deblock = _defop("k_h264_deblock(Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, int qp, int gop, int k, int subpel, Tensor mbinfo, Tensor mv, "
                         "int waves) -> ()", _h264_deblock_impl)


def h264_encode_gop_step_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, first_index: int,
                            mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor, mbinfo: torch.Tensor):
    """``h264_encode_gop_step`` for a stream with the loop filter on (sdv_hip_h264_lf.h; ``torch.ops.sdv.k_h264_encode_gop_step_lf`` ->
    sdv_h264_encode_gop_step_lf): the slice headers say so, and ``mbinfo`` (int32 ``[n, mbh, mbw]``) takes the side information word of
    every macroblock coded.  ``h264_deblock`` for the same ``k`` follows before the next position."""
    _k_h264_encode_gop_step_lf(y, cb, cr, int(qp), int(gop), int(k), int(search), int(first_index), mv, ry, rcb, rcr, scratch, mbinfo)


def h264_encode_gop_step_sub_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                                first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor,
                                mbinfo: torch.Tensor):
    """``h264_encode_gop_step_sub`` for a stream with the loop filter on (``torch.ops.sdv.k_h264_encode_gop_step_sub_lf`` ->
    sdv_h264_encode_gop_step_sub_lf); see ``h264_encode_gop_step_lf``."""
    _k_h264_encode_gop_step_sub_lf(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch,
                                   mbinfo)


def h264_encode_idr4_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, first_index: int, ry: torch.Tensor,
                        rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor, mbinfo: torch.Tensor):
    """``h264_encode_idr4`` for a stream with the loop filter on (``torch.ops.sdv.k_h264_encode_idr4_lf`` -> sdv_h264_encode_idr4_lf); see
    ``h264_encode_gop_step_lf``."""
    _k_h264_encode_idr4_lf(y, cb, cr, int(qp), int(gop), int(first_index), ry, rcb, rcr, scratch, mbinfo)


def h264_deblock(ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, qp: int, gop: int, k: int, subpel: int, mbinfo: torch.Tensor,
                 mv: torch.Tensor, waves: int = 0):
    """The in-loop deblocking filter (8.7; rule of sdv_hip_h264_lf.h) on the reconstruction planes of the pictures at position ``k`` of
    every GOP, in place (``torch.ops.sdv.k_h264_deblock`` -> sdv_h264_deblock), from the side information ``mbinfo`` and the vectors
    ``mv`` (even whole samples with ``subpel`` 0, quarter samples else).  Enqueue it after the encode launch of position ``k`` and before
    that of ``k + 1``.  ``waves`` 0 is the default workgroup size, 1 .. 16 explicit; the result does not depend on it."""
    _k_h264_deblock(ry, rcb, rcr, int(qp), int(gop), int(k), int(subpel), mbinfo, mv, int(waves))


# ---- macroblock partitions (include/sdv_hip_h264_part.h): four quarter-sample vectors per macroblock ----
H264_PART_SUBPELS = (0,) + H264_SUBPELS


def _h264_part_subpel_value(what, subpel):
    if subpel not in H264_PART_SUBPELS:
        raise SdvHipError(f"{what}: subpel must be 0, 1, 2 or 4, got {subpel}")


def _h264_part_mv_check(what, mv, n, mbh, mbw):
    """The vector tensor of sdv_hip_h264_part.h: int16 [n, mbh, mbw, 4, 2], contiguous."""
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or not mv.is_contiguous() or tuple(mv.shape) != (n, mbh, mbw, 4, 2):
        raise SdvHipError(f"{what}: mv must be a contiguous int16 {[n, mbh, mbw, 4, 2]} tensor, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")


def _h264_motion_search_part_impl(y, qp, gop, search, subpel, mv, sad):
    what = "h264_motion_search_part"
    if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.ndim != 3 or not y.is_contiguous() or y.shape[0] < 1 \
            or y.shape[1] % 16 or y.shape[2] % 16 or not y.shape[1] or not y.shape[2]:
        raise SdvHipError(f"{what}: y must be a contiguous uint8 [n, 16 mbh, 16 mbw] tensor, got {getattr(y, 'dtype', type(y))} "
                          f"{tuple(getattr(y, 'shape', ()))}")
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    _h264_search_range(what, search)
    _h264_part_subpel_value(what, subpel)
    _h264_part_mv_check(what, mv, n, mbh, mbw)
    if sad is not None and (sad.dtype != torch.int32 or not sad.is_contiguous() or tuple(sad.shape) != (n, mbh, mbw, 5)):
        raise SdvHipError(f"{what}: sad must be a contiguous int32 {[n, mbh, mbw, 5]} tensor, got {sad.dtype} {tuple(sad.shape)}")
    lib = load()
    args = (_ptr(y, name="y"), n, mbh, mbw, int(qp), int(gop), int(search), int(subpel), _ptr(mv, name="mv"), mv.numel(), _ptr(sad, name="sad"),
            0 if sad is None else sad.numel())
    _launch("h264_motion_search_part", dict(bytes=2.0 * y.numel()),
            lambda: _check(lib.sdv_h264_motion_search_part(*args, _stream()), "sdv_h264_motion_search_part"))


_k_h264_motion_search_part = _defop("k_h264_motion_search_part(Tensor y, int qp, int gop, int search, int subpel, Tensor(a!) mv, Tensor(b!)? sad) -> ()",
                                    _h264_motion_search_part_impl)


def h264_motion_search_part(y: torch.Tensor, qp: int, gop: int, search: int, subpel: int, mv: torch.Tensor, sad: Optional[torch.Tensor] = None):
    """``h264_motion_search_sub`` that also keeps the winner of every 8x8 quadrant and decides between them and the 16x16 winner by the
    rule of sdv_hip_h264_part.h (``torch.ops.sdv.k_h264_motion_search_part`` -> sdv_h264_motion_search_part); ``subpel`` 0, 1, 2 or 4.
    ``mv``: int16 ``[n, mbh, mbw, 4, 2]`` in QUARTER samples (four equal vectors where the 16x16 winner stands), zeros for IDR pictures;
    ``sad``: int32 ``[n, mbh, mbw, 5]`` (optional), the source SADs of the four quadrant winners and of the 16x16 winner."""
    _k_h264_motion_search_part(y, int(qp), int(gop), int(search), int(subpel), mv, sad)


def _h264_encode_gop_step_part_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, mbinfo=None):
    what = "h264_encode_gop_step_part" if mbinfo is None else "h264_encode_gop_step_part_lf"
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if mbinfo is not None:
        _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    _h264_search_range(what, search)
    _h264_part_subpel_value(what, subpel)
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded with P pictures, got mbw={mbw}")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    _h264_part_mv_check(what, mv, n, mbh, mbw)
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_gop_scratch_bytes(n, mbh, mbw)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {need}")
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(k), int(search), int(subpel),
            int(first_index) & 0x7fffffff, _ptr(mv, name="mv"), mv.numel(), _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"),
            _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_gop_step_part_lf", dict(bytes=3.0 * y.numel() / min(gop, n)),
                lambda: _check(lib.sdv_h264_encode_gop_step_part_lf(*args, *lf, _stream()), "sdv_h264_encode_gop_step_part_lf"))
        return
    _launch("h264_encode_gop_step_part", dict(bytes=3.0 * y.numel() / min(gop, n)),
            lambda: _check(lib.sdv_h264_encode_gop_step_part(*args, _stream()), "sdv_h264_encode_gop_step_part"))


def _h264_encode_gop_step_part_lf_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, mbinfo):
    _h264_encode_gop_step_part_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch,
                                    _h264_mbinfo_given("h264_encode_gop_step_part_lf", mbinfo))


def _h264_deblock_part_impl(ry, rcb, rcr, qp, gop, k, mbinfo, mv, waves):
    what = "h264_deblock_part"
    n, mbh, mbw = _h264_plane_grid(what, ry, rcb, rcr)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    if not 0 <= waves <= H264_LF_WAVES_MAX:
        raise SdvHipError(f"{what}: waves must be 0 (the default) .. {H264_LF_WAVES_MAX}, got {waves}")
    _h264_part_mv_check(what, mv, n, mbh, mbw)
    lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
    lib = load()
    args = (_ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"), n, mbh, mbw, int(qp), int(gop), int(k), *lf, _ptr(mv, name="mv"),
            mv.numel(), int(waves))
    _launch("h264_deblock_part", dict(bytes=3.0 * ry.numel() / min(gop, n)),
            lambda: _check(lib.sdv_h264_deblock_part(*args, _stream()), "sdv_h264_deblock_part"))


_k_h264_encode_gop_step_part = _defop("k_h264_encode_gop_step_part(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                      "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch) -> ()",
                                      _h264_encode_gop_step_part_impl)
_k_h264_encode_gop_step_part_lf = _defop("k_h264_encode_gop_step_part_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                         "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, "
                                         "Tensor(e!) mbinfo) -> ()", _h264_encode_gop_step_part_lf_impl)
_k_h264_deblock_part = _defop("k_h264_deblock_part(Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, int qp, int gop, int k, Tensor mbinfo, Tensor mv, "
                              "int waves) -> ()", _h264_deblock_part_impl)


def h264_encode_gop_step_part(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                              first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor):
    """``h264_encode_gop_step_sub`` with the four vectors per macroblock of ``h264_motion_search_part`` (``mv`` int16 ``[n, mbh, mbw, 4, 2]``,
    quarter samples; ``subpel`` 0, 1, 2 or 4): ``P_8x8`` where they differ, today's macroblock types where they are equal (rule of
    sdv_hip_h264_part.h; ``torch.ops.sdv.k_h264_encode_gop_step_part`` -> sdv_h264_encode_gop_step_part).  Call it for
    k = 0 .. min(gop, n) - 1 in order on one stream."""
    _k_h264_encode_gop_step_part(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch)


def h264_encode_gop_step_part_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                                 first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor,
                                 mbinfo: torch.Tensor):
    """``h264_encode_gop_step_part`` for a stream with the loop filter on (``torch.ops.sdv.k_h264_encode_gop_step_part_lf`` ->
    sdv_h264_encode_gop_step_part_lf): ``mbinfo`` takes the side information words with bits 19 .. 22; ``h264_deblock_part`` for the same
    ``k`` follows before the next position."""
    _k_h264_encode_gop_step_part_lf(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch,
                                    mbinfo)


def h264_deblock_part(ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, qp: int, gop: int, k: int, mbinfo: torch.Tensor, mv: torch.Tensor,
                      waves: int = 0):
    """``h264_deblock`` with four vectors per macroblock (``mv`` int16 ``[n, mbh, mbw, 4, 2]``, always quarter samples) and the side
    information of ``h264_encode_gop_step_part_lf`` (``torch.ops.sdv.k_h264_deblock_part`` -> sdv_h264_deblock_part)."""
    _k_h264_deblock_part(ry, rcb, rcr, int(qp), int(gop), int(k), mbinfo, mv, int(waves))


# ---- row slices (include/sdv_hip_h264_seg.h): up to 16 slices per macroblock row, one wave each ----
H264_ROW_SLICES_MAX = 16
H264_SEG_SLOT_ROWS = 1024


def h264_row_segments(mbh: int, mbw: int, row_slices: int) -> int:
    """The slices written per macroblock row with the setting ``row_slices``: ``max(1, min(row_slices, mbw, 1024 // mbh))`` - at most one
    per macroblock, and at most the 1024 slot rows a picture that sdv_h264_pack accepts.  The frame size alone decides."""
    return max(1, min(int(row_slices), int(mbw), H264_SEG_SLOT_ROWS // int(mbh)))


def h264_seg_slot_mbw(mbw: int, segs: int) -> int:
    """A slice of at most ``ceil(mbw / segs)`` macroblocks lies in the slot of an intra picture this many macroblocks wide."""
    return h264_gop_slot_mbw((int(mbw) + int(segs) - 1) // int(segs))


def h264_seg_scratch_bytes(n: int, mbh: int, mbw: int, segs: int) -> int:
    """The intra layout at ``(n, mbh * segs, h264_seg_slot_mbw(mbw, segs))``."""
    return h264_scratch_bytes(n, int(mbh) * int(segs), h264_seg_slot_mbw(mbw, segs))


def h264_seg_out_bytes(n: int, mbh: int, mbw: int, segs: int) -> int:
    """The capacity sdv_h264_pack demands of ``out`` behind the seg entry points."""
    return h264_out_bytes(n, int(mbh) * int(segs), h264_seg_slot_mbw(mbw, segs))


def _h264_seg_common(what, y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo, segs):
    n, mbh, mbw = _h264_plane_grid(what, y, cb, cr)
    if mbinfo is not None:
        _h264_mbinfo_check(what, mbinfo, n, mbh, mbw)
    if not 0 <= qp <= 51:
        raise SdvHipError(f"{what}: qp must be 0 .. 51, got {qp}")
    if not 1 <= gop <= H264_GOP_MAX:
        raise SdvHipError(f"{what}: gop must be 1 .. {H264_GOP_MAX}, got {gop}")
    if mbw > H264_GOP_MAX_MBW:
        raise SdvHipError(f"{what}: pictures wider than {H264_GOP_MAX_MBW} macroblocks are not coded in the GOP path's slots, got mbw={mbw}")
    if not 1 <= segs <= min(mbw, H264_ROW_SLICES_MAX):
        raise SdvHipError(f"{what}: segs must be 1 .. min(mbw, {H264_ROW_SLICES_MAX}) = {min(mbw, H264_ROW_SLICES_MAX)}, got {segs}")
    if mbh * segs > H264_SEG_SLOT_ROWS:
        raise SdvHipError(f"{what}: mbh * segs = {mbh * segs} is above the {H264_SEG_SLOT_ROWS} slot rows a picture may have")
    if first_index < 0:
        raise SdvHipError(f"{what}: first_index must be >= 0, got {first_index}")
    _h264_u8(what, "ry", ry, y.shape)
    _h264_u8(what, "rcb", rcb, cb.shape)
    _h264_u8(what, "rcr", rcr, cr.shape)
    _h264_u8(what, "scratch", scratch)
    need = h264_seg_scratch_bytes(n, mbh, mbw, segs)
    if scratch.ndim != 1 or scratch.numel() < need:
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh * segs} slices of at most {(mbw + segs - 1) // segs} "
                          f"macroblocks need {need}")
    return n, mbh, mbw


def _h264_encode_gop_step_seg_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, segs, mbinfo=None):
    what = "h264_encode_gop_step_seg" if mbinfo is None else "h264_encode_gop_step_seg_lf"
    n, mbh, mbw = _h264_seg_common(what, y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo, segs)
    if not 0 <= k < min(gop, n):
        raise SdvHipError(f"{what}: position k must be 0 .. min(gop, n) - 1 = {min(gop, n) - 1}, got {k}")
    _h264_search_range(what, search)
    _h264_part_subpel_value(what, subpel)
    _h264_part_mv_check(what, mv, n, mbh, mbw)
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(k), int(search), int(subpel),
            int(first_index) & 0x7fffffff, _ptr(mv, name="mv"), mv.numel(), _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"),
            _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_gop_step_seg_lf", dict(bytes=3.0 * y.numel() / min(gop, n)),
                lambda: _check(lib.sdv_h264_encode_gop_step_seg_lf(*args, *lf, int(segs), _stream()), "sdv_h264_encode_gop_step_seg_lf"))
        return
    _launch("h264_encode_gop_step_seg", dict(bytes=3.0 * y.numel() / min(gop, n)),
            lambda: _check(lib.sdv_h264_encode_gop_step_seg(*args, int(segs), _stream()), "sdv_h264_encode_gop_step_seg"))


def _h264_encode_gop_step_seg_lf_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, mbinfo, segs):
    _h264_encode_gop_step_seg_impl(y, cb, cr, qp, gop, k, search, subpel, first_index, mv, ry, rcb, rcr, scratch, segs,
                                   _h264_mbinfo_given("h264_encode_gop_step_seg_lf", mbinfo))


def _h264_encode_idr4_seg_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, segs, mbinfo=None):
    what = "h264_encode_idr4_seg" if mbinfo is None else "h264_encode_idr4_seg_lf"
    n, mbh, mbw = _h264_seg_common(what, y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo, segs)
    lib = load()
    args = (_ptr(y, name="y"), _ptr(cb, name="cb"), _ptr(cr, name="cr"), n, mbh, mbw, int(qp), int(gop), int(first_index) & 0x7fffffff,
            _ptr(ry, name="ry"), _ptr(rcb, name="rcb"), _ptr(rcr, name="rcr"), _ptr(scratch, name="scratch"), scratch.numel())
    if mbinfo is not None:
        lf = _h264_mbinfo_args(what, mbinfo, n, mbh, mbw)
        _launch("h264_encode_idr4_seg_lf", dict(bytes=3.0 * y.numel() / gop),
                lambda: _check(lib.sdv_h264_encode_idr4_seg_lf(*args, *lf, int(segs), _stream()), "sdv_h264_encode_idr4_seg_lf"))
        return
    _launch("h264_encode_idr4_seg", dict(bytes=3.0 * y.numel() / gop),
            lambda: _check(lib.sdv_h264_encode_idr4_seg(*args, int(segs), _stream()), "sdv_h264_encode_idr4_seg"))


def _h264_encode_idr4_seg_lf_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, mbinfo, segs):
    _h264_encode_idr4_seg_impl(y, cb, cr, qp, gop, first_index, ry, rcb, rcr, scratch, segs, _h264_mbinfo_given("h264_encode_idr4_seg_lf", mbinfo))


_k_h264_encode_gop_step_seg = _defop("k_h264_encode_gop_step_seg(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                     "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, int segs) -> ()",
                                     _h264_encode_gop_step_seg_impl)
_k_h264_encode_gop_step_seg_lf = _defop("k_h264_encode_gop_step_seg_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int k, int search, int subpel, "
                                        "int first_index, Tensor mv, Tensor(a!) ry, Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, "
                                        "Tensor(e!) mbinfo, int segs) -> ()", _h264_encode_gop_step_seg_lf_impl)
_k_h264_encode_idr4_seg = _defop("k_h264_encode_idr4_seg(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int first_index, Tensor(a!) ry, "
                                 "Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, int segs) -> ()", _h264_encode_idr4_seg_impl)
_k_h264_encode_idr4_seg_lf = _defop("k_h264_encode_idr4_seg_lf(Tensor y, Tensor cb, Tensor cr, int qp, int gop, int first_index, Tensor(a!) ry, "
                                    "Tensor(b!) rcb, Tensor(c!) rcr, Tensor(d!) scratch, Tensor(e!) mbinfo, int segs) -> ()",
                                    _h264_encode_idr4_seg_lf_impl)


def h264_encode_gop_step_seg(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                             first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor,
                             segs: int):
    """``h264_encode_gop_step_part`` with ``segs`` slices per macroblock row, one wave each (rule of sdv_hip_h264_seg.h;
    ``torch.ops.sdv.k_h264_encode_gop_step_seg`` -> sdv_h264_encode_gop_step_seg).  ``scratch`` holds ``h264_seg_scratch_bytes``; pack with
    ``h264_pack(scratch, n, mbh * segs, h264_seg_slot_mbw(mbw, segs), ...)``.  ``segs`` 1 writes ``h264_encode_gop_step_part``'s bytes."""
    _k_h264_encode_gop_step_seg(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch, int(segs))


def h264_encode_gop_step_seg_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, k: int, search: int, subpel: int,
                                first_index: int, mv: torch.Tensor, ry: torch.Tensor, rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor,
                                mbinfo: torch.Tensor, segs: int):
    """``h264_encode_gop_step_seg`` for a stream with the loop filter on (``torch.ops.sdv.k_h264_encode_gop_step_seg_lf`` ->
    sdv_h264_encode_gop_step_seg_lf): ``mbinfo`` takes the side information words; ``h264_deblock_part`` for the same ``k`` follows."""
    _k_h264_encode_gop_step_seg_lf(y, cb, cr, int(qp), int(gop), int(k), int(search), int(subpel), int(first_index), mv, ry, rcb, rcr, scratch,
                                   mbinfo, int(segs))


def h264_encode_idr4_seg(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, first_index: int, ry: torch.Tensor,
                         rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor, segs: int):
    """``h264_encode_idr4`` with ``segs`` slices per macroblock row (``torch.ops.sdv.k_h264_encode_idr4_seg`` -> sdv_h264_encode_idr4_seg)."""
    _k_h264_encode_idr4_seg(y, cb, cr, int(qp), int(gop), int(first_index), ry, rcb, rcr, scratch, int(segs))


def h264_encode_idr4_seg_lf(y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, qp: int, gop: int, first_index: int, ry: torch.Tensor,
                            rcb: torch.Tensor, rcr: torch.Tensor, scratch: torch.Tensor, mbinfo: torch.Tensor, segs: int):
    """``h264_encode_idr4_seg`` with the side information of the loop filter (``torch.ops.sdv.k_h264_encode_idr4_seg_lf`` ->
    sdv_h264_encode_idr4_seg_lf)."""
    _k_h264_encode_idr4_seg_lf(y, cb, cr, int(qp), int(gop), int(first_index), ry, rcb, rcr, scratch, mbinfo, int(segs))


def _h264_pack_impl(scratch, n, mbh, mbw, out, offsets):
    what = "h264_pack"
    if n < 1 or not (1 <= mbh <= 1024 and 1 <= mbw <= 1024):
        raise SdvHipError(f"{what}: macroblock grid must be 1 .. 1024 and n >= 1, got n={n} mbh={mbh} mbw={mbw}")
    _h264_u8(what, "scratch", scratch)
    if scratch.ndim != 1 or scratch.numel() < h264_scratch_bytes(n, mbh, mbw):
        raise SdvHipError(f"{what}: scratch holds {scratch.numel()} bytes, {n * mbh} slices of {mbw} macroblocks need {h264_scratch_bytes(n, mbh, mbw)}")
    _h264_u8(what, "out", out)
    if out.ndim != 1 or out.numel() < h264_out_bytes(n, mbh, mbw):
        raise SdvHipError(f"{what}: out holds {out.numel()} bytes, the capacity bound of {n * mbh} slices of {mbw} macroblocks is "
                          f"{h264_out_bytes(n, mbh, mbw)}")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.ndim != 1 or offsets.numel() != n + 1 or not offsets.is_contiguous():
        raise SdvHipError(f"{what}: offsets must be a contiguous int64 vector of n + 1 = {n + 1} elements, got "
                          f"{getattr(offsets, 'dtype', type(offsets))} x {getattr(offsets, 'numel', lambda: 0)()}")
    lib = load()
    args = (_ptr(scratch, name="scratch"), scratch.numel(), n, mbh, mbw, _ptr(out, name="out"), out.numel(), _ptr(offsets, name="offsets"))
    _launch("h264_pack", dict(bytes=2.0 * out.numel()), lambda: _check(lib.sdv_h264_pack(*args, _stream()), "sdv_h264_pack"))


_k_h264_pack = _defop("k_h264_pack(Tensor scratch, int n, int mbh, int mbw, Tensor(a!) out, Tensor(b!) offsets) -> ()", _h264_pack_impl)


def h264_pack(scratch: torch.Tensor, n: int, mbh: int, mbw: int, out: torch.Tensor, offsets: torch.Tensor):
    """Compact the slices ``h264_encode_rows`` left in ``scratch`` into ``out`` in sample order (``torch.ops.sdv.k_h264_pack`` ->
    sdv_h264_pack): ``out[offsets[k]:offsets[k + 1]]`` is the mp4 sample of picture k.  ``out`` must hold ``h264_out_bytes``."""
    _k_h264_pack(scratch, int(n), int(mbh), int(mbw), out, offsets)


def _h264_vlc_tables_impl():
    lib = load()
    lengths, codes = (C.c_uint8 * H264_VLC_WORDS)(), (C.c_uint16 * H264_VLC_WORDS)()
    _check(lib.sdv_h264_vlc_tables(lengths, codes, H264_VLC_WORDS), "sdv_h264_vlc_tables")
    return list(zip(lengths, codes))


def h264_vlc_tables():
    """The kernel's VLC tables as 656 ``(length, code)`` pairs in the layout of sdv_hip.h (sdv_h264_vlc_tables; host only, no GPU work)."""
    return _h264_vlc_tables_impl()
