"""Python binding of libH265ToJpeg.so (ctypes over the C ABI in include/h2j.h).

This mirrors the reference's operator surface for the path:
``IDecoder::getInstance()->H265ToJpeg(in, out)`` (/root/reference/export_inc/IDecoder.h:29,35)
is :func:`h265_to_jpeg`; the batch engine underneath it is :class:`Engine`.
There is no CPU fallback: constructing an :class:`Engine` without a HIP
device raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libH265ToJpeg.so"
# the C entry points younger than libH265ToJpeg.so's fixed export list (csrc/host/api_ext.h): a thin library beside it
_EXT_LIB_NAME = "libH265ToJpegExt.so"
_EXT_SYMBOLS = ("h2j_engine_transcode_multi7", "h2j_engine_submit_multi7", "h2j_engine_decode_multi7",
                "h2j_h265_to_jpeg_mem_multi7", "h2j_crop_window7", "h2j_pad_colour",
                # colour (an older build of the library beside an older host library lacks these: it still loads)
                "h2j_engine_transcode_multi8", "h2j_engine_submit_multi8", "h2j_engine_decode_multi8",
                "h2j_h265_to_jpeg_mem_multi8", "h2j_stream_colour", "h2j_colour_coeffs")
_lib = None


class OutOpts(ctypes.Structure):
    """include/h2j.h h2j_out_opts: per-item scaled output."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32)]


class OutOpts2(ctypes.Structure):
    """include/h2j.h h2j_out_opts2: per-item scaled or exact-size output."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class OutOpts3(ctypes.Structure):
    """include/h2j.h h2j_out_opts3: h2j_out_opts2 and a window of the picture (crop and cover)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class OutOpts4(ctypes.Structure):
    """include/h2j.h h2j_out_opts4: h2j_out_opts3 and an orientation (rotate / flip on the GPU)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("orient", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


class OutOpts5(ctypes.Structure):
    """include/h2j.h h2j_out_opts5: h2j_out_opts4 and the finishing options (a fixed JPEG quantiser scale, an
    unsharp mask on the GPU)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("orient", ctypes.c_int32), ("qscale", ctypes.c_int32), ("sharpen", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


class OutOpts6(ctypes.Structure):
    """include/h2j.h h2j_out_opts6: h2j_out_opts5 and the pixel format (the JPEG, or raw RGB made on the GPU)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("orient", ctypes.c_int32), ("qscale", ctypes.c_int32), ("sharpen", ctypes.c_int32),
                ("format", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class OutOpts7(ctypes.Structure):
    """include/h2j.h h2j_out_opts7: h2j_out_opts6 and the padding (letterbox to the box, the fill colour 0x00RRGGBB)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("orient", ctypes.c_int32), ("qscale", ctypes.c_int32), ("sharpen", ctypes.c_int32),
                ("format", ctypes.c_int32), ("pad", ctypes.c_int32), ("background", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 1)]


class OutOpts8(ctypes.Structure):
    """include/h2j.h h2j_out_opts8: h2j_out_opts7 and the colour (the source matrix and range K3v normalises to JFIF's)."""
    _fields_ = [("scale_log2", ctypes.c_int32), ("max_dim", ctypes.c_int32), ("fit_w", ctypes.c_int32),
                ("fit_h", ctypes.c_int32), ("flags", ctypes.c_int32), ("crop_x", ctypes.c_int32),
                ("crop_y", ctypes.c_int32), ("crop_w", ctypes.c_int32), ("crop_h", ctypes.c_int32),
                ("orient", ctypes.c_int32), ("qscale", ctypes.c_int32), ("sharpen", ctypes.c_int32),
                ("format", ctypes.c_int32), ("pad", ctypes.c_int32), ("background", ctypes.c_int32),
                ("colour", ctypes.c_int32)]


COLOUR_AUTO, COLOUR_EXPLICIT = -1, 0x100  # include/h2j.h H2J_COLOUR_*
COLOUR_MATRICES = {"bt709": 1, "bt601": 6, "bt2020": 9}  # the matrix_coefficients value of each name
COLOUR_RANGES = {"limited": 0, "full": 1}
FMT_JPEG, FMT_RGB8, FMT_RGB8_PLANAR = 0, 1, 2  # include/h2j.h H2J_FMT_*
FORMATS = {"jpeg": FMT_JPEG, "rgb": FMT_RGB8, "rgb_planar": FMT_RGB8_PLANAR}  # the spec key "format"
FIT_STRETCH = 1  # include/h2j.h H2J_FIT_STRETCH
FIT_COVER = 2  # include/h2j.h H2J_FIT_COVER
ERR_OUT_OPTS = -60  # include/h2j.h H2J_ERR_OUT_OPTS: status of an item with invalid output options
MAX_RENDITIONS = 8  # include/h2j.h H2J_MAX_RENDITIONS: JPEG outputs of one item of a multi call
ERR_RENDITIONS = -61  # include/h2j.h H2J_ERR_RENDITIONS: a rendition count outside 1..MAX_RENDITIONS
ORIENT_AUTO = -1  # include/h2j.h H2J_ORIENT_AUTO: the orientation the stream's display orientation SEI names
ERR_NO_STAGE = -62  # include/h2j.h H2J_ERR_NO_STAGE: an oriented rendition on a kernel library without the stage


def lib_path() -> str:
    # H2J_LIB_DIR selects an alternative build of the same libraries (e.g. build/prof)
    return os.path.join(os.environ.get("H2J_LIB_DIR", _HERE), _LIB_NAME)


def load_library() -> ctypes.CDLL:
    """Load libH265ToJpeg.so (and, through its RUNPATH, libh2j_hip.so)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run `make -C h264-h265-to-jpeg_amd` or __graft_entry__.build()")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    szp = ctypes.POINTER(ctypes.c_size_t)
    lib.h2j_engine_create.restype = ctypes.c_void_p
    lib.h2j_engine_create.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.h2j_engine_destroy.argtypes = [ctypes.c_void_p]
    lib.h2j_engine_error.restype = ctypes.c_char_p
    lib.h2j_engine_error.argtypes = [ctypes.c_void_p]
    lib.h2j_engine_transcode.restype = ctypes.c_int
    lib.h2j_engine_transcode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, u8p,
                                         ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
    lib.h2j_engine_decode.restype = ctypes.c_int
    lib.h2j_engine_decode.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_uint16), ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.h2j_engine_decode_batch.restype = ctypes.c_int
    lib.h2j_engine_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int)]
    lib.h2j_engine_jpeg_coeffs.restype = ctypes.c_int
    lib.h2j_engine_jpeg_coeffs.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int16),
                                           ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.h2j_engine_submit.restype = ctypes.c_int64
    lib.h2j_engine_submit.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, u8p,
                                      ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
    # scaled output; an older build selected through H2J_LIB_DIR (same-box A/B runs) lacks these
    # symbols and still loads -- a scaled call on it fails with AttributeError
    if hasattr(lib, "h2j_engine_transcode_opts"):
        optp = ctypes.POINTER(OutOpts)
        lib.h2j_engine_transcode_opts.restype = ctypes.c_int
        lib.h2j_engine_transcode_opts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, optp, u8p,
                                                  ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_opts.restype = ctypes.c_int64
        lib.h2j_engine_submit_opts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, optp, u8p,
                                               ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_decode_scaled.restype = ctypes.c_int
        lib.h2j_engine_decode_scaled.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_scaled.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_scaled.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u8p), szp]
    # exact-size output: likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_opts2"):
        opt2p = ctypes.POINTER(OutOpts2)
        lib.h2j_engine_transcode_opts2.restype = ctypes.c_int
        lib.h2j_engine_transcode_opts2.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, opt2p, u8p,
                                                   ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_opts2.restype = ctypes.c_int64
        lib.h2j_engine_submit_opts2.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, opt2p, u8p,
                                                ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_decode_resized.restype = ctypes.c_int
        lib.h2j_engine_decode_resized.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_fit.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_fit.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(u8p), szp]
        lib.h2j_fit_size.restype = ctypes.c_int
        lib.h2j_fit_size.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    # renditions (several JPEGs of one decoded picture): likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_multi"):
        opt2p = ctypes.POINTER(OutOpts2)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt2p, u8p,
                                                   ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_multi.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi.argtypes = lib.h2j_engine_transcode_multi.argtypes
        lib.h2j_engine_decode_multi.restype = ctypes.c_int
        lib.h2j_engine_decode_multi.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt2p, ctypes.c_int,
                                                u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt2p, ctypes.POINTER(u8p), szp,
                                                   ctypes.POINTER(ctypes.c_int)]
    # crop and cover (a window of the picture): likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_multi3"):
        opt3p = ctypes.POINTER(OutOpts3)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi3.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi3.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt3p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_multi3.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi3.argtypes = lib.h2j_engine_transcode_multi3.argtypes
        lib.h2j_engine_decode_multi3.restype = ctypes.c_int
        lib.h2j_engine_decode_multi3.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt3p, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi3.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi3.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt3p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int)]
        lib.h2j_crop_window.restype = ctypes.c_int
        lib.h2j_crop_window.argtypes = [ctypes.c_int, ctypes.c_int, opt3p, i32p, ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_int)]
    # orientation (rotate / flip): likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_multi4"):
        opt4p = ctypes.POINTER(OutOpts4)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi4.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi4.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt4p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_multi4.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi4.argtypes = lib.h2j_engine_transcode_multi4.argtypes
        lib.h2j_engine_decode_multi4.restype = ctypes.c_int
        lib.h2j_engine_decode_multi4.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt4p, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi4.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi4.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt4p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int)]
        lib.h2j_crop_window4.restype = ctypes.c_int
        lib.h2j_crop_window4.argtypes = [ctypes.c_int, ctypes.c_int, opt4p, ctypes.c_int, i32p, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        lib.h2j_stream_orientation.restype = ctypes.c_int
        lib.h2j_stream_orientation.argtypes = [u8p, ctypes.c_size_t]
    # finishing (qscale, sharpen): likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_multi5"):
        opt5p = ctypes.POINTER(OutOpts5)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi5.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi5.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt5p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_engine_submit_multi5.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi5.argtypes = lib.h2j_engine_transcode_multi5.argtypes
        lib.h2j_engine_decode_multi5.restype = ctypes.c_int
        lib.h2j_engine_decode_multi5.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt5p, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi5.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi5.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt5p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int)]
        lib.h2j_crop_window5.restype = ctypes.c_int
        lib.h2j_crop_window5.argtypes = [ctypes.c_int, ctypes.c_int, opt5p, ctypes.c_int, i32p, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    # RGB output (raw renditions): likewise absent from an older build
    if hasattr(lib, "h2j_engine_transcode_multi6"):
        opt6p = ctypes.POINTER(OutOpts6)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi6.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi6.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt6p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_engine_submit_multi6.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi6.argtypes = lib.h2j_engine_transcode_multi6.argtypes
        lib.h2j_h265_to_jpeg_mem_multi6.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi6.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt6p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_crop_window6.restype = ctypes.c_int
        lib.h2j_crop_window6.argtypes = [ctypes.c_int, ctypes.c_int, opt6p, ctypes.c_int, i32p, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    # padded output: its entry points live in libH265ToJpegExt.so, in the directory the host library came from (an
    # older build selected through H2J_LIB_DIR has none: it still loads, and a padded call on it fails with
    # AttributeError); they are bound as attributes of `lib`, so callers find every entry point in one place
    ext_path = os.path.join(os.path.dirname(path), _EXT_LIB_NAME)
    if os.path.exists(ext_path):
        ext = ctypes.CDLL(ext_path, mode=ctypes.RTLD_GLOBAL)
        for sym in _EXT_SYMBOLS:
            if hasattr(ext, sym):
                setattr(lib, sym, getattr(ext, sym))
    if hasattr(lib, "h2j_engine_transcode_multi7"):
        opt7p = ctypes.POINTER(OutOpts7)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi7.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi7.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt7p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_engine_submit_multi7.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi7.argtypes = lib.h2j_engine_transcode_multi7.argtypes
        lib.h2j_engine_decode_multi7.restype = ctypes.c_int
        lib.h2j_engine_decode_multi7.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt7p, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi7.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi7.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt7p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_crop_window7.restype = ctypes.c_int
        lib.h2j_crop_window7.argtypes = [ctypes.c_int, ctypes.c_int, opt7p, ctypes.c_int, i32p, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_pad_colour.restype = ctypes.c_int
        lib.h2j_pad_colour.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)]
    if hasattr(lib, "h2j_engine_transcode_multi8"):  # colour
        opt8p = ctypes.POINTER(OutOpts8)
        i32p = ctypes.POINTER(ctypes.c_int32)
        lib.h2j_engine_transcode_multi8.restype = ctypes.c_int
        lib.h2j_engine_transcode_multi8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(u8p), szp, i32p, opt8p, u8p,
                                                    ctypes.c_size_t, szp, szp, ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_engine_submit_multi8.restype = ctypes.c_int64
        lib.h2j_engine_submit_multi8.argtypes = lib.h2j_engine_transcode_multi8.argtypes
        lib.h2j_engine_decode_multi8.restype = ctypes.c_int
        lib.h2j_engine_decode_multi8.argtypes = [ctypes.c_void_p, u8p, ctypes.c_size_t, ctypes.c_int, opt8p, ctypes.c_int,
                                                 u8p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        lib.h2j_h265_to_jpeg_mem_multi8.restype = ctypes.c_int
        lib.h2j_h265_to_jpeg_mem_multi8.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, opt8p, ctypes.POINTER(u8p), szp,
                                                    ctypes.POINTER(ctypes.c_int), i32p]
        lib.h2j_stream_colour.restype = ctypes.c_int
        lib.h2j_stream_colour.argtypes = [u8p, ctypes.c_size_t, i32p]
        lib.h2j_colour_coeffs.restype = ctypes.c_int
        lib.h2j_colour_coeffs.argtypes = [ctypes.c_int, ctypes.c_int, i32p]
    lib.h2j_free.argtypes = [ctypes.c_void_p]
    lib.h2j_engine_wait.restype = ctypes.c_int
    lib.h2j_engine_wait.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.h2j_engine_stats.restype = ctypes.c_int
    lib.h2j_engine_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.h2j_engine_frame_error.restype = ctypes.c_char_p
    lib.h2j_engine_frame_error.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.h2j_engine_host_info.restype = ctypes.c_int
    lib.h2j_engine_host_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.h2j_device_count.restype = ctypes.c_int
    lib.h2j_engine_chunk_times.restype = ctypes.c_int
    lib.h2j_engine_chunk_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.h2j_version.restype = ctypes.c_char_p
    lib.h2j_gpu_device_count.restype = ctypes.c_int
    _lib = lib
    return lib


def device_count() -> int:
    return int(load_library().h2j_gpu_device_count())


def _u8(buf: bytes):
    arr = (ctypes.c_uint8 * len(buf)).from_buffer_copy(buf)
    return arr


STAT_KEYS = ["parse_ms", "h2d_ms", "recon_ms", "deblock_ms", "sao_ms", "jpeg_ms", "d2h_ms",
             "assemble_ms", "total_ms", "frames", "alg_bytes", "entropy_ms", "prep_ms", "chunks", "pack_ms",
             "parse_run_ms", "d2h_stats_ms", "d2h_payload_ms", "payload_bytes", "host_grow_ms", "h2d_bytes",
             "payload_copied_bytes", "scale_ms", "renditions", "parsed", "raw_bytes"]
# the entries of h2j_engine_stats behind those (a kernel or host library older than them leaves them 0)
STAT_KEYS_LATER = ["pad_bytes"]
STAT_KEYS_COLOUR = ["colour_bytes"]  # ... and behind that one


def _per_item(v, n, name):
    """A scalar or a per-item sequence of n ints (None: 0)."""
    if v is None:
        return [0] * n
    if isinstance(v, (int, np.integer)):
        return [int(v)] * n
    v = [int(x) for x in v]
    if len(v) != n:
        raise ValueError(f"{name}: {len(v)} entries for {n} streams")
    return v


def _is_pair(v):
    """A (w, h) pair of ints (0 or None: no bound on that axis)."""
    return (isinstance(v, (tuple, list)) and len(v) == 2 and
            all(x is None or isinstance(x, (int, np.integer)) for x in v))


def _per_item_fit(fit, n):
    """fit -> n (w, h) int pairs: one pair for every item, or a per-item sequence of pairs or None."""
    if fit is None:
        return [(0, 0)] * n
    if not _is_pair(fit):
        fit = list(fit)
        if len(fit) != n:
            raise ValueError(f"fit: {len(fit)} entries for {n} streams")
        for p in fit:
            if p is not None and not _is_pair(p):
                raise ValueError(f"fit: {p!r} is not a (w, h) pair")
    else:
        fit = [fit] * n
    return [(0, 0) if p is None else (int(p[0] or 0), int(p[1] or 0)) for p in fit]


def _out_opts(scale, max_dim, n, fit=None, stretch=False):
    """ctypes h2j_out_opts[n], h2j_out_opts2[n] when fit or stretch is given, or None (the unscaled
    call) when no keyword is."""
    if fit is None and (stretch is None or stretch is False):
        if scale is None and max_dim is None:
            return None
        sc, md = _per_item(scale, n, "scale"), _per_item(max_dim, n, "max_dim")
        return (OutOpts * n)(*[OutOpts(a, b) for a, b in zip(sc, md)])
    sc, md = _per_item(scale, n, "scale"), _per_item(max_dim, n, "max_dim")
    ft = _per_item_fit(fit, n)
    if isinstance(stretch, (bool, np.bool_)) or stretch is None:
        stf = [bool(stretch)] * n
    else:
        stf = [bool(x) for x in stretch]
        if len(stf) != n:
            raise ValueError(f"stretch: {len(stf)} entries for {n} streams")
    return (OutOpts2 * n)(*[OutOpts2(a, b, w, h, FIT_STRETCH if t else 0)
                            for a, b, (w, h), t in zip(sc, md, ft, stf)])


_SPEC_KEYS = ("scale", "max_dim", "fit", "stretch", "crop", "cover", "orient", "qscale", "sharpen", "format", "pad", "colour")


def _is_colour_source(v):
    """A named source: a (matrix, range) pair of strings, the first a matrix's name (so a per-item sequence of two
    "auto" is not one)."""
    return isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, str) for x in v) and v[0] in COLOUR_MATRICES


def _colour_value(v, what):
    """A colour as h2j_out_opts8 takes it: None or False: 0 (off); "auto": H2J_COLOUR_AUTO, the stream's signalling; a
    (matrix, range) pair -- "bt601" / "bt709" / "bt2020", "limited" / "full" -- the source the caller names:
    H2J_COLOUR_EXPLICIT | matrix_coefficients << 1 | full."""
    if v is None or v is False:
        return 0
    if isinstance(v, str) and v == "auto":
        return COLOUR_AUTO
    if _is_colour_source(v) and v[0] in COLOUR_MATRICES and v[1] in COLOUR_RANGES:
        return COLOUR_EXPLICIT | COLOUR_MATRICES[v[0]] << 1 | COLOUR_RANGES[v[1]]
    raise ValueError(f"{what}: colour {v!r} is not \"auto\" or a (matrix, range) pair of {sorted(COLOUR_MATRICES)} and {sorted(COLOUR_RANGES)}")


def _is_colour(v):
    """An (r, g, b) colour: a tuple or list of three ints (no entry of a per-item or per-batch sequence is an int, so a
    sequence of three ints is never one of those)."""
    return (isinstance(v, (tuple, list)) and len(v) == 3 and
            all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in v))


def _pad_value(v, what):
    """A padding as h2j_out_opts7 takes it, (pad, background): None or False: (0, 0); True: black; (r, g, b), each
    0..255: that colour as 0x00RRGGBB."""
    if v is None or v is False:
        return (0, 0)
    if v is True:
        return (1, 0)
    if _is_colour(v) and all(0 <= x <= 255 for x in v):
        return (1, (int(v[0]) << 16) | (int(v[1]) << 8) | int(v[2]))
    raise ValueError(f"{what}: pad {v!r} is not True or an (r, g, b) colour with each value 0..255")


def _format_value(v, what):
    """A pixel format as h2j_out_opts6 takes it: "jpeg", "rgb" or "rgb_planar" (None: the JPEG)."""
    if v is None:
        return FMT_JPEG
    if isinstance(v, str) and v in FORMATS:
        return FORMATS[v]
    raise ValueError(f'{what}: format {v!r} is not "jpeg", "rgb" or "rgb_planar"')


def _finish_value(v, what, name):
    """qscale / sharpen as h2j_out_opts5 takes them: an int (the engine checks the range); None is 0."""
    if v is None:
        return 0
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        return int(v)
    raise ValueError(f"{what}: {name} {v!r} is not an int")


def _orient_value(v, what):
    """An orientation as h2j_out_opts4 takes it: an int (0..8; the engine checks the range) or "auto"."""
    if isinstance(v, str) and v == "auto":
        return ORIENT_AUTO
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        return int(v)
    raise ValueError(f'{what}: orient {v!r} is not an int (0..8) or "auto"')


def _is_window(v):
    """An (x, y, w, h) window of ints (w, h 0 or None: to the right / bottom edge)."""
    return (isinstance(v, (tuple, list)) and len(v) == 4 and
            all(x is None or (isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))) for x in v))


def rendition_spec(spec):
    """One rendition spec -> (scale_log2, max_dim, fit_w, fit_h, flags), the fields of h2j_out_opts2; with
    a crop or cover key (crop_x, crop_y, crop_w, crop_h) follow: the fields of h2j_out_opts3; with an orient
    key those and orient: the fields of h2j_out_opts4; with a qscale or sharpen key those (orient 0 if the spec
    names none), qscale and sharpen: the fields of h2j_out_opts5; with a format key those (0 where the spec names
    none) and format: the fields of h2j_out_opts6; with a pad key those (0 where the spec names none), pad and
    background: the fields of h2j_out_opts7; with a colour key those (0 where the spec names none) and colour: the
    fields of h2j_out_opts8.

    A spec is an int (scale), a (w, h) pair (fit; 0 or None: no bound on that axis) or a dict with any
    of scale, max_dim, fit, stretch, crop (an (x, y, w, h) window in luma samples of the picture; w, h 0:
    to the edge) and cover (a (w, h) box: the largest centred part of the window with the box's aspect, at
    the box's size) and orient (0..8, the EXIF orientation that makes the picture upright, or "auto": the one
    the stream's display orientation SEI names; crop, cover, scale and fit then act on the oriented
    picture), qscale (2..31: the JPEG quantiser scale instead of the rate control's; 0: the rate control's) and
    sharpen (1..64: an unsharp mask of strength sharpen / 16 on the luma of the rendition's final 8-bit planes;
    0: none) and format ("jpeg": the file, as without the key; "rgb": the rendition's final picture as 8-bit RGB
    pixels, numpy (H, W, 3); "rgb_planar": the same as (3, H, W) -- converted on the GPU, no JPEG loss) and pad (True,
    or an (r, g, b) colour: the rendition letterboxed to the exact size of its box -- a two-sided fit, or a cover -- the
    picture part centred, the rest black or that colour; the rendition then has the box's size whatever the picture's)
    and colour ("auto", or a (matrix, range) pair such as ("bt709", "limited"): the rendition's planes converted on the
    GPU from that source matrix and range -- "auto": what the stream signals -- to JFIF's BT.601 full range, which every
    JPEG and RGB array is read as).
    Values are not range-checked here: the engine fails a rendition
    with invalid options alone (ERR_OUT_OPTS)."""
    if isinstance(spec, (bool, np.bool_)):
        raise ValueError(f"rendition {spec!r}: an int (scale), a (w, h) pair (fit) or a dict")
    if isinstance(spec, (int, np.integer)):
        return (int(spec), 0, 0, 0, 0)
    if _is_pair(spec):
        return (0, 0, int(spec[0] or 0), int(spec[1] or 0), 0)
    if isinstance(spec, dict):
        bad = [k for k in spec if k not in _SPEC_KEYS]
        if bad:
            raise ValueError(f"rendition {spec!r}: unknown key {bad[0]!r} (scale, max_dim, fit, stretch, crop, cover, orient, qscale, sharpen, format, pad, colour)")
        if "colour" in spec:  # the h2j_out_opts8 fields, whatever else the spec names
            rest = dict(spec)
            col = _colour_value(rest.pop("colour"), f"rendition {spec!r}")
            return (tuple(rendition_spec(rest)) + (0,) * 10)[:15] + (col,)
        if "pad" in spec:  # the h2j_out_opts7 fields, whatever else the spec names
            rest = dict(spec)
            pad = _pad_value(rest.pop("pad"), f"rendition {spec!r}")
            return (tuple(rendition_spec(rest)) + (0,) * 8)[:13] + pad
        if "format" in spec:  # the h2j_out_opts6 fields, whatever else the spec names
            rest = dict(spec)
            fmt = _format_value(rest.pop("format"), f"rendition {spec!r}")
            return (tuple(rendition_spec(rest)) + (0,) * 7)[:12] + (fmt,)
        if "qscale" in spec or "sharpen" in spec:  # the h2j_out_opts5 fields, whatever else the spec names
            rest = dict(spec)
            q = _finish_value(rest.pop("qscale", None), f"rendition {spec!r}", "qscale")
            a = _finish_value(rest.pop("sharpen", None), f"rendition {spec!r}", "sharpen")
            return (tuple(rendition_spec(rest)) + (0,) * 5)[:10] + (q, a)
        fit = spec.get("fit")
        if fit is not None and not _is_pair(fit):
            raise ValueError(f"rendition {spec!r}: fit is not a (w, h) pair")
        fw, fh = (0, 0) if fit is None else (int(fit[0] or 0), int(fit[1] or 0))
        old = (int(spec.get("scale") or 0), int(spec.get("max_dim") or 0), fw, fh,
               FIT_STRETCH if spec.get("stretch") else 0)
        crop, cover = spec.get("crop"), spec.get("cover")
        if "orient" in spec:  # the h2j_out_opts4 fields, whatever else the spec names
            rest = dict(spec)
            orient = _orient_value(rest.pop("orient"), f"rendition {spec!r}")
            return (tuple(rendition_spec(rest)) + (0, 0, 0, 0))[:9] + (orient,)
        if crop is None and cover is None:
            return old
        if crop is not None and not _is_window(crop):
            raise ValueError(f"rendition {spec!r}: crop is not an (x, y, w, h) window")
        if cover is not None:
            if not _is_pair(cover):
                raise ValueError(f"rendition {spec!r}: cover is not a (w, h) pair")
            if fit is not None:
                raise ValueError(f"rendition {spec!r}: cover and fit both name a box")
            old = old[:2] + (int(cover[0] or 0), int(cover[1] or 0), old[4] | FIT_COVER)
        return old + ((0, 0, 0, 0) if crop is None else tuple(int(x or 0) for x in crop))
    raise ValueError(f"rendition {spec!r}: an int (scale), a (w, h) pair (fit) or a dict")


def _is_spec(v):
    return (isinstance(v, (int, np.integer, dict)) and not isinstance(v, (bool, np.bool_))) or _is_pair(v)


def normalize_renditions(renditions, n: int):
    """renditions -> n lists of (scale_log2, max_dim, fit_w, fit_h, flags) tuples, one list per item.

    renditions is one list of specs (rendition_spec) used for every item, or a sequence of n such lists,
    one per item.  A list of two ints is one list of two scales, not a fit: write a fit inside a list of
    specs as a tuple, (w, h), or as {"fit": (w, h)}.  Every item has 1..MAX_RENDITIONS renditions."""
    if renditions is None or isinstance(renditions, (int, np.integer, dict, str, bytes)):
        raise ValueError("renditions: a list of specs, or one such list per item")
    renditions = list(renditions)
    # one list for every item: each element is a spec and not itself a list of specs (a tuple pair is a
    # fit; a list is read as a per-item list)
    shared = all(_is_spec(r) and not isinstance(r, list) for r in renditions)
    if shared:
        per_item = [renditions] * n
    else:
        if len(renditions) != n:
            raise ValueError(f"renditions: {len(renditions)} per-item lists for {n} streams")
        for r in renditions:
            if not isinstance(r, (list, tuple)) or _is_spec(r) and not isinstance(r, list):
                raise ValueError(f"renditions: {r!r} is not a list of specs")
        per_item = [list(r) for r in renditions]
    out = []
    for specs in per_item:
        if not 1 <= len(specs) <= MAX_RENDITIONS:
            raise ValueError(f"renditions: {len(specs)} for one item (1..{MAX_RENDITIONS})")
        out.append([rendition_spec(x) for x in specs])
    return out


def _multi_cap(streams, per_item, floor):
    """Output bytes to offer first: per rendition what transcode() offers per item, halved per scale
    level for a plain scale (a JPEG at 1/4 of the samples is well under half the bytes); too little is
    retried (-50)."""
    cap = 0
    for s, specs in zip(streams, per_item):
        full = max(floor, 4 * len(s))
        for spec in specs:
            scale, max_dim, fw, fh = spec[:4]
            plain_scale = 0 <= scale <= 3 and not (max_dim or fw or fh)
            cap += (full >> scale) + 65536 if plain_scale else full
            if len(spec) > 12 and spec[12] and fw > 0 and fh > 0:
                cap += 3 * fw * fh  # raw pixels of a boxed output: never more than the box (any other: the retry sizes it)
    return cap


def _multi_opts(per_item):
    """(nrend int32[n], h2j_out_opts2[sum], total) of normalize_renditions' result; h2j_out_opts3[sum] when
    a rendition names a window or a cover (the multi3 calls take those)."""
    n = len(per_item)
    nrend = (ctypes.c_int32 * n)(*[len(x) for x in per_item])
    flat = [t for x in per_item for t in x]
    if any(len(t) > 15 for t in flat):  # a colour: the multi8 calls
        opts = (OutOpts8 * len(flat))(*[OutOpts8(*(tuple(t) + (0,) * 11)[:16]) for t in flat])
    elif any(len(t) > 13 for t in flat):  # a padding: the multi7 calls
        opts = (OutOpts7 * len(flat))(*[OutOpts7(*(tuple(t) + (0,) * 10)[:15]) for t in flat])
    elif any(len(t) > 12 for t in flat):  # a format: the multi6 calls
        opts = (OutOpts6 * len(flat))(*[OutOpts6(*(tuple(t) + (0,) * 8)[:13]) for t in flat])
    elif any(len(t) > 10 for t in flat):  # a finishing option: the multi5 calls
        opts = (OutOpts5 * len(flat))(*[OutOpts5(*(tuple(t) + (0,) * 7)[:12]) for t in flat])
    elif any(len(t) > 9 for t in flat):  # an orientation: the multi4 calls
        opts = (OutOpts4 * len(flat))(*[OutOpts4(*(tuple(t) + (0,) * 5)[:10]) for t in flat])
    elif any(len(t) > 5 for t in flat):
        opts = (OutOpts3 * len(flat))(*[OutOpts3(*(tuple(t) + (0, 0, 0, 0))[:9]) for t in flat])
    else:
        opts = (OutOpts2 * len(flat))(*[OutOpts2(a, b, w, h, f) for a, b, w, h, f in flat])
    return nrend, opts, len(flat)


def _per_item_shape(v, n, name, ok, what):
    """v (None, one value for every item, or a per-item sequence of values or None) -> n values or None."""
    if v is None:
        return [None] * n
    if ok(v):
        return [tuple(v)] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"{name}: {len(v)} entries for {n} streams")
    for p in v:
        if p is not None and not ok(p):
            raise ValueError(f"{name}: {p!r} is not {what}")
    return [None if p is None else tuple(p) for p in v]


def _per_item_orient(orient, n):
    """orient (None, one value for every item, or a per-item sequence of values or None) -> n values or None."""
    if orient is None:
        return [None] * n
    if isinstance(orient, (str, int, np.integer)):
        return [_orient_value(orient, "orient")] * n
    v = list(orient)
    if len(v) != n:
        raise ValueError(f"orient: {len(v)} entries for {n} streams")
    return [None if x is None else _orient_value(x, "orient") for x in v]


def _per_item_finish(v, n, name):
    """qscale / sharpen (None, one int for every item, or a per-item sequence of ints or None) -> n values or None."""
    if v is None:
        return [None] * n
    if isinstance(v, (int, np.integer)):
        return [_finish_value(v, name, name)] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"{name}: {len(v)} entries for {n} streams")
    return [None if x is None else _finish_value(x, name, name) for x in v]


def _per_item_format(v, n):
    """format (None, one name for every item, or a per-item sequence of names or None) -> n names or None."""
    if v is None or isinstance(v, str):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"format: {len(v)} entries for {n} streams")
    return v


def _per_item_pad(v, n):
    """pad (None, True / False or one (r, g, b) colour for every item, or a per-item sequence of those) -> n values."""
    if v is None or isinstance(v, (bool, np.bool_)) or _is_colour(v):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"pad: {len(v)} entries for {n} streams")
    return v


def _per_item_colour(v, n):
    """colour (None, "auto" or one (matrix, range) pair for every item, or a per-item sequence of those) -> n values."""
    if v is None or v is False or isinstance(v, str) or _is_colour_source(v):
        return [v] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"colour: {len(v)} entries for {n} streams")
    return v


def _window_specs(n, scale, max_dim, fit, stretch, crop, cover, orient=None, qscale=None, sharpen=None, format=None, pad=None, colour=None):
    """Per-item rendition dicts of transcode()'s keywords when crop, cover, orient, qscale, sharpen, format, pad or colour is given."""
    sc, md = _per_item(scale, n, "scale"), _per_item(max_dim, n, "max_dim")
    ft = [None] * n if fit is None else _per_item_fit(fit, n)
    if isinstance(stretch, (bool, np.bool_)) or stretch is None:
        stf = [bool(stretch)] * n
    else:
        stf = [bool(x) for x in stretch]
        if len(stf) != n:
            raise ValueError(f"stretch: {len(stf)} entries for {n} streams")
    cr = _per_item_shape(crop, n, "crop", _is_window, "an (x, y, w, h) window")
    cv = _per_item_shape(cover, n, "cover", _is_pair, "a (w, h) pair")
    orr = _per_item_orient(orient, n)
    qs, sh = _per_item_finish(qscale, n, "qscale"), _per_item_finish(sharpen, n, "sharpen")
    fm = _per_item_format(format, n)
    pd = _per_item_pad(pad, n)
    cl = _per_item_colour(colour, n)
    out = []
    for i in range(n):
        d = {"scale": sc[i], "max_dim": md[i], "stretch": stf[i]}
        if ft[i] is not None and ft[i] != (0, 0):
            d["fit"] = ft[i]
        if cr[i] is not None:
            d["crop"] = cr[i]
        if cv[i] is not None:
            d["cover"] = cv[i]
        if orr[i] is not None:
            d["orient"] = orr[i]
        if qs[i] is not None:
            d["qscale"] = qs[i]
        if sh[i] is not None:
            d["sharpen"] = sh[i]
        if fm[i] is not None:
            d["format"] = fm[i]
        if pd[i] is not None and pd[i] is not False:
            d["pad"] = pd[i]
        if cl[i] is not None and cl[i] is not False:
            d["colour"] = cl[i]
        out.append([d])
    return out


def crop_window(w: int, h: int, crop=None, cover=None, scale: int = 0, max_dim: int = 0, fit=None,
                stretch: bool = False, orient=0, sei_orient: int = 0):
    """((x, y, w, h), (W_o, H_o)): the window and the output size of a cropped w x h picture for these
    options -- include/h2j.h h2j_crop_window, the one place the window and cover rule lives.  ValueError
    where the engine would fail the rendition (ERR_OUT_OPTS).

    orient (0..8 or "auto", which resolves to sei_orient) other than 0: through h2j_crop_window4, for a decoded
    w x h picture; the window and the size are those of the oriented picture and the resolved orientation
    (0 or 2..8) follows them: ((x, y, w, h), (W_o, H_o), orientation)."""
    if not (isinstance(orient, (int, np.integer)) and not isinstance(orient, (bool, np.bool_)) and orient == 0):
        spec = {"scale": scale, "max_dim": max_dim, "stretch": stretch, "crop": (0, 0, 0, 0) if crop is None else crop,
                "orient": orient}
        if fit is not None:
            spec["fit"] = fit
        if cover is not None:
            spec["cover"] = cover
        o = OutOpts4(*rendition_spec(spec))
        win, ow, oh, ro = (ctypes.c_int32 * 4)(), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        rc = load_library().h2j_crop_window4(int(w), int(h), ctypes.byref(o), int(sei_orient), win, ctypes.byref(ow),
                                             ctypes.byref(oh), ctypes.byref(ro))
        if rc != 0:
            raise ValueError(f"h2j_crop_window4({w}, {h}, {spec!r}, {sei_orient}) failed ({rc})")
        return tuple(int(x) for x in win), (ow.value, oh.value), ro.value
    spec = {"scale": scale, "max_dim": max_dim, "stretch": stretch, "crop": (0, 0, 0, 0) if crop is None else crop}
    if fit is not None:
        spec["fit"] = fit
    if cover is not None:
        spec["cover"] = cover
    o = OutOpts3(*rendition_spec(spec))
    win, ow, oh = (ctypes.c_int32 * 4)(), ctypes.c_int(0), ctypes.c_int(0)
    rc = load_library().h2j_crop_window(int(w), int(h), ctypes.byref(o), win, ctypes.byref(ow), ctypes.byref(oh))
    if rc != 0:
        raise ValueError(f"h2j_crop_window({w}, {h}, {spec!r}) failed ({rc})")
    return tuple(int(x) for x in win), (ow.value, oh.value)


def stream_orientation(stream: bytes) -> int:
    """The display orientation (0, 2..8) of picture 0 of an Annex-B stream: what orient="auto" resolves to
    (include/h2j.h h2j_stream_orientation; no entropy decode, no GPU).  ValueError for a stream that is neither
    H.264 nor H.265."""
    r = load_library().h2j_stream_orientation(_u8(stream), len(stream))
    if r < 0:
        raise ValueError(f"h2j_stream_orientation failed ({r}): not an H.264/H.265 Annex-B stream")
    return r


def stream_colour(stream: bytes) -> dict:
    """What a stream signals of its colour, without decoding it (include/h2j_ext.h h2j_stream_colour; no GPU):
    {"primaries", "transfer", "matrix", "full_range"} -- colour_primaries, transfer_characteristics and
    matrix_coefficients as the specs number them, from the SPS's VUI or, in a HEIF file, the nclx colour property, which
    wins; 2, 2, 2 and False where nothing is signalled.  colour="auto" acts on the last two.  ValueError for bytes that
    are no stream."""
    info = (ctypes.c_int32 * 4)()
    r = load_library().h2j_stream_colour(_u8(stream), len(stream), info)
    if r < 0:
        raise ValueError(f"h2j_stream_colour failed ({r}): not an H.264/H.265 Annex-B stream or a HEIF file the library reads")
    return {"primaries": int(info[0]), "transfer": int(info[1]), "matrix": int(info[2]), "full_range": bool(info[3])}


def colour_coeffs(matrix, full) -> tuple:
    """(oy, LY, LB, LR, CB, CR, RB, RR): K3v's constants for a source matrix ("bt601" / "bt709" / "bt2020", or a
    matrix_coefficients value 1, 5, 6, 9) and range (include/h2j_ext.h h2j_colour_coeffs)."""
    k = (ctypes.c_int32 * 8)()
    rc = load_library().h2j_colour_coeffs(int(COLOUR_MATRICES.get(matrix, matrix)), int(bool(full)), k)
    if rc != 0:
        raise ValueError(f"h2j_colour_coeffs({matrix!r}, {full!r}) failed ({rc})")
    return tuple(int(x) for x in k)


def fit_size(w: int, h: int, fit, stretch: bool = False):
    """(W_o, H_o): the output size of a cropped w x h picture for fit=(fit_w, fit_h) (0 or None: no
    bound on that axis) -- include/h2j.h h2j_fit_size, the one place the size rule lives."""
    ow, oh = ctypes.c_int(0), ctypes.c_int(0)
    fw, fh = (0, 0) if fit is None else (int(fit[0] or 0), int(fit[1] or 0))
    rc = load_library().h2j_fit_size(int(w), int(h), fw, fh, FIT_STRETCH if stretch else 0,
                                     ctypes.byref(ow), ctypes.byref(oh))
    if rc != 0:
        raise ValueError(f"h2j_fit_size({w}, {h}, {fw}, {fh}, stretch={bool(stretch)}) failed ({rc})")
    return ow.value, oh.value


class Engine:
    """One process-per-GPU transcoding engine (host entropy threads + HIP pipeline)."""

    def __init__(self, device: int = 0, host_threads: int = 0):
        self._lib = load_library()
        self.last_status: List[int] = []
        self._h = self._lib.h2j_engine_create(int(device), int(host_threads))
        if not self._h:
            raise RuntimeError("h2j_engine_create failed: no usable HIP device for the MI355X pipeline")

    def close(self) -> None:
        if self._h:
            self._lib.h2j_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self) -> str:
        return self._lib.h2j_engine_error(self._h).decode(errors="replace")

    def frame_error(self, i: int) -> str:
        """Message of picture i of the last transcode ('' if it succeeded)."""
        return self._lib.h2j_engine_frame_error(self._h, int(i)).decode(errors="replace")

    def host_info(self) -> dict:
        """Host entropy pool placement (include/h2j.h h2j_engine_host_info)."""
        arr = (ctypes.c_int * 4)()
        self._lib.h2j_engine_host_info(self._h, arr, 4)
        return {"threads": arr[0], "numa_node": arr[1], "pinned_cpus": arr[2], "first_cpu": arr[3]}

    def transcode(self, streams: Sequence[bytes], scale=None, max_dim=None, fit=None,
                  stretch=False, crop=None, cover=None, orient=None, qscale=None, sharpen=None, format=None, pad=None,
                  colour=None) -> List[Optional[bytes]]:
        """Annex-B H.264/H.265 stills -> JPEG bytes (None for items that failed).

        scale (0..3: the JPEG at 1/1, 1/2, 1/4, 1/8 of the decoded size) and max_dim (> 0: the
        smallest scale from `scale` up whose JPEG is at most max_dim wide and high) are scalars
        or per-item sequences (include/h2j.h h2j_out_opts); the same stream may be listed several
        times with different scales.

        fit: exact-size output (h2j_out_opts2), a (w, h) box for every item or a per-item sequence
        of boxes or None; the JPEG is the largest even size inside the box with the aspect kept
        (fit_size), never larger than the picture; 0 / None leaves an axis unbounded.  stretch (a
        bool or a per-item sequence): the box is the output size itself.

        crop: the JPEG of a window of the picture (h2j_out_opts3), an (x, y, w, h) tuple in luma samples for
        every item or a per-item sequence of windows or None; the other options act on the window.  cover: a
        (w, h) box likewise: the largest centred part of the window (or picture) with the box's aspect, at
        the box's size (crop_window has the rule).

        orient: the JPEG of the picture rotated / mirrored on the GPU (h2j_out_opts4): 0..8 (the EXIF
        orientation that makes the picture upright) or "auto" (the stream's display orientation SEI), for every
        item or a per-item sequence of values or None; every other option acts on the oriented picture.

        qscale (2..31: that JPEG quantiser scale instead of the rate control's) and sharpen (1..64: an unsharp
        mask of strength sharpen / 16 on the output's luma, on the GPU) (h2j_out_opts5): an int for every item
        or a per-item sequence of ints or None.

        format ("jpeg", "rgb", "rgb_planar"; h2j_out_opts6): one name for every item or a per-item sequence of names
        or None; the entry of a raw item is a numpy uint8 array, (H, W, 3) or (3, H, W), instead of bytes.

        pad (True: black, or an (r, g, b) tuple; h2j_out_opts7): one value for every item or a per-item sequence of
        values or None; the item is letterboxed to the exact size of its box (a two-sided fit, or a cover), so
        transcode(streams, fit=(224, 224), pad=True, format="rgb_planar") returns arrays of one shape, (3, 224, 224).

        colour ("auto", or a (matrix, range) pair such as ("bt709", "limited"); h2j_out_opts8): one value for every item
        or a per-item sequence of values or None; the item's planes are converted from that source -- "auto": what the
        stream signals (stream_colour) -- to JFIF's BT.601 full range before anything else finishes them."""
        n = len(streams)
        if n == 0:
            return []
        if any(v is not None for v in (crop, cover, orient, qscale, sharpen, format, pad, colour)):  # one rendition per item through the multi3 .. multi8 call
            out = self.transcode_multi(streams, _window_specs(n, scale, max_dim, fit, stretch, crop, cover, orient, qscale, sharpen, format, pad, colour))
            self.last_status = [st[0] for st in self.last_status]
            return [o[0] for o in out]
        opts = _out_opts(scale, max_dim, n, fit, stretch)
        bufs = [_u8(s) for s in streams]
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        # JPEG bytes: usually well under 1 MiB per still; on -50 (output buffer too small) retry larger
        cap = sum(max(1 << 20, 4 * len(s)) for s in streams)
        offs = (ctypes.c_size_t * n)()
        lens = (ctypes.c_size_t * n)()
        status = (ctypes.c_int * n)()
        for _ in range(4):
            out = (ctypes.c_uint8 * cap)()
            if opts is None:
                rc = self._lib.h2j_engine_transcode(self._h, n, ptrs, sizes, out, cap, offs, lens, status)
            elif opts._type_ is OutOpts2:
                rc = self._lib.h2j_engine_transcode_opts2(self._h, n, ptrs, sizes, opts, out, cap, offs, lens, status)
            else:
                rc = self._lib.h2j_engine_transcode_opts(self._h, n, ptrs, sizes, opts, out, cap, offs, lens, status)
            if not any(status[i] == -50 for i in range(n)):
                break
            cap *= 4
        if rc < 0 and rc != -3:
            raise RuntimeError(f"h2j_engine_transcode failed ({rc}): {self.error()}")
        self.last_status = [int(status[i]) for i in range(n)]  # per-item status of this call
        mv = memoryview(out)
        return [bytes(mv[offs[i]:offs[i] + lens[i]]) if status[i] == 0 else None for i in range(n)]

    def transcode_multi(self, streams: Sequence[bytes], renditions, out_cap: int = 0) -> List[List[Optional[bytes]]]:
        """Several JPEGs of every picture from one decode: result[i][r] is rendition r of stream i, the
        bytes transcode() returns for that stream with the same options (None where it failed).

        renditions: one list of specs for every item, or one such list per item (normalize_renditions);
        a spec is an int (scale), a (w, h) tuple (fit) or a dict with any of scale, max_dim, fit,
        stretch, crop, cover, orient, qscale, sharpen, format, pad, colour (rendition_spec).  The entry of a raw rendition (format "rgb" /
        "rgb_planar") is a numpy uint8 array, (H, W, 3) / (3, H, W).  last_status has the result's shape.  out_cap: the
        output buffer size tried first (0: an estimate); renditions that did not fit (-50) make the call retry with a
        larger one -- raw renditions are then sized exactly, from the sizes the first pass reported."""
        n = len(streams)
        per_item = normalize_renditions(renditions, n)
        if n == 0:
            self.last_status = []
            return []
        return self._transcode_specs(streams, per_item, out_cap)

    def _transcode_specs(self, streams, per_item, out_cap=0):
        """transcode_multi with the renditions already normalised (normalize_renditions' result)."""
        n = len(streams)
        nrend, opts, total = _multi_opts(per_item)
        bufs = [_u8(s) for s in streams]
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        cap = int(out_cap) or _multi_cap(streams, per_item, 1 << 20)
        offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
        wh = (ctypes.c_int32 * (2 * total))() if opts._type_ in (OutOpts6, OutOpts7, OutOpts8) else None  # the multi6 / multi7 calls report the sizes
        jpeg_cap = cap
        for _ in range(4):  # on -50 (output buffer too small) retry larger, as transcode()
            out = (ctypes.c_uint8 * cap)()
            call = {OutOpts8: "h2j_engine_transcode_multi8", OutOpts7: "h2j_engine_transcode_multi7", OutOpts6: "h2j_engine_transcode_multi6", OutOpts5: "h2j_engine_transcode_multi5", OutOpts4: "h2j_engine_transcode_multi4", OutOpts3: "h2j_engine_transcode_multi3"}.get(opts._type_, "h2j_engine_transcode_multi")
            call = getattr(self._lib, call)
            rc = call(self._h, n, ptrs, sizes, nrend, opts, out, cap, offs, lens, status, *(() if wh is None else (wh,)))
            small = [i for i in range(total) if status[i] == -50]
            if not small:
                break
            if wh is None:
                cap *= 4
            else:  # raw renditions: exactly what they need; the JPEGs' share grows only if one of them did not fit
                raw = sum(3 * wh[2 * i] * wh[2 * i + 1] for i in range(total) if opts[i].format)
                if raw == 0 or any(not opts[i].format for i in small) or jpeg_cap + raw <= cap:
                    jpeg_cap *= 4
                cap = jpeg_cap + raw
        if rc < 0 and rc != -3:
            raise RuntimeError(f"h2j_engine_transcode_multi failed ({rc}): {self.error()}")
        return self._multi_result(per_item, out, offs, lens, status, wh)

    def _multi_result(self, per_item, out, offs, lens, status, wh=None):
        mv = memoryview(out)

        def entry(o, spec):
            if status[o] != 0:
                return None
            fmt = spec[12] if len(spec) > 12 else FMT_JPEG
            if fmt == FMT_JPEG:
                return bytes(mv[offs[o]:offs[o] + lens[o]])
            w, h = int(wh[2 * o]), int(wh[2 * o + 1])
            px = np.frombuffer(out, dtype=np.uint8, count=int(lens[o]), offset=int(offs[o]))
            return px.reshape((h, w, 3) if fmt == FMT_RGB8 else (3, h, w)).copy()

        res, st, o = [], [], 0
        for specs in per_item:
            res.append([entry(o + r, specs[r]) for r in range(len(specs))])
            st.append([int(status[o + r]) for r in range(len(specs))])
            o += len(specs)
        self.last_status = st
        return res

    def transcode_multi_async(self, batches: Sequence[Sequence[bytes]], renditions) -> List[List[List[Optional[bytes]]]]:
        """transcode_multi for several batches through the asynchronous path, all submitted before the
        first wait; renditions as in transcode_multi, for every batch (per-item lists: one per item of
        each batch, so the batches then have the same length).  A raw rendition's size is the picture's, unknown before
        the parse: the items of raw renditions that did not fit the first buffer are run once more, synchronously, with
        a buffer sized from the sizes the first pass reported."""
        return self._multi_async(batches, [renditions] * len(batches))

    def _multi_async(self, batches, renditions_of):
        """transcode_multi_async with the renditions of each batch."""
        held, tickets, streams_of = [], [], [list(b) for b in batches]
        for streams, renditions in zip(batches, renditions_of):
            n = len(streams)
            per_item = normalize_renditions(renditions, n)
            nrend, opts, total = _multi_opts(per_item)
            bufs = [_u8(s) for s in streams]
            ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
            sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
            cap = _multi_cap(streams, per_item, 2 << 20)
            out = (ctypes.c_uint8 * cap)()
            offs, lens, status = (ctypes.c_size_t * total)(), (ctypes.c_size_t * total)(), (ctypes.c_int * total)()
            wh = (ctypes.c_int32 * (2 * total))() if opts._type_ in (OutOpts6, OutOpts7, OutOpts8) else None
            held.append((bufs, ptrs, sizes, nrend, opts, out, offs, lens, status, per_item, wh))
            call = {OutOpts8: "h2j_engine_submit_multi8", OutOpts7: "h2j_engine_submit_multi7", OutOpts6: "h2j_engine_submit_multi6", OutOpts5: "h2j_engine_submit_multi5", OutOpts4: "h2j_engine_submit_multi4", OutOpts3: "h2j_engine_submit_multi3"}.get(opts._type_, "h2j_engine_submit_multi")
            call = getattr(self._lib, call)
            t = call(self._h, n, ptrs, sizes, nrend, opts, out, cap, offs, lens, status, *(() if wh is None else (wh,)))
            if t <= 0:
                raise RuntimeError(f"h2j_engine_submit_multi failed ({t})")
            tickets.append(t)
        res, sts = [], []
        for t, h in zip(tickets, held):
            rc = self.wait(t)
            if rc < 0 and rc != -3:
                raise RuntimeError(f"h2j_engine_wait failed ({rc}): {self.error()}")
            out = self._multi_result(h[9], h[5], h[6], h[7], h[8], h[10])
            st = self.last_status
            # raw renditions that did not fit the estimate (their size is the picture's, unknown before the parse): their
            # items once more, synchronously, the buffer sized from the sizes this pass reported
            again = [i for i, row in enumerate(st) if -50 in row] if h[10] is not None else []
            if again:
                base = [0]
                for specs in h[9]:
                    base.append(base[-1] + len(specs))
                wh, cap2 = h[10], 0
                for i in again:
                    for r, spec in enumerate(h[9][i]):
                        o = base[i] + r
                        raw_px = 3 * wh[2 * o] * wh[2 * o + 1] if len(spec) > 12 and spec[12] else 0
                        cap2 += raw_px or max(8 << 20, 16 * len(streams_of[len(res)][i]))
                redo = self._transcode_specs([streams_of[len(res)][i] for i in again], [h[9][i] for i in again], cap2)
                for i, row, row_st in zip(again, redo, self.last_status):
                    out[i], st[i] = row, row_st
            res.append(out)
            sts.append(st)
        self.last_status = sts
        return res

    def decode_multi(self, stream: bytes, renditions, pick: int):
        """(Y, U, V uint8 numpy, (W_o, H_o), mode): the 8-bit planes the JPEG stage reads for rendition
        `pick` of this picture with all of `renditions` (a list of specs) in flight; mode 0 unscaled,
        1..3 K3s at that scale, 4 K3r, 5 a level K3p wrote (include/h2j.h h2j_engine_decode_multi).
        Renditions with a crop or cover key go through decode_multi3, with an orient key through decode_multi4,
        with a qscale or sharpen key through decode_multi5, with a pad key through decode_multi7."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        if any(len(t) > 15 for t in specs):
            return self.decode_multi8(stream, renditions, pick)[:5]
        if any(len(t) > 13 for t in specs):
            return self.decode_multi7(stream, renditions, pick)[:5]
        if any(len(t) > 10 for t in specs):
            return self.decode_multi5(stream, renditions, pick)[:5]
        if any(len(t) > 9 for t in specs):
            return self.decode_multi4(stream, renditions, pick)[:5]
        if any(len(t) > 5 for t in specs):
            return self.decode_multi3(stream, renditions, pick)[:5]
        _, opts, total = _multi_opts([specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 4)()
        rc = self._lib.h2j_engine_decode_multi(self._h, buf, len(stream), total, opts, int(pick),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return y, u, v, (int(info[0]), int(info[1])), int(info[2])

    def decode_multi3(self, stream: bytes, renditions, pick: int):
        """decode_multi through h2j_engine_decode_multi3 (crop and cover), with the rendition's resolved
        window: (Y, U, V, (W_o, H_o), mode, (x, y, w, h)).  Mode 5: the window has two or more K3s levels
        among the renditions."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        total = len(specs)
        opts = (OutOpts3 * total)(*[OutOpts3(*(tuple(t) + (0, 0, 0, 0))[:9]) for t in specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 8)()
        rc = self._lib.h2j_engine_decode_multi3(self._h, buf, len(stream), total, opts, int(pick),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi3 failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return y, u, v, (int(info[0]), int(info[1])), int(info[2]), tuple(int(info[i]) for i in range(4, 8))

    def decode_multi4(self, stream: bytes, renditions, pick: int):
        """decode_multi through h2j_engine_decode_multi4 (orientation): (Y, U, V, (W_o, H_o), mode, (x, y, w, h),
        orientation, sei_orientation) -- the window in the oriented picture, the rendition's resolved
        orientation (0 or 2..8) and the one the stream's display orientation SEI names.  At mode 0 the planes
        of an oriented rendition are the oriented planes K3o wrote."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        total = len(specs)
        opts = (OutOpts4 * total)(*[OutOpts4(*(tuple(t) + (0,) * 5)[:10]) for t in specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 10)()
        rc = self._lib.h2j_engine_decode_multi4(self._h, buf, len(stream), total, opts, int(pick),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi4 failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return (y, u, v, (int(info[0]), int(info[1])), int(info[2]), tuple(int(info[i]) for i in range(4, 8)),
                int(info[8]), int(info[9]))

    def decode_multi5(self, stream: bytes, renditions, pick: int):
        """decode_multi through h2j_engine_decode_multi5 (finishing): decode_multi4's result, then the quantiser
        scale K4 used for the rendition (the forced one, or the rate control's) and its sharpen.  The planes are
        what K4 reads: those of a sharpened rendition are the sharpened planes K3u wrote."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        total = len(specs)
        opts = (OutOpts5 * total)(*[OutOpts5(*(tuple(t) + (0,) * 7)[:12]) for t in specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 12)()
        rc = self._lib.h2j_engine_decode_multi5(self._h, buf, len(stream), total, opts, int(pick),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi5 failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return (y, u, v, (int(info[0]), int(info[1])), int(info[2]), tuple(int(info[i]) for i in range(4, 8)),
                int(info[8]), int(info[9]), int(info[10]), int(info[11]))

    def decode_multi7(self, stream: bytes, renditions, pick: int):
        """decode_multi through h2j_engine_decode_multi7 (padded output): decode_multi5's result -- the size is the
        output's (the canvas of a padded rendition), the mode that of its picture part -- then whether the rendition was
        padded (0: pad off, or nothing to pad), the place (px, py, w, h) of the picture part and the fill bytes
        (Y, Cb, Cr).  The planes are what K4 reads: those of a padded rendition are the padded planes K3b wrote."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        total = len(specs)
        opts = (OutOpts7 * total)(*[OutOpts7(*(tuple(t) + (0,) * 10)[:15]) for t in specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 18)()
        rc = self._lib.h2j_engine_decode_multi7(self._h, buf, len(stream), total, opts, int(pick),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi7 failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return (y, u, v, (int(info[0]), int(info[1])), int(info[2]), tuple(int(info[i]) for i in range(4, 8)),
                int(info[8]), int(info[9]), int(info[10]), int(info[11]), int(info[12]),
                tuple(int(info[i]) for i in range(13, 17)), (info[17] & 255, (info[17] >> 8) & 255, (info[17] >> 16) & 255))

    def decode_multi8(self, stream: bytes, renditions, pick: int):
        """decode_multi through h2j_engine_decode_multi8 (colour): decode_multi7's result, then the resolved source
        matrix (matrix_coefficients 1, 6 or 9; 0 with colour off), the resolved range (1 full, 0 limited) and whether the
        rendition was converted (0: colour off, or BT.601 full range).  The planes are what K4 reads."""
        specs = normalize_renditions([list(renditions)], 1)[0]
        total = len(specs)
        opts = (OutOpts8 * total)(*[OutOpts8(*(tuple(t) + (0,) * 11)[:16]) for t in specs])
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 21)()
        rc = self._lib.h2j_engine_decode_multi8(self._h, buf, len(stream), total, opts, int(pick),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_multi8 failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return (y, u, v, (int(info[0]), int(info[1])), int(info[2]), tuple(int(info[i]) for i in range(4, 8)),
                int(info[8]), int(info[9]), int(info[10]), int(info[11]), int(info[12]),
                tuple(int(info[i]) for i in range(13, 17)), (info[17] & 255, (info[17] >> 8) & 255, (info[17] >> 16) & 255),
                int(info[18]), int(info[19]), int(info[20]))

    def transcode_raw(self, ptrs, sizes, n, out, cap, offs, lens, status) -> int:
        """Zero-copy variant for benchmarks (pre-built ctypes arrays)."""
        return self._lib.h2j_engine_transcode(self._h, n, ptrs, sizes, out, cap, offs, lens, status)

    def submit_raw(self, ptrs, sizes, n, out, cap, offs, lens, status, opts=None) -> int:
        """Asynchronous batch (h2j_engine_submit): returns a ticket; the ctypes arrays must stay
        alive until wait(ticket).  opts: h2j_out_opts[n] (h2j_engine_submit_opts), h2j_out_opts2[n]
        (h2j_engine_submit_opts2) or None."""
        if opts is None:
            t = self._lib.h2j_engine_submit(self._h, n, ptrs, sizes, out, cap, offs, lens, status)
        elif opts._type_ is OutOpts2:
            t = self._lib.h2j_engine_submit_opts2(self._h, n, ptrs, sizes, opts, out, cap, offs, lens, status)
        else:
            t = self._lib.h2j_engine_submit_opts(self._h, n, ptrs, sizes, opts, out, cap, offs, lens, status)
        if t <= 0:
            raise RuntimeError(f"h2j_engine_submit failed ({t})")
        return t

    def wait(self, ticket: int) -> int:
        return self._lib.h2j_engine_wait(self._h, int(ticket))

    def transcode_async(self, batches: Sequence[Sequence[bytes]], scale=None, max_dim=None, fit=None,
                        stretch=False, crop=None, cover=None, orient=None, qscale=None, sharpen=None, format=None, pad=None) -> List[List[Optional[bytes]]]:
        """Several batches through the asynchronous path, all submitted before the first wait.

        scale / max_dim as in transcode(): a scalar for every picture, or one entry per batch
        (each a scalar or a per-item sequence).  fit / stretch likewise: one (w, h) pair / bool for
        every picture, or one entry per batch (each what transcode() takes).  crop / cover likewise: one
        window / box for every picture, or one entry per batch; orient likewise: one value (0..8 or "auto")
        for every picture, or one entry per batch; qscale and sharpen likewise: one int for every picture, or one
        entry per batch; format likewise: one name for every picture, or one entry per batch; pad likewise: True or one
        (r, g, b) colour for every picture, or one entry per batch."""
        if any(v is not None for v in (crop, cover, orient, qscale, sharpen, format, pad)):
            one_pad = isinstance(pad, (bool, np.bool_)) or _is_colour(pad)
            one_orient = isinstance(orient, (str, int, np.integer))
            one_int = lambda v: isinstance(v, (int, np.integer))
            for name, v, one in (("crop", crop, _is_window(crop)), ("cover", cover, _is_pair(cover)), ("orient", orient, one_orient),
                                 ("qscale", qscale, one_int(qscale)), ("sharpen", sharpen, one_int(sharpen)),
                                 ("format", format, isinstance(format, str)), ("pad", pad, one_pad)):
                if v is not None and not one and len(v) != len(batches):
                    raise ValueError(f"{name}: {len(v)} entries for {len(batches)} batches (one entry per batch)")
            pick = lambda v, one, bi: v if v is None or one else v[bi]
            rends = [_window_specs(len(streams),
                                   pick(scale, isinstance(scale, (int, np.integer)), bi),
                                   pick(max_dim, isinstance(max_dim, (int, np.integer)), bi),
                                   pick(fit, _is_pair(fit), bi), pick(stretch, isinstance(stretch, (bool, np.bool_)), bi),
                                   pick(crop, _is_window(crop), bi), pick(cover, _is_pair(cover), bi),
                                   pick(orient, one_orient, bi), pick(qscale, one_int(qscale), bi),
                                   pick(sharpen, one_int(sharpen), bi), pick(format, isinstance(format, str), bi), pick(pad, one_pad, bi))
                     for bi, streams in enumerate(batches)]
            res = self._multi_async(batches, rends)
            self.last_status = [[st[0] for st in b] for b in self.last_status]
            return [[o[0] for o in b] for b in res]
        for name, v, one in (("fit", fit, _is_pair(fit)), ("stretch", stretch, isinstance(stretch, (bool, np.bool_)))):
            if v is not None and not one and len(v) != len(batches):
                raise ValueError(f"{name}: {len(v)} entries for {len(batches)} batches (one entry per batch)")
        for name, v in (("scale", scale), ("max_dim", max_dim)):
            if v is not None and not isinstance(v, (int, np.integer)) and len(v) != len(batches):
                raise ValueError(f"{name}: {len(v)} entries for {len(batches)} batches (one entry per batch)")
        held, tickets = [], []
        for bi, streams in enumerate(batches):
            n = len(streams)
            bsc = scale if scale is None or isinstance(scale, (int, np.integer)) else scale[bi]
            bmd = max_dim if max_dim is None or isinstance(max_dim, (int, np.integer)) else max_dim[bi]
            bft = fit if fit is None or _is_pair(fit) else fit[bi]
            bst = stretch if stretch is None or isinstance(stretch, (bool, np.bool_)) else stretch[bi]
            opts = _out_opts(bsc, bmd, n, bft, bst)
            bufs = [_u8(s) for s in streams]
            ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
            sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
            cap = sum(max(2 << 20, 4 * len(s)) for s in streams)
            out = (ctypes.c_uint8 * cap)()
            offs, lens, status = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
            held.append((bufs, ptrs, sizes, out, offs, lens, status, n))
            tickets.append(self.submit_raw(ptrs, sizes, n, out, cap, offs, lens, status, opts))
        res = []
        for t, (bufs, ptrs, sizes, out, offs, lens, status, n) in zip(tickets, held):
            rc = self.wait(t)
            if rc < 0 and rc != -3:
                raise RuntimeError(f"h2j_engine_wait failed ({rc}): {self.error()}")
            mv = memoryview(out)
            res.append([bytes(mv[offs[i]:offs[i] + lens[i]]) if status[i] == 0 else None for i in range(n)])
        return res

    def decode(self, stream: bytes, stage: int = 0):
        """Decoded picture planes (uint16 numpy Y, U, V) of the first picture.

        stage 0: final, 1: before loop filters, 2: after deblocking (before SAO).
        """
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint16)
        info = (ctypes.c_int * 3)()
        rc = self._lib.h2j_engine_decode(self._h, buf, len(stream), int(stage),
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode failed ({rc}): {self.error()}")
        return self._planes(out, info)

    def decode_batch(self, streams: Sequence[bytes], pick: int, stage: int = 0):
        """Planes of picture `pick` of `streams` reconstructed as one GPU batch (the launch shapes
        of a production chunk of that many pictures)."""
        n = len(streams)
        bufs = [_u8(s) for s in streams]
        ptrs = (ctypes.POINTER(ctypes.c_uint8) * n)(*[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b in bufs])
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint16)
        info = (ctypes.c_int * 3)()
        rc = self._lib.h2j_engine_decode_batch(self._h, n, ptrs, sizes, int(stage), int(pick),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_batch failed ({rc}): {self.error()}")
        return self._planes(out, info)

    def decode_resized(self, stream: bytes, fit, stretch: bool = False):
        """(Y, U, V uint8 numpy, (W_o, H_o)): the 8-bit planes the JPEG stage reads for this picture
        at the size fit / stretch give (include/h2j.h h2j_engine_decode_resized)."""
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 4)()
        fw, fh = (0, 0) if fit is None else (int(fit[0] or 0), int(fit[1] or 0))
        rc = self._lib.h2j_engine_decode_resized(self._h, buf, len(stream), fw, fh, FIT_STRETCH if stretch else 0,
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_resized failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return y, u, v, (int(info[0]), int(info[1]))

    def decode_scaled(self, stream: bytes, scale: int = 0, max_dim: int = 0):
        """(Y, U, V uint8 numpy, k): the 8-bit planes the JPEG stage reads for this picture at the
        resolved scale k (include/h2j.h h2j_engine_decode_scaled)."""
        buf = _u8(stream)
        cap = 8192 * 8192 * 3 // 2
        out = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_int * 4)()
        rc = self._lib.h2j_engine_decode_scaled(self._h, buf, len(stream), int(scale), int(max_dim),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_decode_scaled failed ({rc}): {self.error()}")
        y, u, v, _ = self._planes(out, info)
        return y, u, v, info[2]

    @staticmethod
    def _planes(out, info):
        w, h, bd = info[0], info[1], info[2]
        ys = w * h
        cs = (w // 2) * (h // 2)
        y = out[:ys].reshape(h, w).copy()
        u = out[ys:ys + cs].reshape(h // 2, w // 2).copy()
        v = out[ys + cs:ys + 2 * cs].reshape(h // 2, w // 2).copy()
        return y, u, v, bd

    def jpeg_coeffs(self, stream: bytes):
        """(qscale, int16 array [nmcu, 6, 64]) computed by the GPU JPEG stage."""
        buf = _u8(stream)
        cap = (8192 // 16) * (8192 // 16) * 384
        out = np.zeros(cap, dtype=np.int16)
        info = (ctypes.c_int * 4)()
        rc = self._lib.h2j_engine_jpeg_coeffs(self._h, buf, len(stream),
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), cap, info)
        if rc < 0:
            raise RuntimeError(f"h2j_engine_jpeg_coeffs failed ({rc}): {self.error()}")
        nmcu = info[3]
        return info[2], out[:nmcu * 384].reshape(nmcu, 6, 64).copy()

    def chunk_times(self) -> list:
        """[(pictures, K1 ms, K0..K5 ms)] per chunk of the last transcode."""
        cap = 4096
        arr = (ctypes.c_double * (3 * cap))()
        n = self._lib.h2j_engine_chunk_times(self._h, arr, cap)
        return [(int(arr[3 * i]), arr[3 * i + 1], arr[3 * i + 2]) for i in range(min(n, cap))]

    def stats(self) -> dict:
        keys = STAT_KEYS + STAT_KEYS_LATER + STAT_KEYS_COLOUR
        arr = (ctypes.c_double * len(keys))()
        self._lib.h2j_engine_stats(self._h, arr, len(keys))
        return {k: arr[i] for i, k in enumerate(keys)}


def h265_to_jpeg(input_path: str, output_path: str) -> bool:
    """Python mirror of IDecoder::getInstance()->H265ToJpeg(in, out)."""
    if not input_path or not output_path:
        return False
    try:
        with open(input_path, "rb") as f:
            data = f.read()
    except OSError:
        return False
    eng = _shared_engine()
    out = eng.transcode([data])[0]
    if out is None:
        return False
    try:
        with open(output_path, "wb+") as f:
            f.write(out)
    except OSError:
        return False
    return True


_ENGINE: Optional[Engine] = None


def _shared_engine() -> Engine:
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = Engine()
    return _ENGINE
