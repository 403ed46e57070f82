"""ctypes loader for libsicn.so (the HIP implementation behind include/sicn.h).

There is no CPU fallback: if the shared library is missing or does not export a symbol of
include/sicn.h this module raises, loudly, at import of the first entry point that needs it."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

from .config import CLayerDesc

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("SICN_LIB", _PKG / "libsicn.so"))

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


class COptions(ctypes.Structure):
    """ctypes image of `sicn_options` (include/sicn.h): kernel-selection knobs, passed by value per call / per net."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "force_generic", "mfma_shape", "tile_x", "strip_chunks",
                                              "no_phase_layout", "split_n", "wave_tile", "prefetch", "persistent_grid", "split_k", "l7_loader", "l0_form", "gdn_fuse")] + [("reserved", ctypes.c_int32 * 2)]


def make_options(**kw) -> "COptions":
    """Library defaults (sicn_options_init) with the given fields replaced, e.g. make_options(tile_x=16)."""
    o = COptions()
    lib().sicn_options_init(ctypes.byref(o))
    for k, v in kw.items():
        if k not in dict(COptions._fields_) or k in ("struct_bytes", "reserved"):
            raise AttributeError(f"sicn_options has no field {k}")
        setattr(o, k, int(v))
    return o


# every symbol include/sicn.h declares: (restype, argtypes)
_descp = ctypes.POINTER(CLayerDesc)
ABI = {
    "sicn_version": (_i, []),
    "sicn_has_alt_kernels": (_i, []),
    "sicn_strerror": (ctypes.c_char_p, [_i]),
    "sicn_validate_desc": (_i, [_descp]),
    "sicn_weights_from_finn_tiles": (_i, [_descp, _vp, _i, _vp, ctypes.POINTER(_vp)]),
    "sicn_weights_free": (None, [_vp]),
    "sicn_conv2d": (_i, [_descp, _vp, _vp, _vp, _i, _vp]),
    "sicn_deconv522": (_i, [_descp, _vp, _vp, _vp, _i, _vp]),
    "sicn_kernel_for": (ctypes.c_char_p, [_descp]),
    "sicn_options_init": (None, [ctypes.POINTER(COptions)]),
    "sicn_conv2d_opt": (_i, [_descp, _vp, _vp, _vp, _i, ctypes.POINTER(COptions), _vp]),
    "sicn_deconv522_opt": (_i, [_descp, _vp, _vp, _vp, _i, ctypes.POINTER(COptions), _vp]),
    "sicn_net_create_opt": (_i, [_descp, ctypes.POINTER(_vp), _i, ctypes.POINTER(COptions), ctypes.POINTER(_vp)]),
    "sicn_net_create": (_i, [_descp, ctypes.POINTER(_vp), _i, ctypes.POINTER(_vp)]),
    "sicn_net_free": (None, [_vp]),
    "sicn_net_workspace_bytes": (_sz, [_vp, _i]),
    "sicn_net_forward": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "sicn_eight_layers_net": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "sicn_net_profile": (_i, [_vp, _i]),
    "sicn_net_layer_ms": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_i)]),
    "sicn_crop_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sicn_debug_plan": (_i, [_descp, _i, ctypes.POINTER(COptions), _i, ctypes.POINTER(ctypes.c_int32)]),
    "sicn_debug_xcd_item": (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_longlong, _i]),
    "sicn_debug_chip": (_i, [ctypes.POINTER(ctypes.c_int32)]),
    "sicn_debug_net_columns": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "sicn_debug_net_input_halves": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32)]),
    "sicn_debug_net_groups": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "sicn_debug_net_walk_groups": (_i, [_vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32)]),
}


class CodecInfo(ctypes.Structure):
    """ctypes image of `sicn_codec_info` (include/sicn_codec.h)."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("mode", "image_width", "image_height", "lat_w", "lat_h", "lat_c",
                                               "n_symbols", "n_streams", "payload_bytes", "adler32", "stream_symbols")]


class CConvLayerDesc(ctypes.Structure):
    """ctypes image of `sicn_convlayer_desc` (include/sicn_convlayer.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("K", "IFM_CH", "IFM_DIM", "OFM_CH", "OFM_DIM", "SIMD", "PE", "IN_BIT", "IN_SIGNED",
                                              "W_BIT", "W_TILES", "ACC_BIT", "ACC_SIGNED", "OUT_BIT", "activation", "NUM_TH",
                                              "ACT_VAL")]


_cldp = ctypes.POINTER(CConvLayerDesc)
# include/sicn_convlayer.h (the generic ConvLayer_Batch surface of convlayer.h:89-125)
CONVLAYER_ABI = {
    "sicn_convlayer_validate": (_i, [_cldp]),
    "sicn_convlayer_params_create": (_i, [_cldp, _vp, _i, _vp, ctypes.POINTER(_vp)]),
    "sicn_convlayer_params_free": (None, [_vp]),
    "sicn_conv_layer_batch": (_i, [_cldp, _vp, _vp, _vp, _i, _vp]),
    "sicn_conv_layer_batch_kernel": (_i, [_cldp, _vp, _vp, _vp, _i, _i, _vp]),
    "sicn_convlayer_kernel_for": (ctypes.c_char_p, [_cldp]),
}

# include/sicn_gdn.h (extension beyond the reference: fixed-point GDN / IGDN in place of the ReLU)
GDN_ABI = {
    "sicn_gdn_create": (_i, [_i, _i, _i, _vp, _vp, ctypes.POINTER(_vp)]),
    "sicn_gdn_free": (None, [_vp]),
    "sicn_gdn_apply": (_i, [_vp, _vp, ctypes.c_longlong, _vp]),
    "sicn_conv2d_gdn": (_i, [_descp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(COptions), _vp]),
    "sicn_deconv522_gdn": (_i, [_descp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(COptions), _vp]),
    "sicn_net_create_gdn": (_i, [_descp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, ctypes.POINTER(COptions), ctypes.POINTER(_vp)]),
    "sicn_gdn_selftest_roots": (ctypes.c_longlong, [_i, ctypes.c_uint32, ctypes.c_ulonglong]),
    "sicn_gdn_spec_version": (_i, []),
}

_u32 = ctypes.c_uint32
# include/sicn_codec.h (extension beyond the reference: latent container + rANS coder)
CODEC_ABI = {
    "sicn_codec_max_bytes": (_sz, [_i, _u32]),
    "sicn_codec_workspace_bytes": (_sz, [_i, _u32]),
    "sicn_codec_encode": (_i, [_i, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _sz, ctypes.POINTER(_sz), _vp, _sz, _vp]),
    "sicn_codec_parse_header": (_i, [_vp, _sz, ctypes.POINTER(CodecInfo)]),
    "sicn_codec_decode": (_i, [_vp, _sz, _vp, _sz, ctypes.POINTER(CodecInfo), _vp, _sz, _vp]),
    "sicn_codec_batch_workspace_bytes": (_sz, [_i, _u32, _u32]),
    "sicn_codec_encode_batch": (_i, [_i, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, ctypes.POINTER(_sz), _vp, _sz, _vp]),
    "sicn_codec_decode_batch": (_i, [_vp, _sz, ctypes.POINTER(_sz), _u32, _vp, _sz, ctypes.POINTER(CodecInfo), _vp, _sz, _vp]),
    "sicn_codec_encode_batch_async": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "sicn_codec_decode_batch_async": (_i, [_vp, _sz, _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "sicn_codec_max_bytes_sl": (_sz, [_u32, _u32]),
    "sicn_codec_workspace_bytes_sl": (_sz, [_u32, _u32]),
    "sicn_codec_batch_workspace_bytes_sl": (_sz, [_u32, _u32, _u32]),
    "sicn_codec_encode_batch_async_sl": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp, _u32]),
    "sicn_codec_decode_batch_async_sl": (_i, [_vp, _sz, _vp, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp, _u32]),
    "sicn_codec_ctx_max_bytes": (_sz, [_u32, _u32, _u32]),
    "sicn_codec_ctx_workspace_bytes": (_sz, [_u32, _u32, _u32, _u32]),
    "sicn_codec_ctx_encode_batch_async": (_i, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "sicn_codec_ctx_decode_batch_async": (_i, [_vp, _sz, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _sz, _vp]),
    "sicn_codec_selftest_div": (ctypes.c_longlong, [_u32, _u32, ctypes.POINTER(ctypes.c_ulonglong)]),
}

_i32p, _i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
# include/sicn_ragged.h (ragged batches: images of different sizes through one launch per layer)
RAGGED_ABI = {
    "sicn_ragged_layout": (_i, [_descp, _i, _i32p, _i32p, _i, _i, _i, _i64p]),
    "sicn_ragged_net_create": (_i, [_descp, ctypes.POINTER(_vp), _i, _i32p, _i32p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_net_free": (None, [_vp]),
    "sicn_ragged_net_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_net_forward": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
}
# include/sicn_ragged_hyper.h (library 0.8: GDN / IGDN layers in a ragged net, and the crop of every image of a ragged tensor in one launch)
RAGGED_HYPER_ABI = {
    "sicn_ragged_net_create_gdn": (_i, [_descp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _i32p, _i32p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_crop_layout": (_i, [_i32p, _i32p, _i32p, _i32p, _i, _i, _i, _i64p]),
    "sicn_ragged_crop_create": (_i, [_i32p, _i32p, _i32p, _i32p, _i, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_crop_free": (None, [_vp]),
    "sicn_ragged_crop_run": (_i, [_vp, _vp, _vp, _vp]),
}
RAGGED_CROP_ROWS = 8      # SICN_RAGGED_CROP_ROWS: destination rows of one work item of the crop



class RaggedCodecImage(ctypes.Structure):
    """ctypes image of `sicn_ragged_codec_image` (include/sicn_ragged_codec.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("latent_offset", "slot_offset", "workspace_offset")] + \
               [(n, ctypes.c_uint32) for n in ("slot_bytes", "n_symbols", "n_streams", "stream_symbols")]


_u32p, _u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
# include/sicn_ragged_codec.h (the rANS-W coder over latents of different shapes: 3 + 2 launches for the whole batch)
RAGGED_CODEC_ABI = {
    "sicn_ragged_codec_layout": (_i, [_u32p, _u32p, _u32, _u32p, _i, ctypes.POINTER(RaggedCodecImage), _u64p]),
    "sicn_ragged_coder_create": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_coder_free": (None, [_vp]),
    "sicn_ragged_coder_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_coder_encode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_coder_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


class RaggedCtxImage(ctypes.Structure):
    """ctypes image of `sicn_ragged_ctx_image` (include/sicn_ragged_ctx.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("latent_offset", "slot_offset", "workspace_offset", "slot_bytes")] + \
               [(n, ctypes.c_uint32) for n in ("n_symbols", "anchor_streams", "nonanchor_streams")]


# include/sicn_ragged_ctx.h (library 0.9: the rANS-WC coder over latents of different shapes, 6 + 8 launches for the whole batch)
RAGGED_CTX_ABI = {
    "sicn_ragged_ctx_layout": (_i, [_u32p, _u32p, _u32, _i, ctypes.POINTER(RaggedCtxImage), _u64p]),
    "sicn_ragged_ctx_coder_create": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_ctx_coder_free": (None, [_vp]),
    "sicn_ragged_ctx_coder_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_ctx_encode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_ctx_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


class RaggedArchiveInfo(ctypes.Structure):
    """ctypes image of `sicn_ragged_archive_info` (include/sicn_ragged_archive.h)."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("version", "n_sections", "n_images", "tag")] + \
               [(n, ctypes.c_uint64) for n in ("total_bytes", "payload_offset")]


class RaggedArchiveStatus(ctypes.Structure):
    """ctypes image of `sicn_ragged_archive_status` (include/sicn_ragged_archive.h); lives in device memory, 16 bytes."""
    _fields_ = [("error", ctypes.c_uint32), ("first_bad", ctypes.c_uint32), ("bytes", ctypes.c_uint64)]


_u64pp = ctypes.POINTER(_u64p)
_vpp = ctypes.POINTER(_vp)
# include/sicn_ragged_archive.h (library 0.10: the containers of a ragged batch as one byte string, 2 + 2 launches)
RAGGED_ARCHIVE_ABI = {
    "sicn_ragged_archive_layout": (_i, [_u32p, _u32, _u32, _u64p, _u64p]),
    "sicn_ragged_archive_parse": (_i, [_vp, _sz, ctypes.POINTER(RaggedArchiveInfo), _u32p, _u64p]),
    "sicn_ragged_archive_chunk_bytes": (_sz, []),
    "sicn_ragged_archive_create": (_i, [_i, _i, _u64pp, _u64pp, ctypes.POINTER(_vp)]),
    "sicn_ragged_archive_free": (None, [_vp]),
    "sicn_ragged_archive_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_archive_max_bytes": (_sz, [_vp]),
    "sicn_ragged_archive_pack_async": (_i, [_vp, _vpp, _vpp, _u32, _vp, _sz, _vp, _vp, _sz, _vp]),
    "sicn_ragged_archive_unpack_async": (_i, [_vp, _vp, _sz, _u32, _vpp, _vpp, _vp, _vp, _sz, _vp]),
}

# include/sicn_ragged_archive_select.h (library 0.11: a selection of an archive's images unpacked with 2 launches; the selection's own archive on the host)
RAGGED_ARCHIVE_SELECT_ABI = {
    "sicn_ragged_archive_unpack_select_async": (_i, [_vp, _vp, _sz, _u32, _vp, _vpp, _vpp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_archive_subset": (_i, [_vp, _sz, _u32p, _u32, _vp, _sz, _u64p]),
}

class RaggedRect(ctypes.Structure):
    """ctypes image of `sicn_ragged_rect` (include/sicn_ragged_window.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("x0", "y0", "w", "h")]


class RaggedRoiPlan(ctypes.Structure):
    """ctypes image of `sicn_ragged_roi` (include/sicn_ragged_window.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("c0", "r0", "cw", "rh", "x", "y", "margin_lo", "margin_hi")]


class RaggedWindowImage(ctypes.Structure):
    """ctypes image of `sicn_ragged_window_image` (include/sicn_ragged_window.h)."""
    _fields_ = [("band_offset", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in ("band_bytes", "first_stream", "end_stream", "lead")]


_rectp = ctypes.POINTER(RaggedRect)
# include/sicn_ragged_window.h (library 0.12: a pixel rectangle of each image from its streams — window decoder 2 launches, cut 1)
RAGGED_WINDOW_ABI = {
    "sicn_ragged_roi_plan": (_i, [_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _rectp, ctypes.POINTER(RaggedRoiPlan)]),
    "sicn_ragged_window_layout": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, ctypes.POINTER(RaggedWindowImage), _u64p]),
    "sicn_ragged_window_create": (_i, [_vp, _u32p, _u32p, ctypes.POINTER(_vp)]),
    "sicn_ragged_window_free": (None, [_vp]),
    "sicn_ragged_window_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_window_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_cut_layout": (_i, [_i32p, _i32p, _rectp, _i, _u64p, _i, _i, _i64p]),
    "sicn_ragged_cut_create": (_i, [_i32p, _i32p, _rectp, _i, _u64p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_cut_free": (None, [_vp]),
    "sicn_ragged_cut_run": (_i, [_vp, _vp, _vp, _vp]),
}


class RaggedCtxWindowImage(ctypes.Structure):
    """ctypes image of `sicn_ragged_ctx_window_image` (include/sicn_ragged_ctx_window.h)."""
    _fields_ = [("band_offset", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in ("band_bytes", "band_row0", "band_rows")] + \
               [("first_stream", ctypes.c_uint32 * 2), ("end_stream", ctypes.c_uint32 * 2), ("symbols", ctypes.c_uint32)]


# include/sicn_ragged_ctx_window.h (library 0.13: a window of latent rows of each image from its rANS-WC streams — 7 enqueued operations)
RAGGED_CTX_WINDOW_ABI = {
    "sicn_ragged_ctx_window_layout": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _i, ctypes.POINTER(RaggedCtxWindowImage), _u64p]),
    "sicn_ragged_ctx_window_create": (_i, [_vp, _u32p, _u32p, ctypes.POINTER(_vp)]),
    "sicn_ragged_ctx_window_free": (None, [_vp]),
    "sicn_ragged_ctx_window_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_ctx_window_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# library 0.14: the stream length of the rANS-WC coder (mode 4) as an encoder parameter — the last argument of the uniform calls, one
# value per image (or NULL = 16384) after lat_c in the ragged ones
CTX_SL_ABI = {
    "sicn_codec_ctx_max_bytes_sl": (_sz, [_u32, _u32, _u32, _u32]),
    "sicn_codec_ctx_workspace_bytes_sl": (_sz, [_u32, _u32, _u32, _u32, _u32]),
    "sicn_codec_ctx_encode_batch_async_sl": (_i, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _sz, _vp, _vp, _sz, _vp, _u32]),
    "sicn_codec_ctx_decode_batch_async_sl": (_i, [_vp, _sz, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _sz, _vp, _u32]),
    "sicn_ragged_ctx_layout_sl": (_i, [_u32p, _u32p, _u32, _u32p, _i, ctypes.POINTER(RaggedCtxImage), _u64p]),
    "sicn_ragged_ctx_coder_create_sl": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_ctx_window_layout_sl": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, ctypes.POINTER(RaggedCtxWindowImage), _u64p]),
}

# include/sicn_ragged_rgb.h (library 0.15: a ragged net's RGB ends — conv 3 -> N, deconv N -> 3 — on packed-K kernels of their own)
RAGGED_RGB_ABI = {
    "sicn_ragged_net_create_rgb": (_i, [_descp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _i32p, _i32p, _i, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_net_kernel_for": (ctypes.c_char_p, [_vp, _i]),
    "sicn_ragged_rgb_layout": (_i, [_descp, _i, _i32p, _i32p, _i, _i, _i, _i, _i64p]),
}
RAGGED_RGB_ENDS = {"generic": 0, "packed": 1}     # SICN_RAGGED_RGB_GENERIC / SICN_RAGGED_RGB_PACKED

# include/sicn_ragged_planar.h (planar RGB [3][h][w] at a ragged net's pixel boundaries, the output at sizes of the caller's choice;
# sicn_version() stays 17 — these symbols being present is the marker)
RAGGED_PLANAR_ABI = {
    "sicn_ragged_net_create_planar": (_i, [_descp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _i32p, _i32p, _i, _i, _i, _i, _i32p, _i32p,
                                           ctypes.POINTER(_vp)]),
    "sicn_ragged_planar_layout": (_i, [_descp, _i, _i32p, _i32p, _i, _i, _i32p, _i32p, _i, _i64p]),
}
RAGGED_PIXELS = {"interleaved": 0, "planar": 1}   # SICN_RAGGED_PIXELS_INTERLEAVED / SICN_RAGGED_PIXELS_PLANAR

# include/sicn_ragged_rect.h (the last layer of a ragged net stores a rectangle of every reconstruction, in either pixel layout, at
# origins of the net's or from the caller's device memory; sicn_version() stays 17 — these symbols being present is the marker)
RAGGED_RECT_ABI = {
    "sicn_ragged_net_create_rect": (_i, [_descp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _i32p, _i32p, _i, _i, _i, _i, _rectp,
                                         ctypes.POINTER(_vp)]),
    "sicn_ragged_rect_layout": (_i, [_descp, _i, _i32p, _i32p, _i, _rectp, _i, _i64p]),
    "sicn_ragged_net_forward_at": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp, _vp]),
    "sicn_ragged_roi_move_origins": (_vp, [_vp]),
    "sicn_ragged_ctx_roi_move_origins": (_vp, [_vp]),
}


class RaggedRoiSlot(ctypes.Structure):
    """ctypes image of `sicn_ragged_roi_slot` (include/sicn_ragged_roi_move.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("image", "w", "h")]


class RaggedRoiPlaced(ctypes.Structure):
    """ctypes image of `sicn_ragged_roi_placed` (include/sicn_ragged_roi_move.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("x0", "y0", "c0", "r0", "cw", "rh", "x", "y")] + [("flags", ctypes.c_uint32)]


class RaggedRoiMoveSlot(ctypes.Structure):
    """ctypes image of `sicn_ragged_roi_move_slot` (include/sicn_ragged_roi_move.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("band_offset", "latent_offset", "recon_offset", "roi_offset", "workspace_offset")] + \
               [(n, ctypes.c_uint32) for n in ("cw_cap", "rh_cap", "max_streams", "first_item")]


_i32 = ctypes.c_int32
_slotp = ctypes.POINTER(RaggedRoiSlot)
# include/sicn_ragged_roi_move.h (library 0.17: the ROI decode with rectangles read from device memory on every call — 4 + 1 launches)
RAGGED_ROI_MOVE_ABI = {
    "sicn_ragged_roi_move_capacity": (_i, [_i, _i32, _i32, _i32, _i32, _i32, _i32, _i32p]),
    "sicn_ragged_roi_move_place": (_i, [_i, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(RaggedRoiPlaced)]),
    "sicn_ragged_roi_move_layout": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, _slotp, _i, ctypes.POINTER(RaggedRoiMoveSlot), _u64p]),
    "sicn_ragged_roi_move_create": (_i, [_vp, _slotp, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_roi_move_free": (None, [_vp]),
    "sicn_ragged_roi_move_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_roi_move_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_roi_move_cut_async": (_i, [_vp, _vp, _vp, _vp]),
}
ROI_MOVE_CLAMPED = 1      # SICN_ROI_MOVE_CLAMPED: flag bit 0, the position was clamped into the image


class RaggedCtxRoiPlaced(ctypes.Structure):
    """ctypes image of `sicn_ragged_ctx_roi_placed` (include/sicn_ragged_ctx_roi_move.h)."""
    _fields_ = [("px", RaggedRoiPlaced), ("first_stream", ctypes.c_uint32 * 2), ("end_stream", ctypes.c_uint32 * 2)] + \
               [(n, ctypes.c_uint32) for n in ("band_row0", "band_rows", "symbols", "pad")] + \
               [(n, ctypes.c_uint64) for n in ("lat_bias", "cut_offset")]


class RaggedCtxRoiMoveSlot(ctypes.Structure):
    """ctypes image of `sicn_ragged_ctx_roi_move_slot` (include/sicn_ragged_ctx_roi_move.h)."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("band_offset", "latent_offset", "recon_offset", "roi_offset", "meta_offset")] + \
               [(n, ctypes.c_uint32) for n in ("cw_cap", "rh_cap", "band_rows_cap")] + \
               [(n, ctypes.c_uint32 * 2) for n in ("max_streams", "first_item", "items")] + [("pad", ctypes.c_uint32)]


_u64 = ctypes.c_uint64
# include/sicn_ragged_ctx_roi_move.h (the moving ROI decode of the hyperprior configuration: prepare 3 launches per set of containers,
# decode 6 enqueued operations + cut 1 per move; sicn_version() stays 17 — these symbols being present is the marker)
RAGGED_CTX_ROI_MOVE_ABI = {
    "sicn_ragged_ctx_roi_move_capacity": (_i, [_u32, _u32, _u32, _u32, _u32, _u32p]),
    "sicn_ragged_ctx_roi_move_place": (_i, [_i32, _i32, _i32, _i32, _u32, _u32, _i32, _i32, _i32, _i32, _u64, ctypes.POINTER(RaggedCtxRoiPlaced)]),
    "sicn_ragged_ctx_roi_move_layout": (_i, [_u32p, _u32p, _u32, _u32p, _u32p, _u32p, _i, _slotp, _i, ctypes.POINTER(RaggedCtxRoiMoveSlot), _u64p]),
    "sicn_ragged_ctx_roi_move_create": (_i, [_vp, _slotp, _i, ctypes.POINTER(_vp)]),
    "sicn_ragged_ctx_roi_move_free": (None, [_vp]),
    "sicn_ragged_ctx_roi_move_workspace_bytes": (_sz, [_vp]),
    "sicn_ragged_ctx_roi_move_prepare_async": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_ctx_roi_move_decode_async": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sicn_ragged_ctx_roi_move_cut_async": (_i, [_vp, _vp, _vp, _vp]),
}
CTX_ROI_MOVE_STREAMS_PER_ITEM = 8      # SICN_CTX_ROI_MOVE_STREAMS_PER_ITEM

_lib = None


class SicnError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        msg = lib().sicn_strerror(code).decode() if _lib is not None else "?"
        super().__init__(f"{what}: {msg} ({code})")


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C {_PKG / 'csrc'}`; there is no non-HIP fallback")
        # PyTorch ships its own copy of the HIP runtime.  Device pointers handed to this library come from
        # torch, so both must live in ONE runtime: load torch's first and let libsicn.so bind to it (loaded
        # the other way round, the first launch fails with a HIP runtime error).
        try:
            import torch  # noqa: F401
        except ImportError:      # symbol checks etc. work without it
            pass
        L = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in {**ABI, **CODEC_ABI, **CONVLAYER_ABI, **GDN_ABI, **RAGGED_ABI, **RAGGED_HYPER_ABI, **RAGGED_CODEC_ABI, **RAGGED_CTX_ABI, **RAGGED_ARCHIVE_ABI,
                                  **RAGGED_ARCHIVE_SELECT_ABI, **RAGGED_WINDOW_ABI, **RAGGED_CTX_WINDOW_ABI, **CTX_SL_ABI, **RAGGED_RGB_ABI, **RAGGED_ROI_MOVE_ABI,
                                  **RAGGED_CTX_ROI_MOVE_ABI, **RAGGED_PLANAR_ABI, **RAGGED_RECT_ABI}.items():
            fn = getattr(L, name)          # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class Handle:
    """Base of every class that owns one library object in `self._h`: when the Python object goes, the object is given to the
    library function the class names in `_free`."""
    _free = ""

    def __del__(self):
        try:
            if getattr(self, "_h", None) and _lib is not None:
                # The free functions call hipFree, which must not land inside a stream capture: the garbage collector may run
                # this for an object of an earlier reference cycle at any allocation, also between two launches that are being
                # captured, and the captured graph then loses the order of its nodes.  Such an object waits for the next free
                # outside a capture.
                if _capturing():
                    _deferred.append((self._free, self._h))
                else:
                    while _deferred:
                        name, h = _deferred.pop()
                        getattr(_lib, name)(h)
                    getattr(_lib, self._free)(self._h)
                self._h = None
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass


_deferred = []      # (free function, handle) of objects collected while a stream capture was under way


def _capturing() -> bool:
    import sys
    torch = sys.modules.get("torch")
    return bool(torch is not None and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing())


def check(code: int, what: str) -> None:
    if code != 0:
        raise SicnError(code, what)
