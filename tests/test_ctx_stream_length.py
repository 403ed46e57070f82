"""The stream length of the rANS-WC coder (container mode 4) as an encoder parameter, 1024 .. 16384 (include/sicn_ctx_stream_length.h,
library 0.14): what can be checked without a GPU — the reference of the new ground (tests/cpp/ctx_sl_reference.c) held to the oracle,
the host arithmetic of every layer, every refusal, and the window plan at short lengths."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ctx_sl_cases as sl
from oracle import c_oracle
from simple_image_compression_network_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENOSPC = -22, -28
LENGTHS = sl.LENGTHS
# every latent the two new test modules encode (h, w, c)
EDGES = [(16, 32, 4), (16, 33, 4), (17, 32, 4), (1, 1, 4), (1, 5, 8), (3, 3, 4)]
BIG = [(37, 37, 192), (40, 48, 192)]
MIXED = [(37, 37, 192), (12, 16, 192), (40, 48, 192)]
ALL_LATENTS = EDGES + BIG + [(12, 16, 192), (64, 64, 192), (20, 24, 192)]
# (shape, variant) of every sl.latent the GPU module draws: variant 0 of every shape; the large batch's eight 64 x 64 images (variants
# 0 .. 7) and its 20 x 24 image (variant 8), also decoded alone; the graph replays' variants 1 and 2 of the mixed shapes.  The latents
# the networks make in the hyperprior tests are held to the oracle there, on the GPU.
GPU_LATENTS = ([(sh, 0) for sh in ALL_LATENTS] + [((64, 64, 192), v) for v in range(1, 8)] + [((20, 24, 192), 8)]
               + [(sh, v) for sh in MIXED for v in (1, 2)])


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sicn_ctx_stream_length.h").read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol_and_the_binding_table_names_them():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == sorted(["sicn_codec_ctx_max_bytes_sl", "sicn_codec_ctx_workspace_bytes_sl", "sicn_codec_ctx_encode_batch_async_sl",
                           "sicn_codec_ctx_decode_batch_async_sl", "sicn_ragged_ctx_layout_sl", "sicn_ragged_ctx_coder_create_sl",
                           "sicn_ragged_ctx_window_layout_sl"])
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.CTX_SL_ABI), "python binding table and sicn_ctx_stream_length.h disagree"
    for other in (_lib.ABI, _lib.CODEC_ABI, _lib.RAGGED_CTX_ABI, _lib.RAGGED_CTX_WINDOW_ABI, _lib.RAGGED_CODEC_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() >= 14


# ---- the reference, held to the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", GPU_LATENTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"v{v}")
def test_reference_at_16384_is_the_oracle_byte_for_byte(shape, variant):
    y, s = sl.latent(shape, variant)
    want = c_oracle.ctx_encode(y, s, sl.image_wh(shape))
    assert sl.container(shape, 16384, variant) == want
    n, back = sl.ref_decode(want, s, 16384)                  # its decoder reads the oracle's container
    assert n == y.size and np.array_equal(back, y)
    assert np.array_equal(c_oracle.ctx_decode(sl.container(shape, 16384, variant), s)[0], y)


@pytest.mark.parametrize("shape", EDGES + BIG + [(12, 16, 192)], ids=lambda s: "x".join(map(str, s)))
def test_reference_at_every_length_round_trips_and_differs_where_it_must(shape):
    y, s = sl.latent(shape)
    h, w, c = shape
    head0, tables0, _ = sl.fields(sl.container(shape, 16384))
    for S in LENGTHS:
        blob = sl.container(shape, S)
        n, back = sl.ref_decode(blob, s, S)
        assert n == y.size and np.array_equal(back, y), S
        head, tables, lens = sl.fields(blob)
        assert tables == tables0, S                          # the class tables do not depend on how the sets are cut
        assert [i for i in range(12) if head[i] != head0[i]] in ([8, 9, 10], [9, 10], [9]) or S == 16384, (S, head, head0)
        nsym, nst = sl.geometry(h, w, c, S)
        assert head[8] == sum(nst) == lens.size and head[9] == S and head[10] == int(lens.sum())
        assert len(blob) == sl.HEADER + sl.TABLES + 4 * sum(nst) + int(lens.sum()) <= sl.max_bytes(h, w, c, S)
        assert int(lens.max()) <= sl.cap(S) and int(lens.min()) >= 256
        if S != 16384:                                       # a decoder told another length refuses: the header class
            assert sl.ref_decode(blob, s, 16384)[0] == -sl.V_HEADER


def test_one_stream_per_set_at_1024_is_the_oracles_container_but_for_dword_9():
    shape = (16, 32, 4)                                      # 1024 symbols per set: one stream each at every length
    y, s = sl.latent(shape)
    assert sl.geometry(*shape, 1024) == ((1024, 1024), (1, 1))
    want = bytearray(c_oracle.ctx_encode(y, s, sl.image_wh(shape)))
    assert want[36:40] == (16384).to_bytes(4, "little")
    want[36:40] = (1024).to_bytes(4, "little")
    assert sl.container(shape, 1024) == bytes(want)


# ---- host arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", LENGTHS)
def test_size_functions_are_the_references_arithmetic(S):
    L = _lib.lib()
    ref = sl.ref()
    for h, w, c in ALL_LATENTS + [(135, 240, 192), (1, 8193, 4), (270, 480, 192)]:
        assert L.sicn_codec_ctx_max_bytes_sl(w, h, c, S) == ref.ctxsl_max_bytes(w, h, c, S) == sl.max_bytes(h, w, c, S)
        ws = L.sicn_codec_ctx_workspace_bytes_sl(w, h, c, 3, S)
        assert ws == 3 * L.sicn_codec_ctx_workspace_bytes_sl(w, h, c, 1, S) and ws % 256 == 0
        assert ws // 3 >= sum(sl.geometry(h, w, c, S)[1]) * sl.cap(S)       # room for every stream's scratch slot
        if S == 16384:
            assert L.sicn_codec_ctx_max_bytes_sl(w, h, c, S) == L.sicn_codec_ctx_max_bytes(w, h, c)
            assert ws == L.sicn_codec_ctx_workspace_bytes(w, h, c, 3)


def _layout(shapes, c, lengths, want_images=True):
    n = len(shapes)
    images = (_lib.RaggedCtxImage * max(n, 1))() if want_images else None
    totals = (ctypes.c_uint64 * 3)()
    rc = _lib.lib().sicn_ragged_ctx_layout_sl(_u32([w for _, w in shapes]), _u32([h for h, _ in shapes]), c,
                                              None if lengths is None else _u32(lengths), n, images, totals)
    return rc, (list(images)[:n] if want_images else None), [int(v) for v in totals]


def test_ragged_layout_with_mixed_lengths_is_python_arithmetic():
    L = _lib.lib()
    shapes = [(37, 37), (1, 1), (40, 48), (12, 16), (3, 5)]
    lengths = [1024, 16384, 4096, 2048, 8192]
    rc, images, totals = _layout(shapes, 192, lengths)
    assert rc == 0
    lat = slot = ws = 0
    for (h, w), S, im in zip(shapes, lengths, images):
        _, nst = sl.geometry(h, w, 192, S)
        sb = -(-sl.max_bytes(h, w, 192, S) // 16) * 16
        assert (im.latent_offset, im.slot_offset, im.workspace_offset, im.slot_bytes) == (lat, slot, ws, sb)
        assert (im.n_symbols, im.anchor_streams, im.nonanchor_streams) == (h * w * 192, *nst)
        lat, slot, ws = lat + h * w * 192, slot + sb, ws + L.sicn_codec_ctx_workspace_bytes_sl(w, h, 192, 1, S)
    assert totals == [lat, slot, ws]
    # NULL lengths, and 16384 for every image, are the call without lengths
    old = (ctypes.c_uint64 * 3)()
    assert L.sicn_ragged_ctx_layout(_u32([w for _, w in shapes]), _u32([h for h, _ in shapes]), 192, len(shapes), None, old) == 0
    assert _layout(shapes, 192, None)[2] == _layout(shapes, 192, [16384] * 5)[2] == [int(v) for v in old]


def test_ragged_layout_past_4_gib_of_workspace():
    # six images of 0x3F000000 symbols, at 2048 and 4096 in turn: 516 096 streams of 4352 scratch bytes are 2.2 GB of workspace for one
    # image (one image's scratch stays below 2^32 by the symbol limit; a batch's need not)
    w, h, c = 0x3F0000 // 4, 256, 4
    lengths = [2048, 4096] * 3
    rc, images, totals = _layout([(h, w)] * 6, c, lengths)
    assert rc == 0
    one = {S: _lib.lib().sicn_codec_ctx_workspace_bytes_sl(w, h, c, 1, S) for S in (2048, 4096)}
    assert 516096 * sl.cap(2048) < one[2048] < 2 ** 32 and one[4096] < one[2048]
    at = 0
    for im, S in zip(images, lengths):
        assert im.workspace_offset == at
        at += one[S]
    assert totals[2] == at == 3 * (one[2048] + one[4096]) > 2 ** 32 and images[5].workspace_offset > 2 ** 32
    assert images[5].latent_offset == 5 * 0x3F000000 > 2 ** 32


def test_every_refusal_of_a_length():
    L = _lib.lib()
    for bad in (512, 1536, 32768, 0, 16385, 2 ** 31):
        assert L.sicn_codec_ctx_max_bytes_sl(8, 8, 4, bad) == 0
        assert L.sicn_codec_ctx_workspace_bytes_sl(8, 8, 4, 1, bad) == 0
        assert sl.ref().ctxsl_max_bytes(8, 8, 4, bad) == 0
        assert _layout([(8, 8)], 4, [bad])[0] == EINVAL
        assert _layout([(8, 8), (8, 8)], 4, [1024, bad])[0] == EINVAL                        # ... in any image
        h = ctypes.c_void_p()
        assert L.sicn_ragged_ctx_coder_create_sl(_u32([8]), _u32([8]), 4, _u32([bad]), None, None, 1, ctypes.byref(h)) == EINVAL and not h.value
        assert L.sicn_ragged_ctx_window_layout_sl(_u32([8]), _u32([8]), 4, _u32([bad]), _u32([0]), _u32([1]), 1, None, None) == EINVAL
        d = ctypes.c_void_p(64)
        assert L.sicn_codec_ctx_encode_batch_async_sl(d, d, 1, 8, 8, 4, 0, 0, d, 1 << 20, d, d, 1 << 20, None, bad) == EINVAL
        assert L.sicn_codec_ctx_decode_batch_async_sl(d, 1 << 20, None, d, 1, 8, 8, 4, d, d, d, 1 << 20, None, bad) == EINVAL
    # the symbol limit: (anchor + non-anchor streams) * (2 S + 256) < 2^32.  At 1024 that is 1 864 135 streams
    w, c = 0x7F0000 // 4, 4
    assert _layout([(256, w)], c, [16384])[0] == 0                                           # 0x7F000000 symbols: the old limit
    assert _layout([(256, w)], c, [1024])[0] == EINVAL
    assert L.sicn_codec_ctx_max_bytes_sl(w, 256, c, 1024) > 0                                # (the size function states no shape limit)
    h = 2 * 932067                                          # 2 * 932067 streams of 1024 = 1 864 134: the last shape that fits
    assert (h // 2) * 256 * 4 // 1024 * 2 == 1864134 and 1864134 * sl.cap(1024) < 2 ** 32 <= 1864136 * sl.cap(1024)
    assert _layout([(h, 256)], 4, [1024])[0] == 0 and sl.ref().ctxsl_max_bytes(256, h, 4, 1024) > 0
    assert _layout([(h + 2, 256)], 4, [1024])[0] == EINVAL and sl.ref().ctxsl_max_bytes(256, h + 2, 4, 1024) == 0
    assert _layout([(h + 2, 256)], 4, [2048])[0] == 0


def test_device_calls_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    d, S = ctypes.c_void_p(64), 1024
    slot, ws = L.sicn_codec_ctx_max_bytes_sl(8, 8, 4, S), L.sicn_codec_ctx_workspace_bytes_sl(8, 8, 4, 1, S)
    enc, dec = L.sicn_codec_ctx_encode_batch_async_sl, L.sicn_codec_ctx_decode_batch_async_sl
    assert enc(None, d, 1, 8, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == EINVAL
    assert enc(d, None, 1, 8, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == EINVAL
    assert enc(d, d, 1, 8, 8, 4, 0, 0, None, slot, d, d, ws, None, S) == EINVAL
    assert enc(d, d, 1, 8, 8, 4, 0, 0, d, slot, None, d, ws, None, S) == EINVAL
    assert enc(d, d, 1, 8, 8, 6, 0, 0, d, slot, d, d, ws, None, S) == EINVAL                 # lat_c % 4
    assert enc(d, d, 1, 0, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == EINVAL
    assert enc(d, d, 65536, 8, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == EINVAL
    assert enc(ctypes.c_void_p(66), d, 1, 8, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == EINVAL
    assert enc(d, d, 1, 8, 8, 4, 0, 0, d, slot - 2, d, d, ws, None, S) == ENOSPC
    assert enc(d, d, 1, 8, 8, 4, 0, 0, d, slot + 1, d, d, ws, None, S) == ENOSPC             # odd slots
    assert enc(d, d, 1, 8, 8, 4, 0, 0, d, slot, d, d, ws - 1, None, S) == ENOSPC
    assert enc(d, d, 1, 8, 8, 4, 0, 0, d, slot, d, None, ws, None, S) == ENOSPC
    assert enc(d, d, 0, 8, 8, 4, 0, 0, d, slot, d, d, ws, None, S) == 0                      # an empty batch enqueues nothing
    # a slot sized for 16384 is too small for the same shape at 1024 where the latent has more than one stream per set
    assert L.sicn_codec_ctx_max_bytes(37, 37, 192) < L.sicn_codec_ctx_max_bytes_sl(37, 37, 192, 1024)
    assert enc(d, d, 1, 37, 37, 192, 0, 0, d, L.sicn_codec_ctx_max_bytes(37, 37, 192), d, d, 1 << 30, None, S) == ENOSPC
    assert dec(None, slot, None, d, 1, 8, 8, 4, d, d, d, ws, None, S) == EINVAL
    assert dec(d, slot, None, None, 1, 8, 8, 4, d, d, d, ws, None, S) == EINVAL
    assert dec(d, slot, None, d, 1, 8, 8, 4, None, d, d, ws, None, S) == EINVAL
    assert dec(d, slot, None, d, 1, 8, 8, 4, d, None, d, ws, None, S) == EINVAL
    assert dec(d, slot + 1, None, d, 1, 8, 8, 4, d, d, d, ws, None, S) == EINVAL
    assert dec(d, slot, None, d, 1, 8, 8, 4, d, d, d, ws - 1, None, S) == ENOSPC
    assert dec(d, slot, None, d, 0, 8, 8, 4, d, d, d, ws, None, S) == 0
    h = ctypes.c_void_p()
    assert L.sicn_ragged_ctx_coder_create_sl(_u32([8]), _u32([8]), 4, _u32([S]), None, None, 1, None) == EINVAL
    assert L.sicn_ragged_ctx_coder_create_sl(None, _u32([8]), 4, _u32([S]), None, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_coder_create_sl(_u32([8]), _u32([8]), 4, _u32([S]), None, None, 0, ctypes.byref(h)) == EINVAL and not h.value
    rc = L.sicn_ragged_ctx_coder_create_sl(_u32([9]), _u32([7]), 192, _u32([S]), None, None, 1, ctypes.byref(h))
    assert rc in (0, -19)                                    # no gfx950 device here: SICN_ENODEV, nothing made
    if rc == 0:
        assert L.sicn_ragged_ctx_coder_workspace_bytes(h) == L.sicn_codec_ctx_workspace_bytes_sl(9, 7, 192, 1, S)
        L.sicn_ragged_ctx_coder_free(h)


def test_python_classes_refuse_a_bad_length_before_anything_is_made():
    from simple_image_compression_network_amd import codec
    for bad in (512, 1536, 32768):
        with pytest.raises(ValueError):
            codec.ContextCoder(1, 8, 8, 4, stream_symbols=bad)
        with pytest.raises(ValueError):
            codec.RaggedContextCoder([(8, 8)], 4, stream_symbols=bad)
        with pytest.raises(ValueError):
            codec.RaggedContextCoder([(8, 8), (4, 4)], 4, stream_symbols=[1024, bad])
    with pytest.raises(ValueError):
        codec.RaggedContextCoder([(8, 8), (4, 4)], 4, stream_symbols=[1024])
    assert codec._ctx_stream_symbols(None, 3) == [16384] * 3 and codec._ctx_stream_symbols(2048, 2) == [2048, 2048]
    head = np.frombuffer(sl.container((3, 3, 4), 4096)[:48], "<u4")                   # a numpy integer, as read from a header
    assert codec._ctx_stream_symbols(head[9], 2) == [4096, 4096] and codec._ctx_stream_symbols([head[9], None], 2) == [4096, 16384]
    for bad in (np.uint32(1536), True, 2048.0):
        with pytest.raises((ValueError, TypeError)):
            codec._ctx_stream_symbols(bad, 1)
    with pytest.raises(ValueError):
        codec._ctx_stream_symbols(np.uint32(1536), 1)


def test_parse_header_reads_the_length_of_a_mode_4_container():
    from simple_image_compression_network_amd import codec
    for S in LENGTHS:
        info = codec.parse_header(sl.container((37, 37, 192), S)[:48])
        nst = sl.geometry(37, 37, 192, S)[1]
        assert (int(info.mode), int(info.stream_symbols), int(info.n_streams)) == (4, S, sum(nst))
    bad = bytearray(sl.container((37, 37, 192), 1024)[:48])
    bad[36:40] = (1536).to_bytes(4, "little")
    with pytest.raises(_lib.SicnError):
        codec.parse_header(bytes(bad))
    bad[36:40] = (2048).to_bytes(4, "little")                # an admissible length the stream count does not go with
    with pytest.raises(_lib.SicnError):
        codec.parse_header(bytes(bad))


# ---- the window plan at short lengths --------------------------------------------------------------------------------------------
WINDOW_SHAPES = [(1, 1, 4), (2, 2, 4), (5, 1, 192), (3, 3, 192), (37, 37, 192), (40, 48, 192)]


def _window_layout(shapes, rows, c, lengths):
    n = len(shapes)
    images = (_lib.RaggedCtxWindowImage * max(n, 1))()
    totals = (ctypes.c_uint64 * 2)()
    rc = _lib.lib().sicn_ragged_ctx_window_layout_sl(_u32([w for _, w in shapes]), _u32([h for h, _ in shapes]), c,
                                                     None if lengths is None else _u32(lengths), _u32([r for r, _ in rows]),
                                                     _u32([h for _, h in rows]), n, images, totals)
    return rc, list(images)[:n], [int(v) for v in totals]


def _python_plan(H, W, C, S, r0, rh):
    """The plan of include/sicn_ragged_ctx_window.h, in its words, with the image's S: (band_row0, band_rows, first[2], end[2], symbols)."""
    R, r1 = W * C, r0 + rh
    nsym, _ = sl.geometry(H, W, C, S)
    ceil = lambda a, b: -(-a // b)
    lo, hi = (r0 >> 1) * R, min(nsym[1], ((r1 + 1) >> 1) * R)
    P0 = P1 = N0 = N1 = 0
    if hi > lo:
        N0, N1 = lo // S, ceil(hi, S)
        P0, P1 = N0 * S // R, ceil(min(nsym[1], N1 * S), R)
        A0, A1 = max(0, min(r0, 2 * P0 - 1)), min(H, max(r1, 2 * P1 + 1))
    else:
        A0, A1 = r0, r1
    M0, M1 = (A0 >> 1) * R // S, ceil(min(nsym[0], ((A1 + 1) >> 1) * R), S)
    Q0, Q1 = M0 * S // R, ceil(min(nsym[0], M1 * S), R)
    B0, B1 = (2 * min(P0, Q0), min(H, 2 * max(P1, Q1))) if hi > lo else (2 * Q0, min(H, 2 * Q1))
    symbols = min(nsym[0], M1 * S) - M0 * S + (min(nsym[1], N1 * S) - N0 * S if hi > lo else 0)
    return B0, B1 - B0, (M0, N0), (M1, N1), symbols


def _pixel_streams(H, W, C, S):
    """Per pixel [H][W]: its set, and the first and the last stream (the set's own numbering) that hold its C symbols, from the
    numpy statement of the coding order applied to the symbols' own indices."""
    index = np.arange(H * W * C, dtype=np.int64).reshape(H, W, C)
    order = sl.set_order(index)
    na = sl.geometry(H, W, C, S)[0][0]
    pos = np.empty(H * W * C, np.int64)
    pos[order] = np.arange(order.size)
    pos = pos.reshape(H, W, C)
    py, px = np.mgrid[0:H, 0:W]
    anchor = (px + py) % 2 == 0
    stream = np.where(anchor[:, :, None], pos, pos - na) // S
    return (~anchor).astype(np.int64), stream[:, :, 0], stream[:, :, -1]


@pytest.mark.parametrize("S", [1024, 4096])
@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_window_layout_is_the_headers_arithmetic_and_sufficient(shape, S):
    H, W, C = shape
    rows = [(r0, rh) for r0 in range(H) for rh in range(1, H - r0 + 1)]           # every window
    rc, images, totals = _window_layout([(H, W)] * len(rows), rows, C, [S] * len(rows))
    assert rc == 0
    pset, first, last = _pixel_streams(H, W, C, S)
    nst = sl.geometry(H, W, C, S)[1]
    at = 0
    for (r0, rh), im in zip(rows, images):
        b0, brows, f, e, symbols = _python_plan(H, W, C, S, r0, rh)
        assert (im.band_row0, im.band_rows, tuple(im.first_stream), tuple(im.end_stream), im.symbols) == (b0, brows, f, e, symbols), (r0, rh)
        assert im.band_bytes == brows * W * C and im.band_offset == at and at % 16 == 0
        at += -(-im.band_bytes // 16) * 16
        lo, hi = np.array(f)[pset], np.array(e)[pset]
        whole = (first >= lo) & (last < hi)                   # every symbol of the pixel is in a selected stream
        some = ((first >= lo) & (first < hi)) | ((last >= lo) & (last < hi))
        assert whole[r0:r0 + rh].all(), (r0, rh)              # the wanted rows are held
        held_rows = np.nonzero(some.any(axis=1))[0]
        assert held_rows.min() >= b0 and held_rows.max() < b0 + brows, (r0, rh)   # every symbol of a selected stream lies in the band
        assert b0 <= r0 and r0 + rh <= b0 + brows <= H
        held_other = some & (pset == 1)
        need = np.zeros((H, W), bool)                         # the in-range 4-neighbours of every held non-anchor
        need[:-1] |= held_other[1:]
        need[1:] |= held_other[:-1]
        need[:, :-1] |= held_other[:, 1:]
        need[:, 1:] |= held_other[:, :-1]
        assert whole[need].all(), (r0, rh)
        if (r0, rh) == (0, H):
            assert (b0, brows, f, e, symbols) == (0, H, (0, 0), nst, H * W * C)
    assert totals[0] == at
    ws = _layout([(H, W)] * len(rows), C, [S] * len(rows), want_images=False)[2]
    assert totals[1] == ws[2]                                 # the full coder's workspace at that length


def test_window_layout_without_lengths_is_the_old_call_and_shorter_streams_select_fewer_rows():
    L = _lib.lib()
    shapes, rows = [(40, 48), (37, 37)], [(7, 9), (30, 7)]
    old_images = (_lib.RaggedCtxWindowImage * 2)()
    old = (ctypes.c_uint64 * 2)()
    assert L.sicn_ragged_ctx_window_layout(_u32([48, 37]), _u32([40, 37]), 192, _u32([7, 30]), _u32([9, 7]), 2, old_images, old) == 0
    for lengths in (None, [16384, 16384]):
        rc, images, totals = _window_layout(shapes, rows, 192, lengths)
        assert rc == 0 and totals == [int(v) for v in old]
        assert all(bytes(a) == bytes(b) for a, b in zip(images, old_images))
    # a 40 x 48 x 192 latent has 40 rows: the middle 16 of them; the band shrinks with S, strictly from 16384 to 1024
    bands = {S: _window_layout([(40, 48)], [(12, 16)], 192, [S])[1][0].band_rows for S in LENGTHS}
    assert bands[1024] < bands[16384] and all(bands[a] <= bands[b] for a, b in zip(LENGTHS, LENGTHS[1:])), bands
    # and 76 rows in the middle of a tall latent of the same width
    tall = {S: _window_layout([(160, 48)], [(42, 76)], 192, [S])[1][0].band_rows for S in LENGTHS}
    assert 76 <= tall[1024] < tall[16384], tall
    mixed = _window_layout([(40, 48), (40, 48)], [(12, 16), (12, 16)], 192, [1024, 16384])[1]
    assert (mixed[0].band_rows, mixed[1].band_rows) == (bands[1024], bands[16384])            # the length is the image's


# ---- the host arithmetic under the sanitizers ------------------------------------------------------------------------------------
def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/ctx_sl_plan_check.cpp — csrc/ctx_window_host.hpp at every stream length, with its own main — built with the address and undefined-behaviour sanitizers and run as a child process.  Host code only;
    nothing is loaded into Python."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ctx_sl_plan_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ctx_sl_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ctx_sl_plan_check ok: \d+ checks", r.stdout), r.stdout
