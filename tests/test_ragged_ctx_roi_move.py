"""CPU-only checks of the hyperprior moving ROI decode's host side (include/sicn_ragged_ctx_roi_move.h): the symbols and the binding
table; the stream and band capacities by brute force against a Python restatement of the header's plan — sufficient at every
admissible position and TIGHT, each attained somewhere; the placement against sicn_ragged_ctx_window_layout_sl of the placed rows and
against sicn_ragged_roi_move_place, with lat_bias and the latent cut's source held inside the slot's band for every position, the
extremes of int32 included; the layout against plain Python arithmetic; every refusal; the argument checks of the device calls that
come before a device is asked for; and the pure-host header under the host sanitizers.  Nothing here touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simple_image_compression_network_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENOSPC = -22, -28
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
LAT_C = 192
WPB = 8
SYMBOLS = ["sicn_ragged_ctx_roi_move_capacity", "sicn_ragged_ctx_roi_move_place", "sicn_ragged_ctx_roi_move_layout",
           "sicn_ragged_ctx_roi_move_create", "sicn_ragged_ctx_roi_move_free", "sicn_ragged_ctx_roi_move_workspace_bytes",
           "sicn_ragged_ctx_roi_move_prepare_async", "sicn_ragged_ctx_roi_move_decode_async", "sicn_ragged_ctx_roi_move_cut_async"]


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _lat(size):
    return -(-size[0] // 16), -(-size[1] // 16)


def test_library_exports_every_declared_symbol_and_the_version_stays():
    L = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sicn_ragged_ctx_roi_move.h").read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(SYMBOLS)
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_CTX_ROI_MOVE_ABI), "python binding table and sicn_ragged_ctx_roi_move.h disagree"
    others = [v for k, v in vars(_lib).items() if k.endswith("ABI") and isinstance(v, dict) and v is not _lib.RAGGED_CTX_ROI_MOVE_ABI]
    assert len(others) >= 15
    for other in others:
        assert not set(syms) & set(other)
    assert L.sicn_version() == 17                                           # the symbols being present is the marker
    assert _lib.CTX_ROI_MOVE_STREAMS_PER_ITEM == WPB
    assert f"#define SICN_CTX_ROI_MOVE_STREAMS_PER_ITEM {WPB}" in text
    # the ctypes images have the C structs' sizes: 9 + 4 + 4 dwords and two 64-bit words behind a pad; 5 64-bit words and 10 dwords
    assert ctypes.sizeof(_lib.RaggedCtxRoiPlaced) == 88 and ctypes.sizeof(_lib.RaggedCtxRoiMoveSlot) == 80


# ---- the header's plan, restated ------------------------------------------------------------------------------------------------
def _plan(W, H, C, S, r0, rh):
    """include/sicn_ragged_ctx_window.h, the paragraph "Plan": (M0, M1, N0, N1, B0, B1, symbols)."""
    R, r1 = W * C, r0 + rh
    nsym = [((H // 2) * W + ((W + 1) // 2 if H & 1 else 0)) * C, ((H // 2) * W + (W // 2 if H & 1 else 0)) * C]
    cd = lambda a, b: -(-a // b)
    lo, hi = (r0 >> 1) * R, min(nsym[1], ((r1 + 1) >> 1) * R)
    if hi > lo:
        N0, N1 = lo // S, cd(hi, S)
        P0, P1 = N0 * S // R, cd(min(nsym[1], N1 * S), R)
        A0, A1 = max(0, min(r0, 2 * P0 - 1)), min(H, max(r1, 2 * P1 + 1))
    else:
        N0 = N1 = 0
        A0, A1 = r0, r1
    M0, M1 = (A0 >> 1) * R // S, cd(min(nsym[0], ((A1 + 1) >> 1) * R), S)
    Q0, Q1 = M0 * S // R, cd(min(nsym[0], M1 * S), R)
    B0, B1 = (2 * min(P0, Q0), min(H, 2 * max(P1, Q1))) if hi > lo else (2 * Q0, min(H, 2 * Q1))
    symbols = min(nsym[0], M1 * S) - M0 * S + ((min(nsym[1], N1 * S) - N0 * S) if hi > lo else 0)
    return M0, M1, N0, N1, B0, B1, symbols


def _capacity(W, H, C, S, rh):
    cap = (ctypes.c_uint32 * 3)()
    rc = _lib.lib().sicn_ragged_ctx_roi_move_capacity(W, H, C, S, rh, cap)
    return rc, tuple(int(v) for v in cap)


LATENTS = [(37, 37, 192), (10, 40, 192), (48, 40, 192), (3, 3, 192), (1, 5, 192), (5, 1, 192), (1, 1, 4)]       # (W, H, C)


@pytest.mark.parametrize("S", [1024, 16384])
@pytest.mark.parametrize("W,H,C", LATENTS)
def test_capacity_is_sufficient_and_tight(W, H, C, S):
    for rh in sorted({1, 3, 5, H}):
        if rh > H:
            continue
        rc, cap = _capacity(W, H, C, S, rh)
        assert rc == 0
        seen = [0, 0, 0]
        for r0 in range(H - rh + 1):
            M0, M1, N0, N1, B0, B1, _ = _plan(W, H, C, S, r0, rh)
            now = (M1 - M0, N1 - N0, B1 - B0)
            assert all(v <= c for v, c in zip(now, cap)), ("not sufficient", r0, now, cap)
            assert B0 <= r0 and r0 + rh <= B1, "the band holds the rows asked for"
            seen = [max(a, b) for a, b in zip(seen, now)]
        assert tuple(seen) == cap, ("not tight", seen, cap)
    if (W, H) == (1, 1):
        assert _capacity(W, H, C, S, 1) == (0, (1, 0, 1))                      # no non-anchor stream
    if (W, H, S) == (37, 37, 1024):                                            # the figures of the header's example
        assert _capacity(W, H, C, S, 5) == (0, (50, 22, 18))
        per = [_plan(W, H, C, S, r0, 5) for r0 in range(33)]
        assert (min(p[1] - p[0] for p in per), min(p[3] - p[2] for p in per), min(p[5] - p[4] for p in per)) == (25, 18, 9)
    if (W, H, S) == (10, 40, 16384):
        assert _capacity(W, H, C, S, 5) == (0, (3, 2, 40))


def test_capacity_refusals():
    assert _capacity(7, 9, 192, 1024, 5)[0] == 0
    for args in [(0, 9, 192, 1024, 5), (7, 0, 192, 1024, 5), (7, 9, 0, 1024, 5), (7, 9, 190, 1024, 5), (7, 9, 192, 1000, 5),
                 (7, 9, 192, 512, 5), (7, 9, 192, 32768, 5), (7, 9, 192, 1024, 0), (7, 9, 192, 1024, 10), (2 ** 16, 2 ** 16, 4, 1024, 1)]:
        assert _capacity(*args)[0] == EINVAL, args
    assert _lib.lib().sicn_ragged_ctx_roi_move_capacity(7, 9, 192, 1024, 5, None) == EINVAL


# ---- placement ------------------------------------------------------------------------------------------------------------------
def _place(size, S, w, h, x0, y0, band_offset=0, c=LAT_C, lat=None):
    lw, lh = _lat(size) if lat is None else lat
    p = _lib.RaggedCtxRoiPlaced()
    rc = _lib.lib().sicn_ragged_ctx_roi_move_place(size[0], size[1], lw, lh, c, S, w, h, x0, y0, band_offset, ctypes.byref(p))
    return rc, p


@pytest.mark.parametrize("S", [1024, 16384])
@pytest.mark.parametrize("size", [(592, 592), (160, 640)])
def test_place_against_the_window_plan(size, S):
    L = _lib.lib()
    W, H = size
    lw, lh = _lat(size)
    R = lw * LAT_C
    BAND = 48 * 2 ** 20 + 16                                                 # where this slot's band would lie
    for h in (1, 20, 33):
        w = 20
        cap2 = (ctypes.c_int32 * 2)()
        assert L.sicn_ragged_roi_move_capacity(4, W, H, lw, lh, w, h, cap2) == 0
        rh_cap = int(cap2[1])
        rc, (m0, m1, rows_cap) = _capacity(lw, lh, LAT_C, S, rh_cap)
        assert rc == 0
        ys = list(range(0, H - h + 1)) + [-1, -17, H - h + 1, H, INT32_MIN, INT32_MIN + 1, INT32_MAX, INT32_MAX - 1]
        hit = [0, 0, 0]
        for y0 in ys:
            x0 = (7 * y0) % (W - w + 1) if 0 <= y0 <= H - h else (INT32_MAX if y0 & 1 else INT32_MIN)
            rc, p = _place(size, S, w, h, x0, y0, BAND)
            q = _lib.RaggedRoiPlaced()
            assert rc == 0 and L.sicn_ragged_roi_move_place(4, W, H, lw, lh, w, h, x0, y0, ctypes.byref(q)) == 0
            assert all(getattr(p.px, k) == getattr(q, k) for k, _ in _lib.RaggedRoiPlaced._fields_), "the pixel axes are 0.17's"
            assert p.px.rh == rh_cap and 0 <= p.px.r0 <= lh - rh_cap
            im = (_lib.RaggedCtxWindowImage * 1)()
            totals = (ctypes.c_uint64 * 2)()
            assert L.sicn_ragged_ctx_window_layout_sl(_u32([lw]), _u32([lh]), LAT_C, _u32([S]), _u32([p.px.r0]), _u32([rh_cap]), 1, im, totals) == 0
            assert (list(p.first_stream), list(p.end_stream)) == (list(im[0].first_stream), list(im[0].end_stream))
            assert (p.band_row0, p.band_rows, p.symbols) == (im[0].band_row0, im[0].band_rows, im[0].symbols)
            assert (p.band_row0, p.band_row0 + p.band_rows) == _plan(lw, lh, LAT_C, S, p.px.r0, rh_cap)[4:6]
            sel = (p.end_stream[0] - p.first_stream[0], p.end_stream[1] - p.first_stream[1], p.band_rows)
            assert sel[0] <= m0 and sel[1] <= m1 and sel[2] <= rows_cap
            hit = [max(a, b) for a, b in zip(hit, sel)]
            # the band: row band_row0 is its first byte, and the window the cut reads lies inside its capacity
            assert (p.lat_bias + p.band_row0 * R) % 2 ** 64 == BAND
            assert p.cut_offset == BAND + (p.px.r0 - p.band_row0) * R + p.px.c0 * LAT_C
            assert BAND <= p.cut_offset and p.cut_offset + (rh_cap - 1) * R + p.px.cw * LAT_C <= BAND + p.band_rows * R <= BAND + rows_cap * R
        assert tuple(hit) == (m0, m1, rows_cap), "every capacity is met by some pixel position"


def test_place_refusals():
    size = (112, 144)
    assert _place(size, 1024, 20, 20, 0, 0)[0] == 0
    for w, h in [(0, 20), (20, 0), (-1, 20), (113, 20), (20, 145), (INT32_MAX, INT32_MAX), (INT32_MIN, 1)]:
        assert _place(size, 1024, w, h, 0, 0)[0] == EINVAL, (w, h)
    assert _place(size, 1000, 20, 20, 0, 0)[0] == EINVAL and _place(size, 1024, 20, 20, 0, 0, c=190)[0] == EINVAL
    assert _place(size, 1024, 20, 20, 0, 0, c=0)[0] == EINVAL
    assert _place((113, 144), 1024, 20, 20, 0, 0, lat=(7, 9))[0] == EINVAL        # an image larger than its latent reconstructs
    assert _place((0, 144), 1024, 1, 1, 0, 0, lat=(7, 9))[0] == EINVAL and _place(size, 1024, 1, 1, 0, 0, lat=(0, 9))[0] == EINVAL
    assert _place(size, 1024, 20, 20, 0, 0, band_offset=2 ** 62)[0] == EINVAL
    assert _lib.lib().sicn_ragged_ctx_roi_move_place(112, 144, 7, 9, 192, 1024, 1, 1, 0, 0, 0, None) == EINVAL


# ---- the layout -------------------------------------------------------------------------------------------------------------------
SIZES = [(592, 592), (160, 640), (48, 48), (100, 36), (16, 16)]           # (width, height)
SLOTS = [(0, 20, 20), (1, 33, 15), (0, 256, 15), (1, 17, 400), (2, 16, 16), (3, 33, 15), (4, 16, 16), (0, 20, 20), (1, 160, 640)]


def _layout(sizes, wss, slots, c=LAT_C, n_images=None, n_slots=None, lats=None, want=True):
    L = _lib.lib()
    n = len(sizes) if n_images is None else n_images
    k = len(slots) if n_slots is None else n_slots
    lats = [_lat(s) for s in sizes] if lats is None else lats
    cslots = (_lib.RaggedRoiSlot * max(len(slots), 1))(*[_lib.RaggedRoiSlot(*s) for s in slots])
    out = (_lib.RaggedCtxRoiMoveSlot * max(len(slots), 1))() if want else None
    totals = (ctypes.c_uint64 * 7)()
    rc = L.sicn_ragged_ctx_roi_move_layout(_u32([w for w, _ in lats]), _u32([h for _, h in lats]), c, _u32(wss) if wss is not None else None,
                                           _u32([w for w, _ in sizes]), _u32([h for _, h in sizes]), n, cslots, k, out, totals)
    return rc, (list(out)[:len(slots)] if want else None), [int(v) for v in totals]


def _coder_workspace(sizes, wss, c=LAT_C):
    lats = [_lat(s) for s in sizes]
    totals = (ctypes.c_uint64 * 3)()
    assert _lib.lib().sicn_ragged_ctx_layout_sl(_u32([w for w, _ in lats]), _u32([h for _, h in lats]), c, _u32(wss), len(sizes), None, totals) == 0
    return int(totals[2])


@pytest.mark.parametrize("wss", [1024, 16384])
def test_layout_equals_plain_arithmetic(wss):
    L = _lib.lib()
    rc, out, totals = _layout(SIZES, [wss] * len(SIZES), SLOTS)
    assert rc == 0
    coder_ws = _coder_workspace(SIZES, [wss] * len(SIZES))
    band = lat = recon = roi = 0
    items = [0, 0]
    for k, ((img, w, h), s) in enumerate(zip(SLOTS, out)):
        lw, lh = _lat(SIZES[img])
        cap2 = (ctypes.c_int32 * 2)()
        assert L.sicn_ragged_roi_move_capacity(4, *SIZES[img], lw, lh, w, h, cap2) == 0
        cw_cap, rh_cap = int(cap2[0]), int(cap2[1])
        _, (m0, m1, rows) = _capacity(lw, lh, LAT_C, wss, rh_cap)
        assert (s.cw_cap, s.rh_cap, s.band_rows_cap, tuple(s.max_streams)) == (cw_cap, rh_cap, rows, (m0, m1))
        assert tuple(s.items) == (-(-m0 // WPB), -(-m1 // WPB)) and tuple(s.first_item) == tuple(items)
        assert (s.band_offset, s.latent_offset, s.recon_offset, s.roi_offset) == (band, lat, recon, roi)
        assert s.meta_offset == coder_ws + 64 * k and band % 16 == 0 and s.meta_offset % 16 == 0
        band += -(-rows * lw * LAT_C // 16) * 16
        lat += rh_cap * cw_cap * LAT_C
        recon += 16 * rh_cap * 16 * cw_cap * 3
        roi += h * w * 3
        items = [items[0] + s.items[0], items[1] + s.items[1]]
    assert totals == [band, lat, recon, roi, coder_ws + 64 * len(SLOTS), items[0], items[1]]
    one = [s for (img, _, _), s in zip(SLOTS, out) if img == 4]
    assert tuple(one[0].max_streams) == (1, 0) and tuple(one[0].items) == (1, 0)      # a 1 x 1 latent: no non-anchor capacity
    whole = out[-1]                                                                   # the whole 160 x 640 image
    assert (whole.cw_cap, whole.rh_cap, whole.band_rows_cap) == (10, 40, 40)
    # several slots of one image: disjoint bands and meta blocks, one item range each
    mine = [s for (img, _, _), s in zip(SLOTS, out) if img == 0]
    assert len(mine) == 3
    spans = sorted((int(s.band_offset), int(s.band_offset) + int(s.band_rows_cap) * 37 * LAT_C) for s in mine)
    assert all(a_end <= b for (_, a_end), (b, _) in zip(spans, spans[1:]))
    assert len({int(s.meta_offset) for s in out}) == len(out)
    assert len({(s.first_item[0], s.first_item[0] + s.items[0]) for s in out}) == len(out)


def test_layout_default_stream_length_and_bands_beyond_4_gib():
    rc, out, t = _layout([(640, 480)], None, [(0, 32, 32)])
    rc2, out2, t2 = _layout([(640, 480)], [16384], [(0, 32, 32)])
    assert rc == 0 == rc2 and t == t2 and tuple(out[0].max_streams) == tuple(out2[0].max_streams)
    # 40 whole-height slots on a 2048 x 16384 x 4 latent: 2^27 band bytes each, 5 GiB in all — arithmetic only
    n_slots = 40
    rc, out, totals = _layout([(2048 * 16, 16384 * 16)], None, [(0, 16, 16384 * 16)] * n_slots, c=4)
    assert rc == 0
    assert (out[-1].cw_cap, out[-1].rh_cap, out[-1].band_rows_cap) == (5, 16384, 16384)
    assert out[-1].band_offset == (n_slots - 1) * 2 ** 27 > 2 ** 32 and totals[0] == n_slots * 2 ** 27
    assert tuple(out[-1].max_streams) == (4096, 4096) and totals[5] == totals[6] == n_slots * 512


def test_layout_refusals():
    sizes, wss = [(112, 144), (100, 131)], [1024, 1024]
    assert _layout(sizes, wss, [(0, 20, 20), (1, 100, 131), (0, 112, 144)])[0] == 0
    for bad in [(0, 0, 20), (0, 20, 0), (0, -1, 20), (0, 20, -1), (0, 113, 20), (0, 20, 145), (1, 101, 20), (1, 20, 132), (2, 20, 20),
                (-1, 20, 20), (INT32_MAX, 20, 20), (0, INT32_MAX, INT32_MAX)]:
        assert _layout(sizes, wss, [bad])[0] == EINVAL, bad
        assert _layout(sizes, wss, [(0, 20, 20), bad])[0] == EINVAL, bad         # ... in any slot
    assert _layout(sizes, wss, [(0, 20, 20)], n_slots=0)[0] == EINVAL and _layout(sizes, wss, [(0, 20, 20)], n_slots=-1)[0] == EINVAL
    assert _layout(sizes, wss, [(0, 20, 20)], n_images=0)[0] == EINVAL
    assert _layout(sizes, [1000, 1024], [(0, 20, 20)])[0] == EINVAL              # the layouts it builds on
    assert _layout(sizes, wss, [(0, 20, 20)], c=0)[0] == EINVAL and _layout(sizes, wss, [(0, 20, 20)], c=190)[0] == EINVAL
    assert _layout([(0, 144), (100, 131)], wss, [(0, 1, 1)], lats=[(7, 9), (7, 9)])[0] == EINVAL      # an image without a size
    assert _layout([(113, 144), (100, 131)], wss, [(0, 1, 1)], lats=[(7, 9), (7, 9)])[0] == EINVAL    # larger than 16 x its latent
    assert _layout([(65536, 131072)], None, [(0, 65536, 131072)], c=4)[0] == EINVAL                   # a reconstruction of 2^31 bytes
    L = _lib.lib()
    one, slot, totals = _u32([7]), (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(0, 1, 1)), (ctypes.c_uint64 * 7)()
    img = _u32([100])
    assert L.sicn_ragged_ctx_roi_move_layout(one, one, 4, None, img, img, 1, slot, 1, None, None) == 0      # both outputs optional
    assert L.sicn_ragged_ctx_roi_move_layout(None, one, 4, None, img, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_layout(one, None, 4, None, img, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_layout(one, one, 4, None, None, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_layout(one, one, 4, None, img, None, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_layout(one, one, 4, None, img, img, 1, None, 1, None, totals) == EINVAL


def test_device_calls_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    dummy = ctypes.c_void_p(64)
    slot = (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(0, 20, 20))
    assert L.sicn_ragged_ctx_roi_move_create(None, slot, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_roi_move_create(dummy, slot, 1, None) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_create(dummy, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_roi_move_create(dummy, slot, 0, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_roi_move_workspace_bytes(None) == 0
    L.sicn_ragged_ctx_roi_move_free(None)
    assert L.sicn_ragged_ctx_roi_move_prepare_async(None, dummy, None, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_decode_async(None, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_ctx_roi_move_cut_async(None, dummy, dummy, None) == EINVAL
    # with objects (where a gfx950 device exists to create them): NULL and misaligned tensors, a short or odd workspace, before any launch
    coder = ctypes.c_void_p()
    rc = L.sicn_ragged_ctx_coder_create_sl(_u32([7]), _u32([9]), LAT_C, _u32([1024]), _u32([112]), _u32([144]), 1, ctypes.byref(coder))
    assert rc in (0, -19)
    if rc == 0:
        mv = ctypes.c_void_p()
        for bad in [(0, 113, 20), (1, 20, 20), (0, 0, 20)]:
            assert L.sicn_ragged_ctx_roi_move_create(coder, (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(*bad)), 1, ctypes.byref(mv)) == EINVAL
            assert not mv.value
        bare = ctypes.c_void_p()                                                 # a coder made without image sizes
        assert L.sicn_ragged_ctx_coder_create_sl(_u32([7]), _u32([9]), LAT_C, _u32([1024]), None, None, 1, ctypes.byref(bare)) == 0
        assert L.sicn_ragged_ctx_roi_move_create(bare, slot, 1, ctypes.byref(mv)) == EINVAL and not mv.value
        L.sicn_ragged_ctx_coder_free(bare)
        assert L.sicn_ragged_ctx_roi_move_create(coder, slot, 1, ctypes.byref(mv)) == 0
        need = L.sicn_ragged_ctx_roi_move_workspace_bytes(mv)
        assert need == L.sicn_ragged_ctx_coder_workspace_bytes(coder) + 64
        call = L.sicn_ragged_ctx_roi_move_decode_async
        ok = [mv, dummy, dummy, dummy, dummy, dummy, dummy, dummy, dummy, need, None]
        for k in range(1, 8):
            args = list(ok)
            args[k] = None
            assert call(*args) == EINVAL, k
        assert call(*ok[:9], need - 1, None) == ENOSPC
        assert call(*ok[:8], None, need, None) == ENOSPC
        assert call(*ok[:8], ctypes.c_void_p(72), need, None) == EINVAL          # a workspace that is not 16-byte aligned
        for k, odd in [(1, 66), (2, 65), (3, 66), (4, 66)]:                     # xy, containers, scales, band
            args = list(ok)
            args[k] = ctypes.c_void_p(odd)
            assert call(*args) == EINVAL, k
        prep = L.sicn_ragged_ctx_roi_move_prepare_async
        assert prep(mv, None, None, dummy, need, None) == EINVAL and prep(mv, ctypes.c_void_p(65), None, dummy, need, None) == EINVAL
        assert prep(mv, dummy, None, dummy, need - 1, None) == ENOSPC and prep(mv, dummy, None, None, need, None) == ENOSPC
        assert prep(mv, dummy, None, ctypes.c_void_p(72), need, None) == EINVAL
        assert L.sicn_ragged_ctx_roi_move_cut_async(mv, None, dummy, None) == EINVAL
        assert L.sicn_ragged_ctx_roi_move_cut_async(mv, dummy, None, None) == EINVAL
        L.sicn_ragged_ctx_roi_move_free(mv)
        L.sicn_ragged_ctx_coder_free(coder)


def test_python_class_refuses_bad_slots_before_anything_is_made():
    from simple_image_compression_network_amd import hyperprior

    class Net:
        sizes = [(112, 144), (100, 131)]

    class Codec:
        main = Net()
        y_coder = None

    for slots, text in [([], "at least one"), ([(0, 20)], "at least one"), ([(2, 20, 20)], "the net has 2 images"),
                        ([(-1, 20, 20)], "the net has 2 images"), ([(0, 113, 20)], "empty or larger"), ([(1, 20, 132)], "empty or larger"),
                        ([(0, 20, 20), (0, 0, 20)], "empty or larger")]:
        with pytest.raises(ValueError, match=text):
            hyperprior.MovingHyperpriorRoi(Codec(), slots)
    assert hyperprior.RaggedHyperpriorCodec.moving_roi is not None and "MovingHyperpriorRoi" in hyperprior.__all__


def test_ctx_roi_move_host_under_the_sanitizers(tmp_path):
    """tests/cpp/ctx_roi_move_plan_check.cpp — the pure-host header csrc/ctx_roi_move_host.hpp with its own main — built with the
    address and undefined-behaviour sanitizers and run as a child process: capacities, placement and layout into heap blocks of
    exactly their length, the rows of every placement replayed on blocks of exactly the layout's sizes, extreme coordinates and
    every refusal."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ctx_roi_move_plan_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ctx_roi_move_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ctx_roi_move_plan_check ok: \d+ checks", r.stdout), r.stdout
