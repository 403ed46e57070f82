"""CPU-only checks of the moving ROI decode's host side (include/sicn_ragged_roi_move.h): the symbols and the binding table; the
placement rule by brute force against sicn_ragged_roi_plan — the placed window contains the planned one, lies inside the latent and
has exactly the capacity; its sufficiency on the oracle's closed form of layers 4-7 — the reconstruction of the PLACED window, cut
at (x, y), is that rectangle of the full reconstruction; the clamp and its flag; the layout against plain Python arithmetic; every
refusal; the argument checks of the device calls that come before a device is asked for; and the pure-host header under the host
sanitizers.  Nothing here touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import sicn_ref
from simple_image_compression_network_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENOSPC = -22, -28
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
LAT_C = 192
SIZES = [(112, 144), (100, 131), (16, 16), (256, 48), (64, 400)]           # (width, height)


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _lat(size):
    return -(-size[0] // 16), -(-size[1] // 16)


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_roi_move.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_moving_roi_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == sorted(["sicn_ragged_roi_move_capacity", "sicn_ragged_roi_move_place", "sicn_ragged_roi_move_layout",
                           "sicn_ragged_roi_move_create", "sicn_ragged_roi_move_free", "sicn_ragged_roi_move_workspace_bytes",
                           "sicn_ragged_roi_move_decode_async", "sicn_ragged_roi_move_cut_async"])
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_ROI_MOVE_ABI), "python binding table and sicn_ragged_roi_move.h disagree"
    for other in (_lib.RAGGED_ABI, _lib.RAGGED_HYPER_ABI, _lib.RAGGED_CODEC_ABI, _lib.RAGGED_ARCHIVE_ABI, _lib.RAGGED_WINDOW_ABI,
                  _lib.RAGGED_CTX_WINDOW_ABI, _lib.RAGGED_RGB_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() == 17


# ---- capacity and placement -------------------------------------------------------------------------------------------------------
def _capacity(size, w, h, lat=None, layers=4):
    lw, lh = _lat(size) if lat is None else lat
    cap = (ctypes.c_int32 * 2)()
    rc = _lib.lib().sicn_ragged_roi_move_capacity(layers, size[0], size[1], lw, lh, w, h, cap)
    return rc, (int(cap[0]), int(cap[1]))


def _place(size, w, h, x0, y0, lat=None, layers=4):
    lw, lh = _lat(size) if lat is None else lat
    p = _lib.RaggedRoiPlaced()
    rc = _lib.lib().sicn_ragged_roi_move_place(layers, size[0], size[1], lw, lh, w, h, x0, y0, ctypes.byref(p))
    return rc, p


def _plan(size, rect):
    lw, lh = _lat(size)
    r, out = _lib.RaggedRect(*rect), _lib.RaggedRoiPlan()
    assert _lib.lib().sicn_ragged_roi_plan(4, size[0], size[1], lw, lh, ctypes.byref(r), ctypes.byref(out)) == 0
    return out


def _positions(last):
    """Every position near both edges — all 16 phases twice over — and a stride of 7, which meets every phase, between them."""
    return sorted(set(range(0, min(last, 40) + 1)) | set(range(max(last - 40, 0), last + 1)) | set(range(0, last + 1, 7)))


def _python_capacity(image, lat, length):
    best = max(-(-(p + length + 30) // 16) - (p - 15) // 16 for p in range(min(image - length, 15) + 1))
    return min(best, lat)


@pytest.mark.parametrize("size", SIZES)
def test_placement_by_brute_force(size):
    W, H = size
    lw, lh = _lat(size)
    placed = 0
    for w, h in [(1, 1), (15, 15), (16, 16), (17, 17), (33, 33), (W, H), (33, 1), (1, 33), (W, 16), (15, H)]:
        if w > W or h > H:
            continue
        rc, (cw_cap, rh_cap) = _capacity(size, w, h)
        assert rc == 0
        assert cw_cap <= (w + 75) // 16 and rh_cap <= (h + 75) // 16, "a capacity above the bound"
        assert (cw_cap, rh_cap) == (_python_capacity(W, lw, w), _python_capacity(H, lh, h))
        widest = tallest = 0
        for x0 in _positions(W - w):
            for y0 in _positions(H - h) if x0 in (0, W - w) or x0 % 16 == 5 else (0, H - h):
                rc, p = _place(size, w, h, x0, y0)
                plan = _plan(size, (x0, y0, w, h))
                assert rc == 0 and p.flags == 0 and (p.x0, p.y0) == (x0, y0)
                assert (p.cw, p.rh) == (cw_cap, rh_cap), "the placed window's size is the capacity"
                assert 0 <= p.c0 and p.c0 + p.cw <= lw and 0 <= p.r0 and p.r0 + p.rh <= lh, "inside the latent"
                assert p.c0 <= plan.c0 and plan.c0 + plan.cw <= p.c0 + p.cw, "contains the planned columns"
                assert p.r0 <= plan.r0 and plan.r0 + plan.rh <= p.r0 + p.rh, "contains the planned rows"
                assert p.c0 == min(plan.c0, lw - cw_cap) and p.r0 == min(plan.r0, lh - rh_cap)
                # the planned window's edges on the latent's edges stay there: the zero padding is the image's own
                assert (plan.c0 > 0 or p.c0 == 0) and (plan.c0 + plan.cw < lw or p.c0 + p.cw == lw)
                assert (plan.r0 > 0 or p.r0 == 0) and (plan.r0 + plan.rh < lh or p.r0 + p.rh == lh)
                assert (p.x, p.y) == (x0 - 16 * p.c0, y0 - 16 * p.r0)
                assert 0 <= p.x and p.x + w <= 16 * p.cw and 0 <= p.y and p.y + h <= 16 * p.rh
                widest, tallest = max(widest, plan.cw), max(tallest, plan.rh)
                placed += 1
        assert widest <= cw_cap and tallest <= rh_cap
        if lw >= (w + 75) // 16 and W - w >= 15:
            assert widest == cw_cap == (w + 75) // 16, "some position needs the whole capacity"
    assert placed > (500 if min(W, H) > 16 else 50)                             # the 16 x 16 image has few positions


@pytest.fixture(scope="module")
def synthesis():
    lat_h, lat_w = 9, 11                                            # the latent of a 176 x 144 image
    params = sicn_ref.load_param_fixture(ROOT / "tests" / "golden" / "param_weights.npz")[4:]
    latent = np.random.default_rng(12).integers(0, 128, (lat_h, lat_w, LAT_C), dtype=np.uint8)

    def synth(x):
        for w, b, _ in params:
            x = sicn_ref.deconv522_ref(x, w, b)
        return x

    full = synth(latent)
    assert full.shape == (16 * lat_h, 16 * lat_w, 3)
    full.setflags(write=False)
    return latent, synth, full


def test_the_placed_window_reconstructs_the_rectangle(synthesis):
    latent, synth, full = synthesis
    size = W, H = 176, 144
    cases = []
    for w, h in [(1, 1), (15, 15), (16, 16), (17, 17), (33, 33), (W, H)]:
        xs, ys = sorted({0, W - w, min(70, W - w)}), sorted({0, H - h, min(50, H - h)})
        cases += [(w, h, x0, y0) for x0 in xs for y0 in ys]                    # corners, edges, one interior position
    for off in (15, 16, 17, 31, 32):                                           # one pixel, around where a window's first column moves
        cases += [(1, 1, off, 40), (1, 1, 50, off), (1, 1, off, off), (1, 1, W - 1 - off, H - 1 - off)]
    assert len(cases) >= 60
    cache = {}
    moved = 0
    for w, h, x0, y0 in cases:
        rc, p = _place(size, w, h, x0, y0)
        assert rc == 0 and p.flags == 0
        plan = _plan(size, (x0, y0, w, h))
        moved += (p.c0, p.r0, p.cw, p.rh) != (plan.c0, plan.r0, plan.cw, plan.rh)
        key = (p.c0, p.r0, p.cw, p.rh)
        if key not in cache:
            cache[key] = synth(latent[p.r0:p.r0 + p.rh, p.c0:p.c0 + p.cw])
        got = cache[key][p.y:p.y + h, p.x:p.x + w]
        assert np.array_equal(got, full[y0:y0 + h, x0:x0 + w]), (w, h, x0, y0)
    assert moved >= 10, "the cases must include windows the placement enlarged or shifted"


@pytest.mark.parametrize("size", SIZES)
def test_positions_outside_the_image_are_clamped_and_flagged(size):
    W, H = size
    for w, h in [(1, 1), (16, 16), (W, H), (W, 1), (7, H)]:
        for x0, y0 in [(-1, 0), (0, -1), (-5, -7), (W - w + 1, 0), (0, H - h + 1), (W, H), (INT32_MIN, 3), (3, INT32_MIN),
                       (INT32_MAX, 3), (3, INT32_MAX), (INT32_MIN, INT32_MAX), (INT32_MAX, INT32_MIN), (INT32_MAX, INT32_MAX)]:
            cx, cy = min(max(x0, 0), W - w), min(max(y0, 0), H - h)
            if (cx, cy) == (x0, y0):
                continue                                                       # (W, 1) at y0 = 3 and the like: a valid position
            rc, p = _place(size, w, h, x0, y0)
            rc2, q = _place(size, w, h, cx, cy)
            assert rc == 0 and rc2 == 0
            assert p.flags == _lib.ROI_MOVE_CLAMPED == 1 and q.flags == 0
            assert (p.x0, p.y0, p.c0, p.r0, p.cw, p.rh, p.x, p.y) == (cx, cy, q.c0, q.r0, q.cw, q.rh, q.x, q.y)
        for x0, y0 in [(0, 0), (W - w, H - h), (W - w, 0), (0, H - h), ((W - w) // 2, (H - h) // 2)]:
            assert _place(size, w, h, x0, y0)[1].flags == 0


def test_capacity_and_placement_refusals():
    size = (112, 144)
    assert _capacity(size, 20, 20) == (0, (5, 5))
    for w, h in [(0, 20), (20, 0), (-1, 20), (20, -1), (113, 20), (20, 145), (INT32_MAX, INT32_MAX), (INT32_MIN, 1)]:
        assert _capacity(size, w, h)[0] == EINVAL, (w, h)
        assert _place(size, w, h, 0, 0)[0] == EINVAL, (w, h)
    assert _capacity((100, 131), 100, 131)[0] == 0 and _capacity((100, 131), 101, 131)[0] == EINVAL      # held to the IMAGE
    assert _capacity((113, 144), 20, 20, lat=(7, 9))[0] == EINVAL                  # an image larger than its latent reconstructs
    assert _capacity((0, 144), 1, 1, lat=(7, 9))[0] == EINVAL and _capacity(size, 1, 1, lat=(0, 9))[0] == EINVAL
    assert _capacity(size, 1, 1, layers=0)[0] == EINVAL and _capacity(size, 1, 1, layers=13)[0] == EINVAL
    L = _lib.lib()
    assert L.sicn_ragged_roi_move_capacity(4, 112, 144, 7, 9, 1, 1, None) == EINVAL
    assert L.sicn_ragged_roi_move_place(4, 112, 144, 7, 9, 1, 1, 0, 0, None) == EINVAL
    # other layer counts follow the plan's margins
    for layers in (1, 2, 3, 5):
        s = 1 << layers
        rc, p = _place((20 * s, 20 * s), 7, 9, 10 * s, 10 * s, lat=(20, 20), layers=layers)
        assert rc == 0 and p.c0 <= (10 * s - (s - 1)) // s and p.c0 + p.cw >= -(-(10 * s + 7 + 2 * (s - 1)) // s)


# ---- the layout -------------------------------------------------------------------------------------------------------------------
def _layout(sizes, wss, slots, c=LAT_C, n_images=None, n_slots=None, lats=None, want=True):
    L = _lib.lib()
    n = len(sizes) if n_images is None else n_images
    k = len(slots) if n_slots is None else n_slots
    lats = [_lat(s) for s in sizes] if lats is None else lats
    cslots = (_lib.RaggedRoiSlot * max(len(slots), 1))(*[_lib.RaggedRoiSlot(*s) for s in slots])
    out = (_lib.RaggedRoiMoveSlot * max(len(slots), 1))() if want else None
    totals = (ctypes.c_uint64 * 6)()
    rc = L.sicn_ragged_roi_move_layout(_u32([w for w, _ in lats]), _u32([h for _, h in lats]), c, _u32(wss) if wss is not None else None,
                                       _u32([w for w, _ in sizes]), _u32([h for _, h in sizes]), n, cslots, k, out, totals)
    return rc, (list(out)[:len(slots)] if want else None), [int(v) for v in totals]


def _coder_blocks(sizes, wss, c=LAT_C):
    """The bytes of every image's workspace block in the full coder."""
    n = len(sizes)
    lats = [_lat(s) for s in sizes]
    images = (_lib.RaggedCodecImage * n)()
    totals = (ctypes.c_uint64 * 3)()
    assert _lib.lib().sicn_ragged_codec_layout(_u32([w for w, _ in lats]), _u32([h for _, h in lats]), c, _u32(wss), n, images, totals) == 0
    offs = [int(im.workspace_offset) for im in images] + [int(totals[2])]
    return [b - a for a, b in zip(offs, offs[1:])]


SLOTS = [(0, 20, 20), (4, 64, 33), (0, 1, 1), (3, 256, 48), (2, 16, 16), (1, 100, 15), (0, 112, 1), (4, 17, 400), (0, 20, 20), (1, 33, 15)]


@pytest.mark.parametrize("wss", [1024, 16384])
def test_layout_equals_plain_arithmetic(wss):
    rc, out, totals = _layout(SIZES, [wss] * len(SIZES), SLOTS)
    assert rc == 0
    blocks = _coder_blocks(SIZES, [wss] * len(SIZES))
    band = lat = recon = roi = ws = items = 0
    for (img, w, h), s in zip(SLOTS, out):
        lw, lh = _lat(SIZES[img])
        _, (cw_cap, rh_cap) = _capacity(SIZES[img], w, h)
        R, n = lw * LAT_C, lw * lh * LAT_C
        max_streams = min(-(-n // wss), -(-rh_cap * R // wss) + 1)
        assert (s.cw_cap, s.rh_cap, s.max_streams, s.first_item) == (cw_cap, rh_cap, max_streams, items)
        assert (s.band_offset, s.latent_offset, s.recon_offset, s.roi_offset, s.workspace_offset) == (band, lat, recon, roi, ws)
        assert band % 16 == 0 and ws % 16 == 0
        band += -(-max_streams * wss // 16) * 16
        lat += rh_cap * cw_cap * LAT_C
        recon += 16 * rh_cap * 16 * cw_cap * 3
        roi += h * w * 3
        ws += blocks[img]
        items += max_streams
    assert totals == [band, lat, recon, roi, ws, items]
    if wss == 1024:
        assert [-(-_lat(s)[0] * _lat(s)[1] * LAT_C // wss) for s in SIZES] == [12, 12, 1, 9, 19]
        assert out[0].max_streams == 8                                          # a 20 x 20 slot of 112 x 144: at most 8 of 12 streams
    else:
        streams = [1, 1, 1, 1, 2]
        assert all(s.max_streams == streams[img] for (img, _, _), s in zip(SLOTS, out))     # every band is the whole image
    # several slots of one image: disjoint bands and workspace blocks
    mine = [s for (img, _, _), s in zip(SLOTS, out) if img == 0]
    assert len(mine) == 4
    spans = sorted((int(s.band_offset), int(s.band_offset) + int(s.max_streams) * wss) for s in mine)
    assert all(a_end <= b for (_, a_end), (b, _) in zip(spans, spans[1:]))
    blocks0 = sorted((int(s.workspace_offset), int(s.workspace_offset) + blocks[0]) for s in mine)
    assert all(a_end <= b for (_, a_end), (b, _) in zip(blocks0, blocks0[1:]))


def test_layout_default_stream_length_and_64_bit_offsets():
    rc, out, _ = _layout([(640, 480)], None, [(0, 32, 32)])
    rc2, out2, _ = _layout([(640, 480)], [16384], [(0, 32, 32)])
    assert rc == 0 == rc2 and out[0].max_streams == out2[0].max_streams == min(-(-40 * 30 * LAT_C // 16384), -(-6 * 40 * LAT_C // 16384) + 1)
    # 140 slots of 2^25 band bytes each on one image of 2^25 symbols: 4.7 G band bytes — arithmetic only
    n_slots = 140
    rc, out, totals = _layout([(65536, 131072)], None, [(0, 16, 131072)] * n_slots, c=1)
    assert rc == 0
    assert (out[-1].cw_cap, out[-1].rh_cap, out[-1].max_streams) == (5, 8192, 2048)
    assert out[-1].band_offset == (n_slots - 1) * 2 ** 25 > 2 ** 32 and totals[0] == n_slots * 2 ** 25
    assert totals[5] == n_slots * 2048


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
    assert _layout(sizes, wss, [(0, 20, 20)], c=0)[0] == EINVAL
    assert _layout([(0, 144), (100, 131)], wss, [(0, 1, 1)], lats=[(7, 9), (7, 9)])[0] == EINVAL      # an image without a size
    assert _layout([(113, 144), (100, 131)], wss, [(0, 1, 1)], lats=[(7, 9), (7, 9)])[0] == EINVAL    # larger than 16 x its latent
    assert _layout([(2049 * 16, 1024 * 16)], [1024], [(0, 20, 20)], c=1)[0] == EINVAL                 # more than 2048 streams
    assert _layout([(65536, 131072)], None, [(0, 65536, 131072)], c=1)[0] == EINVAL                   # a reconstruction of 2^31 bytes
    L = _lib.lib()
    one, slot, totals = _u32([7]), (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(0, 1, 1)), (ctypes.c_uint64 * 6)()
    img = _u32([100])
    assert L.sicn_ragged_roi_move_layout(one, one, 4, None, img, img, 1, slot, 1, None, None) == 0      # both outputs optional
    assert L.sicn_ragged_roi_move_layout(None, one, 4, None, img, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_roi_move_layout(one, None, 4, None, img, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_roi_move_layout(one, one, 4, None, None, img, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_roi_move_layout(one, one, 4, None, img, None, 1, slot, 1, None, totals) == EINVAL
    assert L.sicn_ragged_roi_move_layout(one, one, 4, None, img, img, 1, None, 1, None, totals) == EINVAL


def test_device_calls_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    dummy = ctypes.c_void_p(64)
    slot = (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(0, 20, 20))
    assert L.sicn_ragged_roi_move_create(None, slot, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_roi_move_create(dummy, slot, 1, None) == EINVAL
    assert L.sicn_ragged_roi_move_create(dummy, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_roi_move_create(dummy, slot, 0, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_roi_move_workspace_bytes(None) == 0
    L.sicn_ragged_roi_move_free(None)
    assert L.sicn_ragged_roi_move_decode_async(None, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_roi_move_cut_async(None, dummy, dummy, None) == EINVAL
    # with objects (where a gfx950 device exists to create them): NULL tensors and a short or odd workspace, before any launch
    coder = ctypes.c_void_p()
    rc = L.sicn_ragged_coder_create(_u32([7]), _u32([9]), LAT_C, _u32([1024]), _u32([112]), _u32([144]), 1, ctypes.byref(coder))
    assert rc in (0, -19)
    if rc == 0:
        mv = ctypes.c_void_p()
        for bad in [(0, 113, 20), (1, 20, 20), (0, 0, 20)]:
            assert L.sicn_ragged_roi_move_create(coder, (_lib.RaggedRoiSlot * 1)(_lib.RaggedRoiSlot(*bad)), 1, ctypes.byref(mv)) == EINVAL
            assert not mv.value
        bare = ctypes.c_void_p()                                                 # a coder made without image sizes
        assert L.sicn_ragged_coder_create(_u32([7]), _u32([9]), LAT_C, _u32([1024]), None, None, 1, ctypes.byref(bare)) == 0
        assert L.sicn_ragged_roi_move_create(bare, slot, 1, ctypes.byref(mv)) == EINVAL and not mv.value
        L.sicn_ragged_coder_free(bare)
        assert L.sicn_ragged_roi_move_create(coder, slot, 1, ctypes.byref(mv)) == 0
        need = L.sicn_ragged_roi_move_workspace_bytes(mv)
        assert need == L.sicn_ragged_coder_workspace_bytes(coder) > 0
        call = L.sicn_ragged_roi_move_decode_async
        ok = [mv, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, need, None]
        for k in (1, 2, 4, 5, 6, 7):
            args = list(ok)
            args[k] = None
            assert call(*args) == EINVAL, k
        assert call(*ok[:9], need - 1, None) == ENOSPC
        assert call(*ok[:8], None, need, None) == ENOSPC
        assert call(*ok[:8], ctypes.c_void_p(72), need, None) == EINVAL
        assert call(mv, ctypes.c_void_p(66), *ok[2:]) == EINVAL
        assert L.sicn_ragged_roi_move_cut_async(mv, None, dummy, None) == EINVAL
        assert L.sicn_ragged_roi_move_cut_async(mv, dummy, None, None) == EINVAL
        L.sicn_ragged_roi_move_free(mv)
        L.sicn_ragged_coder_free(coder)


def test_an_object_collected_during_a_stream_capture_is_freed_after_it(monkeypatch):
    """A library object whose last reference goes while a stream capture is under way — the garbage collector may run at any
    allocation — must not reach hipFree inside the capture: its free waits for the next one outside."""
    freed = []

    class FakeLib:
        def fake_free(self, h):
            freed.append(h)

    class Thing(_lib.Handle):
        _free = "fake_free"

        def __init__(self, h):
            self._h = h

    monkeypatch.setattr(_lib, "_lib", FakeLib())
    monkeypatch.setattr(_lib, "_deferred", [])
    monkeypatch.setattr(_lib, "_capturing", lambda: True)
    a, b = Thing(11), Thing(12)
    del a, b
    assert freed == [] and sorted(h for _, h in _lib._deferred) == [11, 12]
    monkeypatch.setattr(_lib, "_capturing", lambda: False)
    c = Thing(13)
    del c
    assert sorted(freed) == [11, 12, 13] and freed[-1] == 13 and _lib._deferred == []
    assert _lib._capturing.__call__() is False


def test_python_class_refuses_bad_slots_before_anything_is_made():
    """The seven cases of test_ragged_ctx_roi_move.py's test of the same name, against api.MovingRoi: the base class of the two
    states these checks once, and a stub net that has nothing but its sizes shows that nothing else was asked of it."""
    from simple_image_compression_network_amd import api

    class Net:
        sizes = [(112, 144), (100, 131)]

    for slots, text in [([], "at least one"), ([(0, 20)], "at least one"), ([(2, 20, 20)], "the net has 2 images"),
                        ([(-1, 20, 20)], "the net has 2 images"), ([(0, 113, 20)], "empty or larger"), ([(1, 20, 132)], "empty or larger"),
                        ([(0, 20, 20), (0, 0, 20)], "empty or larger")]:
        with pytest.raises(ValueError, match=text):
            api.MovingRoi(Net(), slots)


def test_roi_move_host_under_the_sanitizers(tmp_path):
    """tests/cpp/roi_move_plan_check.cpp — the pure-host header csrc/roi_move_host.hpp with its own main — built with the address and
    undefined-behaviour sanitizers and run as a child process: placement and layout into heap blocks of exactly their length, the
    rows of every placement replayed on blocks of exactly the layout's sizes, extreme coordinates and every refusal."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "roi_move_plan_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "roi_move_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"roi_move_plan_check ok: \d+ checks", r.stdout), r.stdout
