"""CPU-only checks of library 0.8 (include/sicn_ragged_hyper.h): the symbols and the binding table, sicn_ragged_crop_layout against
Python arithmetic, every SICN_EINVAL of the crop and of sicn_ragged_net_create_gdn, and the property RaggedHyperpriorCodec rests on:
hyper_parameters' draws depend on channel counts only.  Nothing here touches a device."""
import ctypes
import re
from pathlib import Path

import numpy as np

from simple_image_compression_network_amd import _lib, hyperprior
from simple_image_compression_network_amd.config import CLayerDesc, eight_layer_descs

ROOT = Path(__file__).resolve().parent.parent
EINVAL = -22


def test_library_exports_every_declared_symbol_of_0_8():
    L = _lib.lib()
    assert L.sicn_version() >= 8
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sicn_ragged_hyper.h").read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))
    assert syms == ["sicn_ragged_crop_create", "sicn_ragged_crop_free", "sicn_ragged_crop_layout", "sicn_ragged_crop_run",
                    "sicn_ragged_net_create_gdn"]
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_HYPER_ABI), "python binding table and sicn_ragged_hyper.h disagree"
    m = re.search(r"#define\s+SICN_RAGGED_CROP_ROWS\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.RAGGED_CROP_ROWS


def _crop_layout(src, dst, channels, image, n_images=None):
    """src, dst: [(h, w)] per image."""
    m = max(len(src), 1)
    i32 = ctypes.c_int32 * m
    sw, sh = i32(*[w for _, w in src]), i32(*[h for h, _ in src])
    dw, dh = i32(*[w for _, w in dst]), i32(*[h for h, _ in dst])
    out = (ctypes.c_int64 * 4)()
    rc = _lib.lib().sicn_ragged_crop_layout(sw, sh, dw, dh, channels, len(src) if n_images is None else n_images, image, out)
    return rc, list(out)


# (src (h, w), dst (h, w)): dst == src, a crop in one dimension only, in both, one-row and one-column images
SHAPES = [((2, 2), (1, 1)), ((16, 16), (16, 16)), ((34, 18), (33, 17)), ((36, 36), (35, 36)), ((36, 100), (36, 99)),
          ((48, 112), (36, 100)), ((70, 132), (70, 131)), ((2, 34), (1, 33)), ((68, 2), (67, 2)), ((1, 1), (1, 1)),
          ((1, 4000), (1, 1)), ((3000, 7), (2999, 1))]


def test_crop_layout_equals_python_arithmetic():
    assert len(SHAPES) == 12
    src, dst = [s for s, _ in SHAPES], [d for _, d in SHAPES]
    for c in (3, 5, 192):
        so = do = 0
        offs = []
        for (sh, sw), (dh, dw) in SHAPES:
            offs.append((so, do))
            so += sh * sw * c
            do += dh * dw * c
        for i in range(len(SHAPES)):
            rc, got = _crop_layout(src, dst, c, i)
            assert rc == 0
            assert got == [offs[i][0], offs[i][1], so, do], (c, i)


def test_crop_layout_offsets_above_4_gib():
    src, dst, c = [(4320, 2048)] * 5, [(4319, 2047)] * 5, 192
    per_src, per_dst = 4320 * 2048 * c, 4319 * 2047 * c
    assert per_src < 2 ** 31 and 3 * per_src > 2 ** 32 and 3 * per_dst > 2 ** 32
    for i in range(5):
        rc, got = _crop_layout(src, dst, c, i)
        assert rc == 0 and got == [i * per_src, i * per_dst, 5 * per_src, 5 * per_dst]


def test_crop_limits_are_einval_without_a_device():
    ok = ([(4, 4), (8, 6)], [(3, 4), (8, 5)])
    assert _crop_layout(*ok, 3, 1)[0] == 0
    assert _crop_layout([], [], 3, 0, n_images=0)[0] == EINVAL                      # n_images < 1
    assert _crop_layout(*ok, 3, 0, n_images=-1)[0] == EINVAL
    assert _crop_layout(*ok, 0, 0)[0] == EINVAL                                     # channels < 1
    assert _crop_layout(*ok, -4, 0)[0] == EINVAL
    for bad in (0, -1):                                                             # a size below 1, in every one of the four arrays
        assert _crop_layout([(4, 4), (bad, 6)], [(3, 4), (bad, 5)], 3, 0)[0] == EINVAL
        assert _crop_layout([(4, 4), (8, bad)], [(3, 4), (8, bad)], 3, 0)[0] == EINVAL
        assert _crop_layout([(4, 4), (8, 6)], [(3, 4), (bad, 5)], 3, 0)[0] == EINVAL
        assert _crop_layout([(4, 4), (8, 6)], [(3, 4), (8, bad)], 3, 0)[0] == EINVAL
    big = (1 << 20) + 1                                                             # a size above 2^20
    assert _crop_layout([(1, 1 << 20)], [(1, 1 << 20)], 1, 0)[0] == 0
    assert _crop_layout([(1, big)], [(1, 1)], 1, 0)[0] == EINVAL
    assert _crop_layout([(big, 1)], [(1, 1)], 1, 0)[0] == EINVAL
    assert _crop_layout([(4, 4), (8, 6)], [(3, 4), (9, 5)], 3, 0)[0] == EINVAL      # dst larger than src, either dimension
    assert _crop_layout([(4, 4), (8, 6)], [(3, 4), (8, 7)], 3, 0)[0] == EINVAL
    # one image's tensor of 2^31 bytes or more: 4096 x 4096 x 128; 4096 x 4095 x 128 is just under
    assert _crop_layout([(4096, 4096)], [(1, 1)], 128, 0)[0] == EINVAL
    assert _crop_layout([(4095, 4096)], [(1, 1)], 128, 0)[0] == 0
    assert _crop_layout([(1 << 20, 1 << 20)], [(1, 1)], 1 << 30, 0)[0] == EINVAL    # the product does not wrap
    # 2^31 - 1 work items or more: images of 2^20 rows hold 2^20 / ROWS items each
    per = (1 << 20) // _lib.RAGGED_CROP_ROWS
    n = -(-(2 ** 31 - 1) // per)
    shapes = [(1 << 20, 1)] * n
    assert _crop_layout(shapes, shapes, 1, 0)[0] == EINVAL
    assert _crop_layout(shapes[:-1], shapes[:-1], 1, n - 2)[0] == 0                 # (n - 1) * per < 2^31 - 1
    assert (n - 1) * per < 2 ** 31 - 1 <= n * per
    assert _crop_layout(*ok, 3, 2)[0] == EINVAL                                     # image out of range
    assert _crop_layout(*ok, 3, -1)[0] == EINVAL
    # creation checks its arguments before it asks for a device; run and free take NULL
    L = _lib.lib()
    out = ctypes.c_void_p()
    one, two = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(2)
    assert L.sicn_ragged_crop_create(one, one, two, one, 3, 1, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_crop_create(one, one, one, one, 0, 1, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_crop_create(one, one, one, one, 3, 0, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_crop_create(None, one, one, one, 3, 1, ctypes.byref(out)) == EINVAL
    assert not out.value
    assert L.sicn_ragged_crop_run(None, None, None, None) == EINVAL
    L.sicn_ragged_crop_free(None)


def _cut_layout_at_the_corner(src, dst, channels, image, n_images=None):
    """sicn_ragged_cut_layout of the rectangles (0, 0, dst_w, dst_h) without source offsets; src, dst: [(h, w)] per image."""
    m = max(len(src), 1)
    i32 = ctypes.c_int32 * m
    sw, sh = i32(*[w for _, w in src]), i32(*[h for h, _ in src])
    rects = (_lib.RaggedRect * m)(*[_lib.RaggedRect(0, 0, w, h) for h, w in dst])
    out = (ctypes.c_int64 * 4)()
    rc = _lib.lib().sicn_ragged_cut_layout(sw, sh, rects, channels, None, len(src) if n_images is None else n_images, image, out)
    return rc, list(out)


def test_crop_layout_is_the_cut_layout_at_the_corner():
    """Destination heights of one row, exactly one work item and two; source rows of 16 c and of 5 c bytes (a multiple of 16 or
    not, for c = 1 and 3); one image and three."""
    r = _lib.RAGGED_CROP_ROWS
    assert r == 8
    for c in (1, 3, 192):
        for sw, dw in ((16, 16), (32, 16), (5, 5), (7, 5)):
            for dh in (1, r, r + 1):
                one = ([(dh + 2, sw)], [(dh, dw)])
                three = ([(dh, sw), (dh + 2, sw + 1), (r + 3, sw)], [(dh, dw), (dh, dw), (r + 1, dw)])
                for src, dst in (one, three):
                    total_src, total_dst = (sum(h * w * c for h, w in s) for s in (src, dst))
                    for i in range(len(src)):
                        crop, cut = _crop_layout(src, dst, c, i), _cut_layout_at_the_corner(src, dst, c, i)
                        assert crop == cut and crop[0] == 0, (c, src, dst, i)
                        assert crop[1][2:] == [total_src, total_dst]
                        assert crop[1][:2] == [sum(h * w * c for h, w in src[:i]), sum(h * w * c for h, w in dst[:i])]
    # what either refuses, both refuse
    for src, dst, c, i, n in [([(4, 4)], [(4, 5)], 3, 0, None), ([(4, 4)], [(5, 4)], 3, 0, None), ([(4, 4)], [(4, 0)], 3, 0, None),
                              ([(4, 4)], [(4, 4)], 0, 0, None), ([(4, 4)], [(4, 4)], 3, 0, 0), ([(4, 4)], [(4, 4)], 3, 1, None)]:
        assert _crop_layout(src, dst, c, i, n)[0] == _cut_layout_at_the_corner(src, dst, c, i, n)[0] == EINVAL


def test_every_refusal_of_crop_layout_is_einval():
    """One case per check of the crop's plan, each with a valid neighbour image in front where the plan looks at every image."""
    ok = [(4, 4)]
    big = (1 << 20) + 1
    assert _crop_layout(ok + [(8, 6)], ok + [(8, 5)], 3, 1)[0] == 0
    assert _crop_layout(ok + [(8, 6)], ok + [(8, 7)], 3, 0)[0] == EINVAL            # dst wider than src
    assert _crop_layout(ok + [(8, 6)], ok + [(9, 6)], 3, 0)[0] == EINVAL            # dst taller than src
    assert _crop_layout(ok + [(8, 6)], ok + [(8, 0)], 3, 0)[0] == EINVAL            # dst_w = 0
    assert _crop_layout(ok + [(8, 6)], ok + [(0, 6)], 3, 0)[0] == EINVAL            # dst_h = 0
    assert _crop_layout(ok + [(1, 1 << 20)], ok + [(1, 1)], 1, 0)[0] == 0
    assert _crop_layout(ok + [(1, big)], ok + [(1, 1)], 1, 0)[0] == EINVAL          # a side above 2^20
    assert _crop_layout(ok + [(big, 1)], ok + [(1, 1)], 1, 0)[0] == EINVAL
    assert _crop_layout(ok + [(1 << 15, 1 << 16)], ok + [(1, 1)], 1, 0)[0] == EINVAL            # an image of 2^31 bytes
    assert _crop_layout(ok + [((1 << 15) - 1, 1 << 16)], ok + [(1, 1)], 1, 0)[0] == 0
    assert _crop_layout(ok, ok, 0, 0)[0] == EINVAL                                  # channels = 0
    assert _crop_layout(ok, ok, 3, 0, n_images=0)[0] == EINVAL                      # n_images = 0
    assert _crop_layout(ok, ok, 3, 1)[0] == EINVAL and _crop_layout(ok, ok, 3, -1)[0] == EINVAL   # image index out of range
    L = _lib.lib()
    one, out = (ctypes.c_int32 * 1)(4), (ctypes.c_int64 * 4)()
    assert L.sicn_ragged_crop_layout(one, one, one, one, 3, 1, 0, out) == 0
    for null in range(4):                                                           # NULL arrays
        arrays = [None if k == null else one for k in range(4)]
        assert L.sicn_ragged_crop_layout(*arrays, 3, 1, 0, out) == EINVAL
    assert L.sicn_ragged_crop_layout(one, one, one, one, 3, 1, 0, None) == EINVAL
    handle = ctypes.c_void_p(1)
    assert L.sicn_ragged_crop_create(one, one, None, one, 3, 1, ctypes.byref(handle)) == EINVAL and not handle.value
    assert L.sicn_ragged_crop_create(one, one, one, one, 3, 1, None) == EINVAL


def test_net_create_gdn_with_a_null_array_rejects_what_net_create_rejects():
    L = _lib.lib()
    descs = eight_layer_descs(768, 512)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in descs])
    one, zero = (ctypes.c_int32 * 1)(16), (ctypes.c_int32 * 1)(0)
    handles = (ctypes.c_void_p * 8)()
    cases = [(cd, handles, 8, one, one, 0), (cd, handles, 8, zero, one, 1), (cd, handles, 8, one, one, 1), (cd, None, 8, one, one, 1),
             (cd, handles, 0, one, one, 1), (None, handles, 8, one, one, 1), (cd, handles, 8, None, one, 1)]
    for d, w, n, ws, hs, n_img in cases:
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        rc = L.sicn_ragged_net_create(d, w, n, ws, hs, n_img, ctypes.byref(a))
        assert rc == EINVAL
        assert L.sicn_ragged_net_create_gdn(d, w, None, n, ws, hs, n_img, ctypes.byref(b)) == rc
        assert L.sicn_ragged_net_create_gdn(d, w, (ctypes.c_void_p * 8)(), n, ws, hs, n_img, ctypes.byref(b)) == rc   # all-NULL entries
        assert not a.value and not b.value
    assert L.sicn_ragged_net_create_gdn(cd, handles, None, 8, one, one, 1, None) == EINVAL


def test_hyper_parameters_depend_on_channel_counts_only():
    """RaggedHyperpriorCodec draws once, for sizes[0], and every image must get what HyperpriorCodec(w_i, h_i, 1, seed) gets."""
    a, b = hyperprior.hyper_parameters(96, 64, 7), hyperprior.hyper_parameters(100, 36, 7)
    assert [g is None for g in a["gdn_np"]] == [g is None for g in b["gdn_np"]] == [False, False, False, True, False, False, False, True]
    for ga, gb in zip(a["gdn_np"], b["gdn_np"]):
        if ga is not None:
            assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]) and ga[2:] == gb[2:]
    for key in ("ha_np", "hs_np"):
        assert len(a[key]) == len(b[key]) == 2
        for (wa, ba), (wb, bb) in zip(a[key], b[key]):
            assert np.array_equal(wa, wb) and np.array_equal(ba, bb)
    for key in ("pa", "ps"):
        for (wa, ba), (wb, bb) in zip(a[key], b[key]):
            assert np.array_equal(wa.m_weights, wb.m_weights) and np.array_equal(ba.m_weights, bb.m_weights)
