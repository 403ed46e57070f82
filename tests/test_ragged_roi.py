"""CPU-only checks of the ROI decode's host side (include/sicn_ragged_window.h): the symbols and the binding table;
sicn_ragged_roi_plan against brute force on the oracle's closed form of layers 4-7 — a rectangle of the window's synthesis IS that
rectangle of the full synthesis, and a margin one smaller is not enough; the window layout and the cut layout against plain Python
arithmetic; every refusal; and the argument checks of the device calls that come before a device is asked for.  Nothing here
touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import sicn_ref
from simple_image_compression_network_amd import _lib, api

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENOSPC = -22, -28
LAT_C = 192
LAT_H, LAT_W = 9, 11                       # the latent of a 176 x 144 image
IMG_W, IMG_H = 16 * LAT_W, 16 * LAT_H


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _i32(values):
    return np.ascontiguousarray(values, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_window.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_window_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == sorted(["sicn_ragged_roi_plan", "sicn_ragged_window_layout", "sicn_ragged_window_create", "sicn_ragged_window_free",
                           "sicn_ragged_window_workspace_bytes", "sicn_ragged_window_decode_async", "sicn_ragged_cut_layout",
                           "sicn_ragged_cut_create", "sicn_ragged_cut_free", "sicn_ragged_cut_run"])
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_WINDOW_ABI), "python binding table and sicn_ragged_window.h disagree"
    for other in (_lib.RAGGED_ABI, _lib.RAGGED_HYPER_ABI, _lib.RAGGED_CODEC_ABI, _lib.RAGGED_ARCHIVE_ABI, _lib.RAGGED_ARCHIVE_SELECT_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() >= 12


# ---- the plan against the oracle ------------------------------------------------------------------------------------------------
def _plan(rect, size=(IMG_W, IMG_H), lat=(LAT_W, LAT_H), layers=4):
    r = _lib.RaggedRect(*rect)
    out = _lib.RaggedRoiPlan()
    rc = _lib.lib().sicn_ragged_roi_plan(layers, size[0], size[1], lat[0], lat[1], ctypes.byref(r), ctypes.byref(out))
    return rc, out


def _python_window(p0, length, lat, lo=15, hi=30):
    """One axis, the issue's closed form with the margins as parameters."""
    a = max(0, (p0 - lo) // 16)
    b = min(lat, -(-(p0 + length + hi) // 16))
    return a, b - a


@pytest.fixture(scope="module")
def synthesis():
    params = sicn_ref.load_param_fixture(ROOT / "tests" / "golden" / "param_weights.npz")[4:]
    latent = np.random.default_rng(12).integers(0, 128, (LAT_H, LAT_W, LAT_C), dtype=np.uint8)

    def synth(x):
        for w, b, _ in params:
            x = sicn_ref.deconv522_ref(x, w, b)
        return x

    full = synth(latent)
    assert full.shape == (IMG_H, IMG_W, 3)
    full.setflags(write=False)
    return latent, synth, full


def _rectangles():
    rects = [(0, 0, IMG_W, IMG_H), (0, 0, 1, 1), (IMG_W - 1, IMG_H - 1, 1, 1), (IMG_W - 1, 0, 1, 1), (0, IMG_H - 1, 1, 1)]
    for off in (15, 16, 17, 31, 32):                               # one pixel, around where a window's first column moves
        rects += [(off, 40, 1, 1), (50, off, 1, 1), (off, off, 1, 1)]
    for off in (1, 2, 3, 18, 19, 34):                              # ... and around where its last column moves
        rects += [(off, 70, 1, 1), (90, off, 1, 1)]
    rects += [(0, 60, IMG_W, 5), (70, 0, 3, IMG_H), (40, 50, 64, 48), (33, 17, 95, 100), (100, 100, 76, 44), (0, 0, 31, 31),
              (145, 113, 31, 31), (16, 16, 16, 16), (63, 63, 2, 2), (64, 64, 1, 1)]
    rng = np.random.default_rng(5)
    for _ in range(4):
        x0, y0 = int(rng.integers(0, IMG_W)), int(rng.integers(0, IMG_H))
        rects.append((x0, y0, int(rng.integers(1, IMG_W - x0 + 1)), int(rng.integers(1, IMG_H - y0 + 1))))
    return rects


def test_plan_is_the_closed_form_and_the_window_reconstructs_the_rectangle(synthesis):
    latent, synth, full = synthesis
    rects = _rectangles()
    assert len(rects) >= 40
    cache = {}
    for rect in rects:
        x0, y0, w, h = rect
        rc, p = _plan(rect)
        assert rc == 0, rect
        assert (p.margin_lo, p.margin_hi) == (15, 30)
        assert (p.c0, p.cw) == _python_window(x0, w, LAT_W) and (p.r0, p.rh) == _python_window(y0, h, LAT_H), rect
        assert (p.x, p.y) == (x0 - 16 * p.c0, y0 - 16 * p.r0), rect
        assert api.roi_plan((IMG_W, IMG_H), rect) == {k: getattr(p, k) for k, _ in _lib.RaggedRoiPlan._fields_}
        key = (p.c0, p.r0, p.cw, p.rh)
        if key not in cache:
            cache[key] = synth(latent[p.r0:p.r0 + p.rh, p.c0:p.c0 + p.cw])
        got = cache[key][p.y:p.y + h, p.x:p.x + w]
        assert np.array_equal(got, full[y0:y0 + h, x0:x0 + w]), rect
    whole = _plan((0, 0, IMG_W, IMG_H))[1]
    assert (whole.c0, whole.r0, whole.cw, whole.rh) == (0, 0, LAT_W, LAT_H)


@pytest.mark.parametrize("lo,hi", [(14, 30), (15, 29)])
def test_a_margin_one_smaller_loses_pixels(synthesis, lo, hi):
    """With 14 or 29 in place of 15 or 30 some one-pixel column of the window's synthesis differs from the full one: the halo is
    tight, and the test above cannot pass on a generous one by accident of the data.  Only the columns whose window changes with the
    smaller margin can differ; there are about eleven for either margin."""
    latent, synth, full = synthesis
    differing = changed = 0
    for x0 in range(IMG_W):
        c0, cw = _python_window(x0, 1, LAT_W, lo, hi)
        if (c0, cw) == _python_window(x0, 1, LAT_W):
            continue
        changed += 1
        col = synth(latent[:, c0:c0 + cw])[:, x0 - 16 * c0]
        differing += not np.array_equal(col, full[:, x0])
    assert changed >= 9
    assert differing >= 1


def test_margins_come_from_the_layer_count():
    for layers, (lo, hi) in {1: (1, 2), 2: (3, 6), 3: (7, 14), 4: (15, 30), 5: (31, 62)}.items():
        s = 1 << layers
        at = 10 * s
        rc, p = _plan((at, at, 7, 9), size=(s * 20, s * 20), lat=(20, 20), layers=layers)
        assert rc == 0 and (p.margin_lo, p.margin_hi) == (lo, hi)
        assert p.c0 == max(0, (at - lo) // s) and p.c0 + p.cw == min(20, -(-(at + 7 + hi) // s))
        assert p.r0 == max(0, (at - lo) // s) and p.r0 + p.rh == min(20, -(-(at + 9 + hi) // s))
        assert (p.x, p.y) == (at - s * p.c0, at - s * p.r0)


def test_plan_refusals():
    ok = (10, 10, 5, 5)
    assert _plan(ok)[0] == 0
    for rect in [(10, 10, 0, 5), (10, 10, 5, 0), (10, 10, -1, 5), (-1, 10, 5, 5), (10, -1, 5, 5), (IMG_W, 0, 1, 1), (0, IMG_H, 1, 1),
                 (IMG_W - 4, 0, 5, 1), (0, IMG_H - 4, 1, 5), (0, 0, IMG_W + 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)]:
        assert _plan(rect)[0] == EINVAL, rect
        with pytest.raises(ValueError):
            api.roi_plan((IMG_W, IMG_H), rect)
    # a cropped image: the rectangle is held to the IMAGE, not to the reconstruction
    assert _plan((99, 130, 1, 1), size=(100, 131), lat=(7, 9))[0] == 0
    assert _plan((99, 130, 2, 1), size=(100, 131), lat=(7, 9))[0] == EINVAL
    assert _plan(ok, layers=0)[0] == EINVAL and _plan(ok, layers=13)[0] == EINVAL
    assert _plan(ok, size=(0, IMG_H))[0] == EINVAL and _plan(ok, lat=(0, LAT_H))[0] == EINVAL
    assert _plan(ok, size=(IMG_W + 1, IMG_H))[0] == EINVAL         # an image larger than its latent reconstructs
    L = _lib.lib()
    r, out = _lib.RaggedRect(*ok), _lib.RaggedRoiPlan()
    assert L.sicn_ragged_roi_plan(4, IMG_W, IMG_H, LAT_W, LAT_H, None, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_roi_plan(4, IMG_W, IMG_H, LAT_W, LAT_H, ctypes.byref(r), None) == EINVAL


# ---- the window layout ----------------------------------------------------------------------------------------------------------
def _window_layout(shapes, wss, rows, c=LAT_C, n_images=None, want_images=True):
    L = _lib.lib()
    n = len(shapes) if n_images is None else n_images
    images = (_lib.RaggedWindowImage * max(n, 1))() if want_images else None
    totals = (ctypes.c_uint64 * 2)()
    rc = L.sicn_ragged_window_layout(_u32([w for w, _ in shapes]), _u32([h for _, h in shapes]), c, _u32(wss) if wss is not None else None,
                                     _u32([r for r, _ in rows]), _u32([h for _, h in rows]), n, images, totals)
    return rc, (list(images)[:max(n, 0)] if want_images else None), [int(v) for v in totals]


def _coder_workspace(shapes, wss, c=LAT_C):
    totals = (ctypes.c_uint64 * 3)()
    assert _lib.lib().sicn_ragged_codec_layout(_u32([w for w, _ in shapes]), _u32([h for _, h in shapes]), c,
                                               _u32(wss) if wss is not None else None, len(shapes), None, totals) == 0
    return int(totals[2])


@pytest.mark.parametrize("wss", [1024, 16384])
def test_window_layout_equals_plain_arithmetic(wss):
    # (lat_w, lat_h), (r0, rh): the whole image; one row; the last row with a short last stream; row boundaries that are stream
    # boundaries (lat_w = 16: 3072 symbols per row, three streams of 1024); a one-position latent
    cases = [((7, 9), (0, 9)), ((7, 9), (4, 1)), ((7, 9), (8, 1)), ((16, 3), (1, 1)), ((16, 3), (2, 1)), ((16, 16), (5, 6)),
             ((1, 1), (0, 1)), ((120, 68), (10, 17)), ((13, 11), (0, 1)), ((13, 11), (3, 8))]
    shapes, rows = [s for s, _ in cases], [r for _, r in cases]
    rc, images, totals = _window_layout(shapes, [wss] * len(cases), rows)
    assert rc == 0
    at = 0
    for (w, h), (r0, rh), im in zip(shapes, rows, images):
        n, row = w * h * LAT_C, w * LAT_C
        first, end = r0 * row // wss, -(-(r0 + rh) * row // wss)
        assert (im.first_stream, im.end_stream) == (first, end)
        assert im.band_bytes == min(n, end * wss) - first * wss
        assert im.lead == r0 * row - first * wss and im.lead < wss
        assert im.lead + rh * row <= im.band_bytes                       # the rows asked for lie inside the band
        assert im.band_offset == at and at % 16 == 0
        at += -(-im.band_bytes // 16) * 16
    assert totals == [at, _coder_workspace(shapes, [wss] * len(cases))]
    whole, last = images[0], images[2]
    assert (whole.first_stream, whole.end_stream, whole.lead, whole.band_bytes) == (0, -(-7 * 9 * LAT_C // wss), 0, 7 * 9 * LAT_C)
    assert last.end_stream == -(-7 * 9 * LAT_C // wss) and last.band_bytes == 7 * 9 * LAT_C - last.first_stream * wss
    if wss == 1024:
        assert (images[3].first_stream, images[3].end_stream, images[3].lead, images[3].band_bytes) == (3, 6, 0, 3072)
        assert last.band_bytes % wss != 0                                # the short last stream


def test_window_layout_default_stream_length_and_64_bit_offsets():
    rc, images, _ = _window_layout([(40, 30)], None, [(7, 3)])
    assert rc == 0 and images[0].first_stream == 7 * 40 * LAT_C // 16384
    # 140 images of 2^25 symbols, whole: 4.7 G band bytes — arithmetic only
    n_img = 140
    rc, images, totals = _window_layout([(4096, 8192)] * n_img, None, [(0, 8192)] * n_img, c=1)
    assert rc == 0
    assert images[-1].band_offset == (n_img - 1) * 2 ** 25 > 2 ** 32 and totals[0] == n_img * 2 ** 25


def test_window_layout_refusals():
    ok = ([(4, 4)], [1024], [(1, 2)])
    assert _window_layout(*ok)[0] == 0
    assert _window_layout(*ok, n_images=0)[0] == EINVAL
    assert _window_layout([(4, 4)], [1024], [(0, 0)])[0] == EINVAL                       # rh < 1
    assert _window_layout([(4, 4)], [1024], [(3, 2)])[0] == EINVAL                       # r0 + rh > lat_h
    assert _window_layout([(4, 4)], [1024], [(4, 1)])[0] == EINVAL
    assert _window_layout([(4, 4)], [1024], [(2 ** 32 - 1, 2)])[0] == EINVAL             # a sum that would wrap
    assert _window_layout([(4, 4), (4, 4)], [1024] * 2, [(0, 4), (0, 5)])[0] == EINVAL   # ... in any image
    assert _window_layout([(0, 4)], [1024], [(0, 1)])[0] == EINVAL                       # the coder layout's limits
    assert _window_layout([(4, 4)], [1000], [(0, 1)])[0] == EINVAL
    assert _window_layout([(4, 4)], [1024], [(0, 1)], c=0)[0] == EINVAL
    assert _window_layout([(2049, 1024)], [1024], [(0, 1)], c=1)[0] == EINVAL            # more than 2048 streams
    L = _lib.lib()
    one = _u32([4])
    assert L.sicn_ragged_window_layout(one, one, 4, None, None, one, 1, None, None) == EINVAL
    assert L.sicn_ragged_window_layout(one, one, 4, None, _u32([0]), None, 1, None, None) == EINVAL
    assert L.sicn_ragged_window_layout(one, one, 4, None, _u32([0]), one, 1, None, None) == 0      # both outputs optional


# ---- the cut layout ---------------------------------------------------------------------------------------------------------------
def _cut_layout(src, rects, channels, offsets=None, image=0, n_images=None):
    n = len(src) if n_images is None else n_images
    crects = (_lib.RaggedRect * max(len(rects), 1))(*[_lib.RaggedRect(*r) for r in rects])
    offs = None if offsets is None else (ctypes.c_uint64 * len(offsets))(*offsets)
    q = (ctypes.c_int64 * 4)()
    rc = _lib.lib().sicn_ragged_cut_layout(_i32([w for w, _ in src]), _i32([h for _, h in src]), crects, channels, offs, n, image, q)
    return rc, [int(v) for v in q]


def test_cut_layout_with_and_without_source_offsets():
    src = [(7, 9), (16, 3), (1, 1), (100, 131)]                    # (w, h)
    rects = [(2, 3, 4, 5), (0, 0, 16, 3), (0, 0, 1, 1), (99, 130, 1, 1)]
    for c in (3, 192):
        so = do = 0
        for i, ((w, h), (x0, y0, rw, rh)) in enumerate(zip(src, rects)):
            rc, q = _cut_layout(src, rects, c, image=i)
            assert rc == 0 and q[:2] == [so, do]
            so += w * h * c
            do += rw * rh * c
        assert q[2:] == [so, do]
        offsets = [5000000000, 64, 1 << 20, 0]                     # any order, gaps, beyond 2^32
        do = 0
        for i, (x0, y0, rw, rh) in enumerate(rects):
            rc, q = _cut_layout(src, rects, c, offsets, image=i)
            assert rc == 0 and q[:2] == [offsets[i], do]
            do += rw * rh * c
        assert q[2:] == [5000000000 + 7 * 9 * c, do]               # the furthest byte a source image reaches


def test_cut_layout_refusals():
    src, rects = [(8, 8)], [(1, 1, 4, 4)]
    assert _cut_layout(src, rects, 3)[0] == 0
    for bad in [(1, 1, 0, 4), (1, 1, 4, 0), (-1, 1, 4, 4), (1, -1, 4, 4), (5, 1, 4, 4), (1, 5, 4, 4), (8, 0, 1, 1), (0, 0, 9, 1),
                (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)]:
        assert _cut_layout(src, [bad], 3)[0] == EINVAL, bad
    assert _cut_layout(src, rects, 0)[0] == EINVAL
    assert _cut_layout(src, rects, 3, n_images=0)[0] == EINVAL
    assert _cut_layout(src, rects, 3, image=1)[0] == EINVAL and _cut_layout(src, rects, 3, image=-1)[0] == EINVAL
    assert _cut_layout([(0, 8)], rects, 3)[0] == EINVAL and _cut_layout([(8, (1 << 20) + 1)], rects, 3)[0] == EINVAL
    assert _cut_layout([(1 << 16, 1 << 15)], [(0, 0, 1, 1)], 1)[0] == EINVAL            # one image of 2^31 bytes
    assert _cut_layout([(1 << 16, (1 << 15) - 1)], [(0, 0, 1, 1)], 1)[0] == 0
    assert _cut_layout(src, rects, 3, offsets=[1 << 62])[0] == EINVAL
    assert _cut_layout([(8, 8), (8, 8)], [(0, 0, 8, 8), (0, 0, 8, 9)], 3, image=0)[0] == EINVAL   # ... in any image
    L = _lib.lib()
    q = (ctypes.c_int64 * 4)()
    r = (_lib.RaggedRect * 1)(_lib.RaggedRect(0, 0, 1, 1))
    assert L.sicn_ragged_cut_layout(None, _i32([8]), r, 3, None, 1, 0, q) == EINVAL
    assert L.sicn_ragged_cut_layout(_i32([8]), _i32([8]), None, 3, None, 1, 0, q) == EINVAL
    assert L.sicn_ragged_cut_layout(_i32([8]), _i32([8]), r, 3, None, 1, 0, None) == EINVAL


def test_device_calls_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    dummy = ctypes.c_void_p(64)
    one = _u32([1])
    assert L.sicn_ragged_window_create(None, one, one, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_window_create(dummy, one, one, None) == EINVAL
    assert L.sicn_ragged_window_workspace_bytes(None) == 0
    L.sicn_ragged_window_free(None)
    assert L.sicn_ragged_window_decode_async(None, dummy, None, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    r = (_lib.RaggedRect * 1)(_lib.RaggedRect(0, 0, 9, 1))
    assert L.sicn_ragged_cut_create(_i32([8]), _i32([8]), r, 3, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_cut_create(_i32([8]), _i32([8]), r, 3, None, 1, None) == EINVAL
    L.sicn_ragged_cut_free(None)
    assert L.sicn_ragged_cut_run(None, dummy, dummy, None) == EINVAL
    # with objects (where a gfx950 device exists to create them): NULL tensors and a short or odd workspace, before any launch
    coder = ctypes.c_void_p()
    rc = L.sicn_ragged_coder_create(_u32([7]), _u32([9]), LAT_C, _u32([1024]), None, None, 1, ctypes.byref(coder))
    assert rc in (0, -19)
    if rc == 0:
        win = ctypes.c_void_p()
        assert L.sicn_ragged_window_create(coder, _u32([8]), _u32([2]), ctypes.byref(win)) == EINVAL and not win.value
        assert L.sicn_ragged_window_create(coder, None, one, ctypes.byref(win)) == EINVAL
        assert L.sicn_ragged_window_create(coder, _u32([3]), _u32([2]), ctypes.byref(win)) == 0
        need = L.sicn_ragged_window_workspace_bytes(win)
        assert need == L.sicn_ragged_coder_workspace_bytes(coder) > 0
        call = L.sicn_ragged_window_decode_async
        assert call(win, None, None, dummy, dummy, dummy, need, None) == EINVAL
        assert call(win, dummy, None, None, dummy, dummy, need, None) == EINVAL
        assert call(win, dummy, None, dummy, None, dummy, need, None) == EINVAL
        assert call(win, dummy, None, dummy, dummy, dummy, need - 1, None) == ENOSPC
        assert call(win, dummy, None, dummy, dummy, None, need, None) == ENOSPC
        assert call(win, dummy, None, dummy, dummy, ctypes.c_void_p(72), need, None) == EINVAL
        L.sicn_ragged_window_free(win)
        L.sicn_ragged_coder_free(coder)


def test_window_host_under_the_sanitizers(tmp_path):
    """tests/cpp/window_plan_check.cpp — the pure-host header csrc/window_host.hpp with its own main — built with the address and
    undefined-behaviour sanitizers and run as a child process: the plan, the band arithmetic and the cut tables into heap blocks of
    exactly their length, extreme coordinates and every refusal."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "window_plan_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "window_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"window_plan_check ok: \d+ checks", r.stdout), r.stdout
