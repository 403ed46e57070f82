"""CPU-only checks of the hyperprior window decode's host side (include/sicn_ragged_ctx_window.h): the symbols and the binding
table; sicn_ragged_ctx_window_layout against the header's arithmetic restated in Python; that the plan is SUFFICIENT, by brute force
over the set order as tests/codec_edge_cases.py states it in numpy (none of the library's code); 64-bit band offsets; every refusal;
the argument checks of the device call that come before a device is asked for; and the pure-host header under the host sanitizers.
Nothing here touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import codec_edge_cases as cases
from simple_image_compression_network_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ENOSPC = -22, -28
WSS = cases.WSS
# (h, w, c): every window of the small ones, a seeded sample of the large ones
SMALL = [(1, 1, 4), (2, 2, 4), (1, 5, 192), (5, 1, 192), (3, 3, 192), (37, 37, 192), (40, 48, 192)]
LARGE = [(37, 200, 192), (37, 201, 192), (86, 86, 192), (135, 240, 192)]


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_ctx_window.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_ctx_window_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == sorted(["sicn_ragged_ctx_window_layout", "sicn_ragged_ctx_window_create", "sicn_ragged_ctx_window_free",
                           "sicn_ragged_ctx_window_workspace_bytes", "sicn_ragged_ctx_window_decode_async"])
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_CTX_WINDOW_ABI), "python binding table and sicn_ragged_ctx_window.h disagree"
    for other in (_lib.ABI, _lib.CODEC_ABI, _lib.CONVLAYER_ABI, _lib.GDN_ABI, _lib.RAGGED_ABI, _lib.RAGGED_HYPER_ABI, _lib.RAGGED_CODEC_ABI,
                  _lib.RAGGED_CTX_ABI, _lib.RAGGED_ARCHIVE_ABI, _lib.RAGGED_ARCHIVE_SELECT_ABI, _lib.RAGGED_WINDOW_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() >= 13
    assert ctypes.sizeof(_lib.RaggedCtxWindowImage) == 40


def _layout(shapes, rows, c=192, n_images=None, want_images=True):
    """shapes: [(h, w)], rows: [(r0, rh)] -> (rc, images, totals)."""
    n = len(shapes) if n_images is None else n_images
    images = (_lib.RaggedCtxWindowImage * max(n, 1))() if want_images else None
    totals = (ctypes.c_uint64 * 2)()
    rc = _lib.lib().sicn_ragged_ctx_window_layout(_u32([w for _, w in shapes]), _u32([h for h, _ in shapes]), c, _u32([r for r, _ in rows]),
                                                  _u32([h for _, h in rows]), n, images, totals)
    return rc, (list(images)[:max(n, 0)] if want_images else None), [int(v) for v in totals]


def _python_plan(H, W, C, r0, rh):
    """The header's plan, in its words: (band_row0, band_rows, first[2], end[2], symbols)."""
    R, r1 = W * C, r0 + rh
    nsym, _ = cases.ctx_geometry(H, W, C)
    ceil = lambda a, b: -(-a // b)
    lo, hi = (r0 >> 1) * R, min(nsym[1], ((r1 + 1) >> 1) * R)
    if hi > lo:
        N0, N1 = lo // WSS, ceil(hi, WSS)
        P0, P1 = N0 * WSS // R, ceil(min(nsym[1], N1 * WSS), R)
        A0, A1 = max(0, min(r0, 2 * P0 - 1)), min(H, max(r1, 2 * P1 + 1))
    else:
        N0 = N1 = 0
        A0, A1 = r0, r1
    M0, M1 = (A0 >> 1) * R // WSS, ceil(min(nsym[0], ((A1 + 1) >> 1) * R), WSS)
    Q0, Q1 = M0 * WSS // R, ceil(min(nsym[0], M1 * WSS), R)
    B0, B1 = (2 * min(P0, Q0), min(H, 2 * max(P1, Q1))) if hi > lo else (2 * Q0, min(H, 2 * Q1))
    symbols = min(nsym[0], M1 * WSS) - M0 * WSS + (min(nsym[1], N1 * WSS) - N0 * WSS if hi > lo else 0)
    return B0, B1 - B0, (M0, N0), (M1, N1), symbols


def _windows(H, every):
    if every:
        return [(r0, rh) for r0 in range(H) for rh in range(1, H - r0 + 1)]
    rng = np.random.default_rng(H)
    out = [(0, H), (0, 1), (H - 1, 1)]
    for _ in range(120):
        r0 = int(rng.integers(0, H))
        out.append((r0, int(rng.integers(1, H - r0 + 1))))
    return out


def _pixel_streams(H, W, C):
    """Per pixel [H][W]: its set, and the first and the last stream (in the set's own numbering) that hold its C symbols — from
    codec_edge_cases.ctx_set_order applied to the symbols' own indices."""
    index = np.arange(H * W * C, dtype=np.int64).reshape(H, W, C)
    order = cases.ctx_set_order(index)                        # coding position -> symbol
    na = cases.ctx_geometry(H, W, C)[0][0]
    pos = np.empty(H * W * C, np.int64)
    pos[order] = np.arange(order.size)
    pos = pos.reshape(H, W, C)
    anchor, _ = cases.ctx_masks(H, W)
    stream = np.where(anchor[:, :, None], pos, pos - na) // WSS
    return (~anchor).astype(np.int64), stream[:, :, 0], stream[:, :, -1]


@pytest.mark.parametrize("shape", SMALL + LARGE, ids=lambda s: "x".join(map(str, s)))
def test_layout_is_the_headers_arithmetic_and_sufficient(shape):
    H, W, C = shape
    rows = _windows(H, shape in SMALL)
    rc, images, totals = _layout([(H, W)] * len(rows), rows, c=C)
    assert rc == 0
    pset, first, last = _pixel_streams(H, W, C)
    nsym, nst = cases.ctx_geometry(H, W, C)
    ys = np.arange(H)[:, None]
    at = 0
    for (r0, rh), im in zip(rows, images):
        b0, brows, f, e, symbols = _python_plan(H, W, C, r0, rh)
        assert (im.band_row0, im.band_rows, tuple(im.first_stream), tuple(im.end_stream), im.symbols) == (b0, brows, f, e, symbols), (r0, rh)
        assert im.band_bytes == brows * W * C and im.band_offset == at and at % 16 == 0
        at += -(-im.band_bytes // 16) * 16
        # sufficiency, on the numpy statement of the order alone
        lo, hi = np.array(f)[pset], np.array(e)[pset]
        whole = (first >= lo) & (last < hi)                   # every symbol of the pixel is in a selected stream
        some = ((first >= lo) & (first < hi)) | ((last >= lo) & (last < hi))
        assert whole[r0:r0 + rh].all(), (r0, rh)              # the wanted rows are held
        held_rows = np.nonzero(some.any(axis=1))[0]
        assert held_rows.min() >= b0 and held_rows.max() < b0 + brows, (r0, rh)     # every symbol of a selected stream lies in the band
        assert b0 <= r0 and r0 + rh <= b0 + brows <= H
        held_other = some & (pset == 1)
        need = np.zeros((H, W), bool)                         # the in-range 4-neighbours of every held non-anchor
        need[:-1] |= held_other[1:]
        need[1:] |= held_other[:-1]
        need[:, :-1] |= held_other[:, 1:]
        need[:, 1:] |= held_other[:, :-1]
        assert not (need & (pset == 1)).any()                 # (the neighbours of a non-anchor are anchors)
        assert whole[need].all(), (r0, rh)
        if (r0, rh) == (0, H):                                # the whole image selects every stream and the band is the latent
            assert (b0, brows, f, e, symbols) == (0, H, (0, 0), nst, H * W * C)
    assert totals[0] == at
    ws = (ctypes.c_uint64 * 3)()
    assert _lib.lib().sicn_ragged_ctx_layout(_u32([W] * len(rows)), _u32([H] * len(rows)), C, len(rows), None, ws) == 0
    assert totals[1] == int(ws[2])                            # the full ctx coder's workspace


def test_band_offsets_are_64_bit():
    # five images of 0x7F000000 symbols, whole: 10.6 G band bytes — arithmetic only
    w, h = 0x7F0000 // 4, 256
    shapes = [(h, w), (3, 3)] + [(h, w)] * 4
    rc, images, totals = _layout(shapes, [(0, h), (1, 1)] + [(0, h)] * 4, c=4)
    assert rc == 0
    assert images[1].band_offset == 0x7F000000 and images[1].band_bytes == 36
    assert images[2].band_offset == 0x7F000000 + 48                      # 36 rounded up to a multiple of 16
    assert images[5].band_offset == 4 * 0x7F000000 + 48 > 2 ** 32 and totals[0] == 5 * 0x7F000000 + 48
    assert all(im.band_offset % 16 == 0 for im in images)


def test_layout_refusals():
    ok = ([(4, 4)], [(1, 2)])
    assert _layout(*ok, c=4)[0] == 0
    assert _layout(*ok, c=4, n_images=0)[0] == EINVAL
    assert _layout([(4, 4)], [(0, 0)], c=4)[0] == EINVAL                       # rh < 1
    assert _layout([(4, 4)], [(3, 2)], c=4)[0] == EINVAL                       # r0 + rh > lat_h
    assert _layout([(4, 4)], [(4, 1)], c=4)[0] == EINVAL
    assert _layout([(4, 4)], [(2 ** 32 - 1, 2)], c=4)[0] == EINVAL             # a sum that would wrap
    assert _layout([(4, 4), (4, 4)], [(0, 4), (0, 5)], c=4)[0] == EINVAL       # ... in any image
    # the limits of sicn_ragged_ctx_layout
    assert _layout([(0, 4)], [(0, 1)], c=4)[0] == EINVAL and _layout([(4, 0)], [(0, 1)], c=4)[0] == EINVAL
    assert _layout([(4, 4)], [(0, 1)], c=0)[0] == EINVAL and _layout([(4, 4)], [(0, 1)], c=6)[0] == EINVAL
    assert _layout([(256, 0x7F0000 // 4 + 1)], [(0, 1)], c=4)[0] == EINVAL     # more than 0x7F000000 symbols
    assert _layout([(256, 0x7F0000 // 4)], [(0, 1)], c=4)[0] == 0
    L = _lib.lib()
    four, one, zero = _u32([4]), _u32([1]), _u32([0])
    assert L.sicn_ragged_ctx_window_layout(None, four, 4, zero, one, 1, None, None) == EINVAL
    assert L.sicn_ragged_ctx_window_layout(four, None, 4, zero, one, 1, None, None) == EINVAL
    assert L.sicn_ragged_ctx_window_layout(four, four, 4, None, one, 1, None, None) == EINVAL
    assert L.sicn_ragged_ctx_window_layout(four, four, 4, zero, None, 1, None, None) == EINVAL
    assert L.sicn_ragged_ctx_window_layout(four, four, 4, zero, one, 1, None, None) == 0        # both outputs optional


def test_device_calls_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    h = ctypes.c_void_p()
    dummy = ctypes.c_void_p(64)
    one = _u32([1])
    assert L.sicn_ragged_ctx_window_create(None, one, one, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_window_create(dummy, one, one, None) == EINVAL
    assert L.sicn_ragged_ctx_window_workspace_bytes(None) == 0
    L.sicn_ragged_ctx_window_free(None)
    assert L.sicn_ragged_ctx_window_decode_async(None, dummy, None, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    # with objects (where a gfx950 device exists to create them): NULL and misaligned tensors, a short or odd workspace
    coder = ctypes.c_void_p()
    rc = L.sicn_ragged_ctx_coder_create(_u32([7]), _u32([9]), 192, None, None, 1, ctypes.byref(coder))
    assert rc in (0, -19)
    if rc == 0:
        win = ctypes.c_void_p()
        assert L.sicn_ragged_ctx_window_create(coder, _u32([8]), _u32([2]), ctypes.byref(win)) == EINVAL and not win.value
        assert L.sicn_ragged_ctx_window_create(coder, _u32([3]), _u32([0]), ctypes.byref(win)) == EINVAL and not win.value
        assert L.sicn_ragged_ctx_window_create(coder, None, one, ctypes.byref(win)) == EINVAL
        assert L.sicn_ragged_ctx_window_create(coder, one, None, ctypes.byref(win)) == EINVAL
        assert L.sicn_ragged_ctx_window_create(coder, _u32([3]), _u32([2]), ctypes.byref(win)) == 0
        need = L.sicn_ragged_ctx_window_workspace_bytes(win)
        assert need == L.sicn_ragged_ctx_coder_workspace_bytes(coder) > 0
        call = L.sicn_ragged_ctx_window_decode_async
        assert call(win, None, None, dummy, dummy, dummy, dummy, need, None) == EINVAL
        assert call(win, dummy, None, None, dummy, dummy, dummy, need, None) == EINVAL
        assert call(win, dummy, None, dummy, None, dummy, dummy, need, None) == EINVAL
        assert call(win, dummy, None, dummy, dummy, None, dummy, need, None) == EINVAL
        assert call(win, ctypes.c_void_p(65), None, dummy, dummy, dummy, dummy, need, None) == EINVAL     # an odd `containers`
        assert call(win, dummy, None, ctypes.c_void_p(66), dummy, dummy, dummy, need, None) == EINVAL     # scales not 4-byte aligned
        assert call(win, dummy, None, dummy, ctypes.c_void_p(66), dummy, dummy, need, None) == EINVAL     # band not 4-byte aligned
        assert call(win, dummy, None, dummy, dummy, dummy, dummy, need - 1, None) == ENOSPC
        assert call(win, dummy, None, dummy, dummy, dummy, None, need, None) == ENOSPC
        assert call(win, dummy, None, dummy, dummy, dummy, ctypes.c_void_p(72), need, None) == EINVAL
        L.sicn_ragged_ctx_window_free(win)
        L.sicn_ragged_ctx_coder_free(coder)


def test_ctx_window_host_under_the_sanitizers(tmp_path):
    """tests/cpp/ctx_window_plan_check.cpp — the pure-host header csrc/ctx_window_host.hpp with its own main — built with the address
    and undefined-behaviour sanitizers and run as a child process: the plan against brute force into heap blocks of exactly their
    length, the largest shapes and every refusal.  Host code only; nothing is loaded into Python."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ctx_window_plan_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ctx_window_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ctx_window_plan_check ok: \d+ checks", r.stdout), r.stdout
