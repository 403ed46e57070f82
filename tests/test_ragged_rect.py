"""CPU-only checks of the rectangle output of a ragged net (include/sicn_ragged_rect.h): the symbols and the binding table,
sicn_ragged_rect_layout against Python arithmetic (offsets past 2^32 and the live-tile count by brute force included), every refusal
that can be reached without a device, and the store's and the tile test's arithmetic (csrc/ragged_rect_host.hpp) through a
stand-alone program under the host sanitizers.  Nothing touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import CLayerDesc, eight_layer_descs

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
EINVAL = -22
INTERLEAVED, PLANAR = 0, 1
GENERIC, PACKED = 0, 1


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_rect.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == ["sicn_ragged_ctx_roi_move_origins", "sicn_ragged_net_create_rect", "sicn_ragged_net_forward_at",
                    "sicn_ragged_rect_layout", "sicn_ragged_roi_move_origins"]
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_RECT_ABI), "python binding table and sicn_ragged_rect.h disagree"
    for other in (_lib.RAGGED_ABI, _lib.RAGGED_HYPER_ABI, _lib.RAGGED_RGB_ABI, _lib.RAGGED_ROI_MOVE_ABI, _lib.RAGGED_PLANAR_ABI,
                  _lib.RAGGED_WINDOW_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() == 17                          # the symbols being present is the marker


def _arrays(descs, sizes):
    n = len(descs)
    cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
    m = max(len(sizes), 1)
    return cd, n, (ctypes.c_int32 * m)(*[w for w, _ in sizes]), (ctypes.c_int32 * m)(*[h for _, h in sizes])


def _crects(rects):
    return None if rects is None else (_lib.RaggedRect * max(len(rects), 1))(*[_lib.RaggedRect(*r) for r in rects])


def _rect_layout(descs, sizes, rects, image, n_images=None):
    cd, n, ws, hs = _arrays(descs, sizes)
    out = (ctypes.c_int64 * 5)()
    rc = _lib.lib().sicn_ragged_rect_layout(cd, n, ws, hs, len(sizes) if n_images is None else n_images, _crects(rects), image, out)
    return rc, list(out)


def _chain_rule(descs, sizes):
    cur = list(sizes)
    for d in descs:
        cur = [(2 * w, 2 * h) if d.transposed else (-(-w // 2), -(-h // 2)) for w, h in cur]
    return cur


def _live_brute(recon, rect):
    """Tiles of 32 x 32 output pixels of a `recon` = (W, H) reconstruction that hold at least one pixel of `rect`."""
    (W, H), (x0, y0, w, h) = recon, rect
    mask = np.zeros((H, W), dtype=bool)
    mask[y0:y0 + h, x0:x0 + w] = True
    return sum(bool(mask[ty:ty + 32, tx:tx + 32].any()) for ty in range(0, H, 32) for tx in range(0, W, 32))


def _rects_for(rule, k):
    """One rectangle per image, of kind k."""
    out = []
    for W, H in rule:
        out.append([(0, 0, W, H), (W - 1, H - 1, 1, 1), (W // 3, H // 2, W - W // 3, H - H // 2), (min(31, W - 1), min(33, H - 1), 1, 1),
                    (W // 2, 0, max(W // 4, 1), H)][k])
    return out


def test_layout_equals_python_arithmetic_and_brute_force_live_tiles():
    eight = eight_layer_descs(768, 512)
    for descs in (eight, eight_layer_descs(768, 512, 64, 96), [eight[7]], eight[4:]):
        rule = _chain_rule(descs, SIZES)
        for k in range(5):
            rects = _rects_for(rule, k)
            off = 0
            total = sum(3 * w * h for _, _, w, h in rects)
            for i, (r, recon) in enumerate(zip(rects, rule)):
                rc, got = _rect_layout(descs, SIZES, rects, i)
                assert rc == 0 and got == [r[2], r[3], off, total, _live_brute(recon, r)], (len(descs), k, i, got)
                off += 3 * r[2] * r[3]
        # no rectangles: the whole reconstructions, every tile live, sicn_ragged_planar_layout's planar offsets
        for i, (W, H) in enumerate(rule):
            rc, got = _rect_layout(descs, SIZES, None, i)
            assert rc == 0 and got[:2] == [W, H] and got[4] == -(-W // 32) * -(-H // 32)
            assert got == _rect_layout(descs, SIZES, [(0, 0, w, h) for w, h in rule], i)[1]


def test_live_tiles_of_one_reconstruction_for_every_small_rectangle():
    """One 3 x 2-tile reconstruction (layer-7 input map 40 x 20, output 80 x 40); rectangles at every corner position on a grid that
    meets every tile edge, three sizes."""
    descs = [eight_layer_descs(768, 512)[7]]
    W, H = 80, 40
    for w, h in ((1, 1), (32, 32), (33, 7)):
        for y0 in list(range(0, H - h + 1, 5)) + [31, 32, H - h]:
            for x0 in list(range(0, W - w + 1, 7)) + [31, 32, 63, 64, W - w]:
                if x0 + w > W or y0 + h > H:
                    continue
                rc, got = _rect_layout(descs, [(40, 20)], [(x0, y0, w, h)], 0)
                assert rc == 0 and got == [w, h, 0, 3 * w * h, _live_brute((W, H), (x0, y0, w, h))], (x0, y0, w, h, got)


def test_layout_offsets_pass_two_to_the_32():
    """23 reconstructions of 8192 x 8176, stored whole — 200,933,376 bytes each — put the last images of the batch above 4 GiB."""
    descs = eight_layer_descs(768, 512)
    big, k = (8192, 8176), 23
    sizes = [big] * k + [(37, 19)]
    per = 3 * big[0] * big[1]
    assert (k - 1) * per > 2 ** 32
    rects = [(0, 0) + big] * k + [(5, 3, 33, 17)]
    rc, got = _rect_layout(descs, sizes, rects, k)
    assert rc == 0 and got == [33, 17, k * per, k * per + 3 * 33 * 17, 2]               # columns 5 .. 37 meet two tiles, rows 3 .. 19 one
    rc, got = _rect_layout(descs, sizes, rects, k - 1)
    assert rc == 0 and got == [big[0], big[1], (k - 1) * per, k * per + 3 * 33 * 17, 256 * 256] and got[2] > 2 ** 32
    rects[0] = (8191, 8175, 1, 1)                                                       # the offsets follow the rectangles
    rc, got = _rect_layout(descs, sizes, rects, k)
    assert rc == 0 and got[2:] == [(k - 1) * per + 3, (k - 1) * per + 3 + 3 * 33 * 17, 2]
    assert _rect_layout(descs, sizes, rects, 0)[1][4] == 1


def test_layout_refusals():
    eight = eight_layer_descs(768, 512)
    rule = _chain_rule(eight, SIZES)
    whole = [(0, 0, w, h) for w, h in rule]
    m = len(SIZES)
    assert _rect_layout(eight, SIZES, whole, 0)[0] == 0
    assert _rect_layout(eight[:4], SIZES, None, 0)[0] == EINVAL                      # the chain ends with a conv
    assert _rect_layout(eight[:7], SIZES, None, 0)[0] == EINVAL                      # ... with a deconv 128 -> 128
    assert _rect_layout(eight[:7], SIZES, whole, 0)[0] == EINVAL
    for i in range(m):
        W, H = rule[i]
        for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -1, 1), (0, 0, 1, -5),           # w < 1, h < 1
                    (-1, 0, 1, 1), (0, -1, 1, 1), (-2 ** 31, 0, 1, 1),                  # a negative corner
                    (0, 0, W + 1, H), (0, 0, W, H + 1), (1, 0, W, H), (0, 1, W, H), (W, 0, 1, 1), (0, H, 1, 1),   # beyond the chain-rule size
                    (2 ** 31 - 1, 0, 1, 1), (1, 0, 2 ** 31 - 1, 1), (0, 2 ** 31 - 1, 1, 2 ** 31 - 1)):            # ... past int32
            rects = list(whole)
            rects[i] = bad
            assert _rect_layout(eight, SIZES, rects, 0)[0] == EINVAL, (i, bad)
        rects = list(whole)
        rects[i] = (W - 1, H - 1, 1, 1)
        assert _rect_layout(eight, SIZES, rects, i)[0] == 0
    assert _rect_layout(eight, SIZES, whole, m)[0] == EINVAL
    assert _rect_layout(eight, SIZES, whole, -1)[0] == EINVAL
    assert _rect_layout(eight, [], None, 0, n_images=0)[0] == EINVAL
    cd, n, ws, hs = _arrays(eight, SIZES)
    L = _lib.lib()
    assert L.sicn_ragged_rect_layout(cd, n, ws, hs, m, _crects(whole), 0, None) == EINVAL
    assert L.sicn_ragged_rect_layout(None, n, ws, hs, m, _crects(whole), 0, (ctypes.c_int64 * 5)()) == EINVAL
    assert L.sicn_ragged_rect_layout(cd, n, None, hs, m, _crects(whole), 0, (ctypes.c_int64 * 5)()) == EINVAL
    # one image's tensor stays below 2 GiB at every boundary: 32768 x 32768 x 3 does not
    assert _rect_layout(eight, [(32768, 32768)], [(0, 0, 1, 1)], 0)[0] == EINVAL


def test_net_create_rect_and_forward_at_refuse_without_a_device_and_create_nothing():
    """Every refusal of the entries that needs no device, with nothing created.  Without weight handles no net can be created at all,
    so the code alone cannot tell one refusal from the other here; tests/test_ragged_rect_gpu.py repeats them over real handles,
    where the same calls with good arguments succeed."""
    L = _lib.lib()
    create = L.sicn_ragged_net_create_rect
    eight = eight_layer_descs(768, 512)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in eight])
    one = (ctypes.c_int32 * 1)(16)
    handles = (ctypes.c_void_p * 8)()
    good = [(3, 5, 7, 9)]
    cases = [
        dict(rects=[(0, 0, 0, 1)]), dict(rects=[(0, 0, 1, 0)]), dict(rects=[(-1, 0, 1, 1)]), dict(rects=[(0, -1, 1, 1)]),
        dict(rects=[(0, 0, 17, 16)]), dict(rects=[(0, 0, 16, 17)]), dict(rects=[(16, 0, 1, 1)]), dict(rects=[(2 ** 31 - 1, 0, 2, 1)]),
        dict(rects=good, rgb_ends=GENERIC), dict(rects=good, pixels_out=2), dict(rects=good, pixels_in=2), dict(rects=good, pixels_out=-1),
        dict(rects=good), dict(rects=good, pixels_out=PLANAR), dict(rects=None),        # good but for the NULL weight handles
    ]
    for case in cases:
        out = ctypes.c_void_p(0)
        rc = create(cd, handles, None, 8, one, one, 1, case.get("rgb_ends", PACKED), case.get("pixels_in", INTERLEAVED),
                    case.get("pixels_out", INTERLEAVED), _crects(case["rects"]), ctypes.byref(out))
        assert rc == EINVAL and not out.value, case
    for descs in (eight[:7], eight[:4]):                                                  # not a deconv N -> 3 at the end
        out = ctypes.c_void_p(0)
        cdd = (CLayerDesc * len(descs))(*[d.to_c() for d in descs])
        assert create(cdd, handles, None, len(descs), one, one, 1, PACKED, INTERLEAVED, INTERLEAVED, _crects([(0, 0, 1, 1)]),
                      ctypes.byref(out)) == EINVAL and not out.value
    assert create(cd, None, None, 8, one, one, 1, PACKED, INTERLEAVED, PLANAR, _crects(good), ctypes.byref(out)) == EINVAL
    assert create(cd, handles, None, 8, one, one, 1, PACKED, INTERLEAVED, PLANAR, _crects(good), None) == EINVAL
    assert L.sicn_ragged_net_forward_at(None, 0, 7, None, None, -1, None, None, 0, None, None) == EINVAL
    assert L.sicn_ragged_roi_move_origins(None) is None and L.sicn_ragged_ctx_roi_move_origins(None) is None


def test_python_keywords_are_checked_before_a_handle_is_made():
    from simple_image_compression_network_amd import api
    with pytest.raises(ValueError, match="exclude"):
        api.RaggedNet([(16, 16)], rgb_layout="planar", out_sizes=[(16, 16)], out_rects=[(0, 0, 16, 16)], shared_weights=[])
    with pytest.raises(ValueError, match="generic"):
        api.RaggedNet([(16, 16)], rgb_ends="generic", out_rects=[(0, 0, 16, 16)], shared_weights=[])
    with pytest.raises(ValueError, match="deconv"):
        api.RaggedNet([(16, 16)], out_rects=[(0, 0, 1, 1)], shared_weights=[], descs=eight_layer_descs(16, 16)[:4])
    with pytest.raises(ValueError, match="one \\(x0, y0, w, h\\) per image"):
        api.RaggedNet([(16, 16)], out_rects=[(0, 0, 1, 1), (0, 0, 1, 1)], shared_weights=[])
    with pytest.raises(ValueError, match="one \\(x0, y0, w, h\\) per image"):
        api.RaggedNet([(16, 16)], out_rects=[(0, 0, 1)], shared_weights=[])
    with pytest.raises(ValueError, match="out_layout"):
        api.RaggedNet([(16, 16)], out_rects=[(0, 0, 1, 1)], out_layout="chw", shared_weights=[])
    with pytest.raises(ValueError, match="out_layout"):
        api.RaggedNet([(16, 16)], out_layout="planar", shared_weights=[])
    for bad in ((0, 0, 17, 16), (-1, 0, 1, 1), (0, 0, 0, 1), (15, 15, 2, 1)):
        for layout in ("interleaved", "planar"):
            with pytest.raises(ValueError, match="out_rects"):
                api.RaggedNet([(16, 16)], rgb_layout=layout, out_rects=[bad], shared_weights=[])


def test_store_and_tile_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/ragged_rect_check.cpp — the host-callable header csrc/ragged_rect_host.hpp with its own main — built with the
    address and undefined-behaviour sanitizers and run as a child process: the store predicate, the address and the tile test
    over byte arrays of exactly 3 h w bytes, for every origin in a margin around six small reconstructions and at the int32
    extremes, both layouts: every in-rectangle pixel stored once, nothing else stored, no stored pixel in a skipped tile."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ragged_rect_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ragged_rect_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ragged_rect_check ok: \d+ checks", r.stdout), r.stdout
