"""CPU-only checks of the planar RGB boundaries of a ragged net (include/sicn_ragged_planar.h): the symbols and the binding table, the
layout of both pixel boundaries (sicn_ragged_planar_layout) against Python arithmetic and against sicn_ragged_layout, every refusal
that can be reached without a device, and the loader's and the store's arithmetic (csrc/ragged_planar_host.hpp) through a
stand-alone program under the host sanitizers.  Nothing touches a device."""
import ctypes
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import CLayerDesc, eight_layer_descs

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
EINVAL = -22
INTERLEAVED, PLANAR = 0, 1
GENERIC, PACKED = 0, 1


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_planar.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert syms == ["sicn_ragged_net_create_planar", "sicn_ragged_planar_layout"]
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_PLANAR_ABI), "python binding table and sicn_ragged_planar.h disagree"
    for other in (_lib.RAGGED_ABI, _lib.RAGGED_HYPER_ABI, _lib.RAGGED_RGB_ABI, _lib.RAGGED_ROI_MOVE_ABI):
        assert not set(syms) & set(other)
    assert L.sicn_version() == 17                          # the symbols being present is the marker
    text = (ROOT / "include" / "sicn_ragged_planar.h").read_text()
    assert re.search(r"#define\s+SICN_RAGGED_PIXELS_INTERLEAVED\s+0\b", text) and re.search(r"#define\s+SICN_RAGGED_PIXELS_PLANAR\s+1\b", text)
    assert _lib.RAGGED_PIXELS == {"interleaved": INTERLEAVED, "planar": PLANAR}


def _arrays(descs, sizes):
    n = len(descs)
    cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
    m = max(len(sizes), 1)
    return cd, n, (ctypes.c_int32 * m)(*[w for w, _ in sizes]), (ctypes.c_int32 * m)(*[h for _, h in sizes])


def _i32(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


def _planar_layout(descs, sizes, pixels_out, out_sizes, image, n_images=None):
    cd, n, ws, hs = _arrays(descs, sizes)
    ow = None if out_sizes is None else _i32([w for w, _ in out_sizes])
    oh = None if out_sizes is None else _i32([h for _, h in out_sizes])
    out = (ctypes.c_int64 * 6)()
    rc = _lib.lib().sicn_ragged_planar_layout(cd, n, ws, hs, len(sizes) if n_images is None else n_images, pixels_out, ow, oh, image, out)
    return rc, list(out)


def _layout(descs, sizes, layer, image):
    cd, n, ws, hs = _arrays(descs, sizes)
    out = (ctypes.c_int64 * 8)()
    assert _lib.lib().sicn_ragged_layout(cd, n, ws, hs, len(sizes), layer, image, out) == 0
    return list(out)


def _chain_rule(descs, sizes):
    cur = list(sizes)
    for d in descs:
        cur = [(2 * w, 2 * h) if d.transposed else (-(-w // 2), -(-h // 2)) for w, h in cur]
    return cur


def _python_layout(descs, sizes, out_sizes):
    """[(w, h, offset, bytes of the output, input offset, bytes of the input)] per image: three planes per image, back to back."""
    outs = _chain_rule(descs, sizes) if out_sizes is None else out_sizes
    c_in, c_out = descs[0].IFM_CH, descs[-1].OFM_CH
    res, o_off, i_off = [], 0, 0
    for (w, h), (ow, oh) in zip(sizes, outs):
        res.append([ow, oh, o_off, None, i_off, None])
        o_off += c_out * ow * oh
        i_off += c_in * w * h
    for r in res:
        r[3], r[5] = o_off, i_off
    return res


def test_layout_equals_python_arithmetic_and_sicn_ragged_layout():
    eight = eight_layer_descs(768, 512)
    cut = [(1, 1)] + SIZES[1:]                                               # image 0 cut to a single pixel, the others to their own sizes
    for descs in (eight, eight_layer_descs(768, 512, 64, 96), [eight[7]], [eight_layer_descs(768, 512, 64, 96)[7]]):
        rule = _chain_rule(descs, SIZES)
        for out_sizes in (None, rule, cut if len(descs) == 8 else [(1, 1)] * len(SIZES), [(w - (w > 1), h) for w, h in rule]):
            want = _python_layout(descs, SIZES, out_sizes)
            for i in range(len(SIZES)):
                rc, got = _planar_layout(descs, SIZES, PLANAR, out_sizes, i)
                assert rc == 0 and got == want[i], (len(descs), out_sizes, i, got, want[i])
                # the input boundary: sicn_ragged_layout's offsets of boundary -1, whatever the pixel layout
                ref = _layout(descs, SIZES, -1, i)
                assert got[4:6] == ref[3:5]
        # INTERLEAVED out: the chain-rule sizes at sicn_ragged_layout's offsets of the last boundary
        for i in range(len(SIZES)):
            rc, got = _planar_layout(descs, SIZES, INTERLEAVED, None, i)
            ref = _layout(descs, SIZES, len(descs) - 1, i)
            assert rc == 0 and got[:4] == [ref[0], ref[1], ref[3], ref[4]] and got[4:6] == _layout(descs, SIZES, -1, i)[3:5]
    # planar out at the chain-rule sizes has the interleaved tensor's offsets: both are 3 h w per image
    for i in range(len(SIZES)):
        assert _planar_layout(eight, SIZES, PLANAR, None, i)[1] == _planar_layout(eight, SIZES, INTERLEAVED, None, i)[1]


def test_layout_offsets_pass_two_to_the_32():
    """23 images of 8192 x 8176 — 200,933,376 bytes each, and 32 bytes per pixel behind layer 0 stay below the 2 GiB limit of one
    image — put the last images of the batch above 4 GiB."""
    descs = eight_layer_descs(768, 512)
    big, k = (8192, 8176), 23
    sizes = [big] * k + [(5, 3)]
    per = 3 * big[0] * big[1]
    assert (k - 1) * per > 2 ** 32
    for out_sizes in (None, sizes):
        rc, got = _planar_layout(descs, sizes, PLANAR, out_sizes, k)
        w, h = (5, 3) if out_sizes else (16, 16)
        assert rc == 0 and got == [w, h, k * per, k * per + 3 * w * h, k * per, k * per + 45]
        assert got[4:6] == _layout(descs, sizes, -1, k)[3:5]
        rc, got = _planar_layout(descs, sizes, PLANAR, out_sizes, k - 1)
        assert rc == 0 and got[:3] == [big[0], big[1], (k - 1) * per] and got[2] > 2 ** 32
    cut = [(1, 1)] * (k - 1) + [big, (5, 3)]                # the offsets follow the cut, not the chain rule
    rc, got = _planar_layout(descs, sizes, PLANAR, cut, k)
    assert rc == 0 and got[2:] == [3 * (k - 1) + per, 3 * (k - 1) + per + 45, k * per, k * per + 45]


def test_layout_refusals():
    eight = eight_layer_descs(768, 512)
    rule = _chain_rule(eight, SIZES)
    L = _lib.lib()
    m = len(SIZES)
    assert _planar_layout(eight, SIZES, PLANAR, SIZES, 0)[0] == 0
    for bad in (2, -1, 256):
        assert _planar_layout(eight, SIZES, bad, None, 0)[0] == EINVAL                      # a pixels value other than the two
    assert _planar_layout(eight[:4], SIZES, PLANAR, None, 0)[0] == EINVAL                   # the chain ends with a conv
    assert _planar_layout(eight[:7], SIZES, PLANAR, None, 0)[0] == EINVAL                   # ... with a deconv 128 -> 128
    assert _planar_layout(eight[:7], SIZES, INTERLEAVED, None, 0)[0] == 0
    assert _planar_layout(eight, SIZES, INTERLEAVED, SIZES, 0)[0] == EINVAL                 # sizes with INTERLEAVED out
    cd, n, ws, hs = _arrays(eight, SIZES)
    out = (ctypes.c_int64 * 6)()
    assert L.sicn_ragged_planar_layout(cd, n, ws, hs, m, PLANAR, ws, None, 0, out) == EINVAL    # only one of the two
    assert L.sicn_ragged_planar_layout(cd, n, ws, hs, m, PLANAR, None, hs, 0, out) == EINVAL
    assert L.sicn_ragged_planar_layout(cd, n, ws, hs, m, PLANAR, ws, hs, 0, None) == EINVAL
    assert L.sicn_ragged_planar_layout(None, n, ws, hs, m, PLANAR, ws, hs, 0, out) == EINVAL
    for i in range(m):
        for dw, dh in ((1, 0), (0, 1)):                                                         # one above the chain-rule size
            over = list(rule)
            over[i] = (rule[i][0] + dw, rule[i][1] + dh)
            assert _planar_layout(eight, SIZES, PLANAR, over, 0)[0] == EINVAL
        for w, h in ((0, 1), (1, 0), (-1, 1)):                                                  # below 1
            under = list(rule)
            under[i] = (w, h)
            assert _planar_layout(eight, SIZES, PLANAR, under, 0)[0] == EINVAL
    assert _planar_layout(eight, SIZES, PLANAR, rule, 0)[0] == 0
    assert _planar_layout(eight, SIZES, PLANAR, None, m)[0] == EINVAL
    assert _planar_layout(eight, SIZES, PLANAR, None, -1)[0] == EINVAL
    assert _planar_layout(eight, [], PLANAR, None, 0, n_images=0)[0] == EINVAL
    # one image's tensor stays below 2 GiB at every boundary: 32768 x 32768 x 3 does not
    assert _planar_layout(eight, [(32768, 32768)], PLANAR, [(1, 1)], 0)[0] == EINVAL


def test_net_create_planar_refuses_without_a_device_and_creates_nothing():
    """Every refusal of the entry, with nothing created.  Without a device and without weight handles no net can be created at all,
    so the code alone cannot tell one refusal from the other here; tests/test_ragged_planar_gpu.py repeats them over real handles,
    where the same calls with good arguments succeed."""
    L = _lib.lib()
    create = L.sicn_ragged_net_create_planar
    eight = eight_layer_descs(768, 512)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in eight])
    one = _i32([16])
    big = _i32([17])
    handles = (ctypes.c_void_p * 8)()
    cases = [
        dict(pixels_in=2), dict(pixels_out=2), dict(pixels_in=-1), dict(pixels_out=-1),
        dict(pixels_in=PLANAR, rgb_ends=GENERIC), dict(pixels_out=PLANAR, rgb_ends=GENERIC),
        dict(ow=one, oh=one), dict(pixels_out=PLANAR, ow=one), dict(pixels_out=PLANAR, oh=one),
        dict(pixels_out=PLANAR, ow=big, oh=one), dict(pixels_out=PLANAR, ow=one, oh=_i32([0])),
        dict(pixels_in=PLANAR, pixels_out=PLANAR, ow=one, oh=one),                      # good but for the NULL weight handles
    ]
    for case in cases:
        out = ctypes.c_void_p(0)
        rc = create(cd, handles, None, 8, one, one, 1, case.get("rgb_ends", PACKED), case.get("pixels_in", INTERLEAVED),
                    case.get("pixels_out", INTERLEAVED), case.get("ow"), case.get("oh"), ctypes.byref(out))
        assert rc == EINVAL and not out.value, case
    # PLANAR at an end whose layer is not conv 3 -> N / deconv N -> 3
    for descs, kw in ((eight[1:], dict(pixels_in=PLANAR)), (eight[:7], dict(pixels_out=PLANAR))):
        out = ctypes.c_void_p(0)
        cdd = (CLayerDesc * 7)(*[d.to_c() for d in descs])
        rc = create(cdd, handles, None, 7, one, one, 1, PACKED, kw.get("pixels_in", INTERLEAVED), kw.get("pixels_out", INTERLEAVED), None, None,
                    ctypes.byref(out))
        assert rc == EINVAL and not out.value
    assert create(cd, None, None, 8, one, one, 1, PACKED, PLANAR, PLANAR, None, None, ctypes.byref(out)) == EINVAL
    assert create(cd, handles, None, 8, one, one, 1, PACKED, PLANAR, PLANAR, None, None, None) == EINVAL


def test_python_keywords_are_checked_before_a_handle_is_made():
    from simple_image_compression_network_amd import api
    for bad in ("chw", "", None, 1):
        with pytest.raises(ValueError, match="rgb_layout"):
            api.RaggedNet([(16, 16)], rgb_layout=bad, shared_weights=[])
    with pytest.raises(ValueError, match="generic"):
        api.RaggedNet([(16, 16)], rgb_layout="planar", rgb_ends="generic", shared_weights=[])
    with pytest.raises(ValueError, match="out_sizes"):
        api.RaggedNet([(16, 16)], out_sizes=[(16, 16)], shared_weights=[])                   # interleaved: no sizes of its own
    with pytest.raises(ValueError, match="out_sizes"):
        api.RaggedNet([(16, 16)], rgb_layout="planar", out_sizes=[(16, 16)], shared_weights=[], descs=eight_layer_descs(16, 16)[:4])
    with pytest.raises(ValueError, match="out_sizes"):
        api.RaggedNet([(16, 16)], rgb_layout="planar", out_sizes=[(16, 16), (1, 1)], shared_weights=[])


def test_loader_and_store_arithmetic_under_the_sanitizers(tmp_path):
    """tests/cpp/ragged_planar_check.cpp — the host-callable header csrc/ragged_planar_host.hpp with its own main — built with the
    address and undefined-behaviour sanitizers and run as a child process: the planar loader over byte arrays of exactly the
    permitted size (every quad of every tile, all four byte phases of plane and row starts, widths 1 .. 35, heights 1 .. 33) against
    direct indexing, and the planar store's address and predicate for four cuts."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ragged_planar_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ragged_planar_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ragged_planar_check ok: \d+ checks", r.stdout), r.stdout
