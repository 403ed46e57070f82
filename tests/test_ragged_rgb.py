"""CPU-only checks of the packed RGB ends of a ragged net (include/sicn_ragged_rgb.h): the symbols and the binding table, the work cut
of both forms (sicn_ragged_rgb_layout) against Python arithmetic and against sicn_ragged_layout, every refusal, and the K packing
and weight images (csrc/ragged_rgb_host.hpp) through a stand-alone program under the host sanitizers.  Nothing touches a device."""
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
GENERIC, PACKED = 0, 1


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_rgb.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) == 3
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_RGB_ABI), "python binding table and sicn_ragged_rgb.h disagree"
    assert L.sicn_version() >= 15
    text = (ROOT / "include" / "sicn_ragged_rgb.h").read_text()
    assert re.search(r"#define\s+SICN_RAGGED_RGB_GENERIC\s+0\b", text) and re.search(r"#define\s+SICN_RAGGED_RGB_PACKED\s+1\b", text)
    assert _lib.RAGGED_RGB_ENDS == {"generic": GENERIC, "packed": PACKED}


def _arrays(descs, sizes):
    n = len(descs)
    cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
    m = max(len(sizes), 1)
    return cd, n, (ctypes.c_int32 * m)(*[w for w, _ in sizes]), (ctypes.c_int32 * m)(*[h for _, h in sizes])


def _rgb_layout(descs, sizes, rgb_ends, layer, image, n_images=None):
    cd, n, ws, hs = _arrays(descs, sizes)
    out = (ctypes.c_int64 * 3)()
    rc = _lib.lib().sicn_ragged_rgb_layout(cd, n, ws, hs, len(sizes) if n_images is None else n_images, rgb_ends, layer, image, out)
    return rc, list(out)


def _layout(descs, sizes, layer, image):
    cd, n, ws, hs = _arrays(descs, sizes)
    out = (ctypes.c_int64 * 8)()
    assert _lib.lib().sicn_ragged_layout(cd, n, ws, hs, len(sizes), layer, image, out) == 0
    return list(out)


def _python_cut(descs, sizes, packed):
    """{(layer, image): [first item, tiles_x, items of the layer]} by the chain rule: one item per 16 x 16 tile of the M grid, times the
    four phases of a deconv unless it is an N -> 3 one of a packed net."""
    res = {}
    cur = list(sizes)
    for l, d in enumerate(descs):
        nxt = [(2 * w, 2 * h) if d.transposed else (-(-w // 2), -(-h // 2)) for w, h in cur]
        per_tile = 4 if d.transposed and not (packed and d.OFM_CH == 3) else 1
        first = 0
        for i, ((iw, ih), (ow, oh)) in enumerate(zip(cur, nxt)):
            mw, mh = (iw, ih) if d.transposed else (ow, oh)
            tx, ty = -(-mw // 16), -(-mh // 16)
            res[(l, i)] = [first, tx, None]
            first += tx * ty * per_tile
        for i in range(len(cur)):
            res[(l, i)][2] = first
        cur = nxt
    return res


def _chains():
    """The eight-layer chain at two width pairs, and each of its layers as a one-layer chain."""
    chains = []
    for widths in [(128, 192), (64, 96)]:
        descs = eight_layer_descs(768, 512, *widths)
        chains.append(descs)
        chains += [[d] for d in descs]
    return chains


def test_layout_of_both_forms_equals_python_arithmetic_and_sicn_ragged_layout():
    for descs in _chains():
        ref = {GENERIC: _python_cut(descs, SIZES, False), PACKED: _python_cut(descs, SIZES, True)}
        for layer, d in enumerate(descs):
            for i in range(len(SIZES)):
                rc_g, gen = _rgb_layout(descs, SIZES, GENERIC, layer, i)
                rc_p, pck = _rgb_layout(descs, SIZES, PACKED, layer, i)
                assert rc_g == 0 and rc_p == 0
                assert gen == ref[GENERIC][(layer, i)] and pck == ref[PACKED][(layer, i)], (layer, i)
                assert gen == _layout(descs, SIZES, layer, i)[5:8], (layer, i)      # GENERIC: sicn_ragged_layout, field for field
                if d.transposed and d.OFM_CH == 3:
                    # one item per tile: exactly a quarter of the generic items, tiles_x unchanged
                    assert [4 * pck[0], pck[1], 4 * pck[2]] == gen, (layer, i)
                else:
                    assert pck == gen, (layer, i)


def test_item_counts_of_the_packed_cut():
    descs = eight_layer_descs(768, 512)

    def counts(size, form):
        return [_rgb_layout(descs, [size], form, l, 0)[1][2] for l in range(8)]
    assert counts((131, 70), GENERIC) == [15, 6, 2, 1, 4, 8, 24, 60]
    assert counts((131, 70), PACKED) == [15, 6, 2, 1, 4, 8, 24, 15]
    assert counts((100, 36), PACKED) == [8, 2, 1, 1, 4, 4, 8, 8]
    both = [(131, 70), (100, 36)]
    assert [_rgb_layout(descs, both, PACKED, l, 1)[1][0] for l in range(8)] == counts((131, 70), PACKED)


def test_every_refusal_is_einval():
    descs = eight_layer_descs(768, 512)
    L = _lib.lib()
    cd, n, ws, hs = _arrays(descs, SIZES)
    out = (ctypes.c_int64 * 3)()
    m = len(SIZES)
    assert L.sicn_ragged_rgb_layout(cd, n, ws, hs, m, PACKED, 0, 0, out) == 0
    assert L.sicn_ragged_rgb_layout(None, n, ws, hs, m, PACKED, 0, 0, out) == EINVAL
    assert L.sicn_ragged_rgb_layout(cd, n, None, hs, m, PACKED, 0, 0, out) == EINVAL
    assert L.sicn_ragged_rgb_layout(cd, n, ws, None, m, PACKED, 0, 0, out) == EINVAL
    assert L.sicn_ragged_rgb_layout(cd, n, ws, hs, m, PACKED, 0, 0, None) == EINVAL
    for form in (2, -1, 256):
        assert _rgb_layout(descs, SIZES, form, 0, 0)[0] == EINVAL
    for form in (GENERIC, PACKED):
        assert _rgb_layout(descs, SIZES, form, 8, 0)[0] == EINVAL
        assert _rgb_layout(descs, SIZES, form, -1, 0)[0] == EINVAL      # the cut of a layer: there is none for the input boundary
        assert _rgb_layout(descs, SIZES, form, 0, m)[0] == EINVAL
        assert _rgb_layout(descs, SIZES, form, 0, -1)[0] == EINVAL
        assert _rgb_layout(descs, [], form, 0, 0, n_images=0)[0] == EINVAL
        assert _rgb_layout(descs, [(16, 16), (0, 5)], form, 0, 0)[0] == EINVAL
        assert _rgb_layout(descs, SIZES, form, 7, m - 1)[0] == 0


def test_net_create_rgb_and_kernel_for_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    out = ctypes.c_void_p()
    descs = eight_layer_descs(768, 512)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in descs])
    one = (ctypes.c_int32 * 1)(16)
    handles = (ctypes.c_void_p * 8)()
    create = L.sicn_ragged_net_create_rgb
    assert create(cd, handles, None, 8, one, one, 1, 2, ctypes.byref(out)) == EINVAL          # rgb_ends = 2
    assert create(cd, handles, None, 8, one, one, 1, -1, ctypes.byref(out)) == EINVAL
    assert create(cd, handles, None, 8, one, one, 0, PACKED, ctypes.byref(out)) == EINVAL
    assert create(cd, handles, None, 8, one, one, 1, PACKED, ctypes.byref(out)) == EINVAL     # NULL weight handles
    assert create(cd, None, None, 8, one, one, 1, GENERIC, ctypes.byref(out)) == EINVAL
    assert create(cd, handles, None, 8, one, one, 1, PACKED, None) == EINVAL
    assert not out.value
    assert L.sicn_ragged_net_kernel_for(None, 0) is None


def test_python_keyword_is_checked_before_a_handle_is_made():
    from simple_image_compression_network_amd import api
    for bad in ("fast", "", None, 1):
        with pytest.raises(ValueError, match="rgb_ends"):
            api.RaggedNet([(16, 16)], rgb_ends=bad, shared_weights=[])


def test_pack_host_under_the_sanitizers(tmp_path):
    """tests/cpp/ragged_rgb_pack_check.cpp — the pure-host header csrc/ragged_rgb_host.hpp with its own main — built with the address
    and undefined-behaviour sanitizers and run as a child process: the K walk of both kernels over packed random weights against the
    closed forms, junk in every byte that only zero weights meet, heap blocks of exactly their length, and a wrong byte is seen."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ragged_rgb_pack_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "ragged_rgb_pack_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"ragged_rgb_pack_check ok: \d+ checks", r.stdout), r.stdout
