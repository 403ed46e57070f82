"""CPU-only checks of the ragged latent coder's ABI (include/sicn_ragged_codec.h): the symbols, the binding table, and
sicn_ragged_codec_layout — where every latent, container slot and workspace block of a batch of different shapes lies and how every
image is cut into streams — against plain Python arithmetic.  Nothing here touches a device."""
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
EINVAL = -22
# (lat_w, lat_h, stream_symbols): 12 mixed shapes — one symbol, exact multiples of a stream, one over, every admissible length
SHAPES = [(1, 1, 1024), (3, 7, 16384), (16, 12, 8192), (13, 11, 2048), (2, 9, 4096), (48, 48, 1024), (64, 1, 16384), (1, 64, 1024),
          (31, 17, 2048), (40, 30, 8192), (5, 5, 4096), (120, 68, 16384)]
LAT_C = 192


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_codec.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_ragged_codec_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) == 6
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_CODEC_ABI), "python binding table and sicn_ragged_codec.h disagree"
    assert L.sicn_version() >= 7


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _layout(ws, hs, c, wss, n_images=None, want_images=True):
    """(rc, [RaggedCodecImage], [latent bytes, slot bytes, workspace bytes]); ws / hs / wss: sequences (wss may be None)."""
    L = _lib.lib()
    n = len(ws) if n_images is None else n_images
    images = (_lib.RaggedCodecImage * max(n, 1))() if want_images else None
    totals = (ctypes.c_uint64 * 3)()
    rc = L.sicn_ragged_codec_layout(_u32(ws), _u32(hs), c, _u32(wss) if wss is not None else None, n, images, totals)
    return rc, (list(images)[:max(n, 0)] if want_images else None), [int(v) for v in totals]


def test_layout_equals_plain_arithmetic():
    L = _lib.lib()
    rc, images, totals = _layout([s[0] for s in SHAPES], [s[1] for s in SHAPES], LAT_C, [s[2] for s in SHAPES])
    assert rc == 0
    lat_off = slot_end = ws_end = 0
    for (w, h, wss), im in zip(SHAPES, images):
        n = w * h * LAT_C
        ns = -(-n // wss)
        assert (im.n_symbols, im.n_streams, im.stream_symbols) == (n, ns, wss)
        assert im.latent_offset == lat_off                                   # back to back: the running sum of h * w * c
        lat_off += n
        assert im.slot_bytes == -(-L.sicn_codec_max_bytes_sl(n, wss) // 16) * 16
        assert im.slot_bytes >= 48 + 256 + 4 * ns + 2 * n + 256 * ns
        assert im.slot_offset % 16 == 0 and im.slot_offset >= slot_end        # 16-aligned, no overlap
        slot_end = im.slot_offset + im.slot_bytes
        assert im.workspace_offset % 16 == 0 and im.workspace_offset >= ws_end
        ws_end = im.workspace_offset + L.sicn_codec_workspace_bytes_sl(n, wss) - 64   # the uniform coder's block (it adds 64 spare bytes)
    assert totals[0] == lat_off and totals[1] >= slot_end and totals[1] == sum(im.slot_bytes for im in images)
    assert totals[2] >= ws_end


def test_default_stream_length_is_16384():
    rc, images, _ = _layout([40, 3], [30, 3], LAT_C, None)
    assert rc == 0 and [im.stream_symbols for im in images] == [16384, 16384]
    assert [im.n_streams for im in images] == [-(-40 * 30 * LAT_C // 16384), 1]


def test_equal_shapes_are_the_uniform_batch():
    n = 17 * 9 * LAT_C
    rc, images, totals = _layout([17] * 6, [9] * 6, LAT_C, [8192] * 6)
    assert rc == 0
    assert [im.latent_offset for im in images] == [i * n for i in range(6)]
    assert len({im.slot_bytes for im in images}) == 1 and totals[0] == 6 * n


def test_offsets_are_64_bit():
    """130 images of 2048 streams of 16384 symbols: 4.4 G symbols, 8.7 GB of slots — arithmetic only, nothing is allocated."""
    w, h, c = 4096, 8192, 1                                        # 2^25 symbols = 2048 streams of 16384
    rc, images, totals = _layout([w] * 130, [h] * 130, c, None)
    assert rc == 0
    n = w * h * c
    assert images[-1].latent_offset == 129 * n > 2 ** 32
    assert images[-1].slot_offset == 129 * images[0].slot_bytes > 2 ** 33
    assert totals[0] == 130 * n and totals[1] == 130 * images[0].slot_bytes


def test_limits_are_einval():
    ok = ([4], [4], 4, [1024])
    assert _layout(*ok)[0] == 0
    assert _layout([4], [4], 4, [1024], n_images=0)[0] == EINVAL                      # n_images < 1
    assert _layout([4], [4], 4, [1024], n_images=-3)[0] == EINVAL
    assert _layout([0], [4], 4, [1024])[0] == EINVAL                                  # a latent dimension < 1
    assert _layout([4], [0], 4, [1024])[0] == EINVAL
    assert _layout([4], [4], 0, [1024])[0] == EINVAL
    assert _layout([4, 4, 0], [4, 4, 4], 4, [1024] * 3)[0] == EINVAL                  # ... in any image
    for wss in (0, 1, 512, 1023, 1025, 3000, 12288, 32768, 65536):                    # not a power of two in 1024 .. 16384
        assert _layout([4], [4], 4, [wss])[0] == EINVAL, wss
    for wss in (1024, 2048, 4096, 8192, 16384):
        assert _layout([4], [4], 4, [wss])[0] == 0, wss
    assert _layout([4, 4], [4, 4], 4, [1024, 1000])[0] == EINVAL


def test_more_than_2048_streams_in_one_image_is_einval():
    # 2048 streams of 1024 symbols are the most; one symbol more is a 2049th stream
    assert _layout([2048], [1024], 1, [1024])[0] == 0
    rc, images, _ = _layout([2048], [1024], 1, [1024])
    assert images[0].n_streams == 2048
    assert _layout([2048 * 1024 + 1], [1], 1, [1024])[0] == EINVAL                    # 2049 streams at 1024 symbols
    assert _layout([2049], [1024], 1, [1024])[0] == EINVAL
    assert _layout([2049], [1024], 1, [2048])[0] == 0                                 # the same latent at 2048 symbols: 1025 streams
    assert _layout([2048], [16384], 1, [16384])[0] == 0
    assert _layout([2048], [16384], 2, [16384])[0] == EINVAL
    assert _layout([2 ** 32 - 1], [2 ** 32 - 1], 2 ** 32 - 1, [16384])[0] == EINVAL   # products that would wrap 64 bits
    assert _layout([3, 2049], [3, 1024], 1, [1024, 1024])[0] == EINVAL                # ... in any image


def test_total_streams_limit():
    """2^31 - 1 streams or more in all are refused: 2^20 images of 2048 streams are 2^31 (totals only, nothing is allocated)."""
    per = 2048
    n_ok = (2 ** 31 - 2) // per                                    # 2^20 - 1 images: 2^31 - 2048 streams
    ws = np.full(n_ok + 1, 2048, np.uint32)
    hs = np.full(n_ok + 1, 1024, np.uint32)
    wss = np.full(n_ok + 1, 1024, np.uint32)
    assert _layout(ws, hs, 1, wss, n_images=n_ok, want_images=False)[0] == 0
    assert _layout(ws, hs, 1, wss, n_images=n_ok + 1, want_images=False)[0] == EINVAL


def test_coder_create_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    one = _u32([4])
    assert L.sicn_ragged_coder_create(one, one, 4, _u32([1024]), None, None, 0, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_coder_create(one, one, 4, _u32([1000]), None, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_coder_create(one, one, 4, None, None, None, 1, None) == EINVAL
    assert L.sicn_ragged_coder_workspace_bytes(None) == 0
    L.sicn_ragged_coder_free(None)
    dummy = ctypes.c_void_p(16)
    assert L.sicn_ragged_coder_encode_async(None, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_coder_decode_async(None, dummy, None, dummy, dummy, dummy, 1 << 20, None) == EINVAL


def test_device_tables_under_the_sanitizers(tmp_path):
    """tests/cpp/device_table_check.cpp — csrc/device_table.hpp with host fakes of hipMalloc, hipFree and hipMemcpy and its own
    main — built with the address and undefined-behaviour sanitizers and run as a child process: every allocation and every copy of
    a create fails in its turn and leaves SICN_ENOMEM, a null handle and no live allocation; success and delete, an empty vector, a
    moved-from table, a build that throws std::bad_alloc, the item map against the insert loop, the workspace check."""
    gxx = shutil.which("g++") or shutil.which("c++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "device_table_check"
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([gxx, *flags, str(ROOT / "tests" / "cpp" / "device_table_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|unrecognized.*-fsanitize", r.stderr):
        pytest.skip(f"the compiler cannot link the sanitizer runtime here: {r.stderr.strip().splitlines()[-1]}")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    if r.returncode != 0 and "ASan runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a library preloaded into every process here comes before the sanitizer's runtime, which refuses to start behind it")
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"device_table_check ok: \d+ checks", r.stdout), r.stdout
