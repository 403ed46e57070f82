"""CPU-only checks of the ragged context coder's ABI (include/sicn_ragged_ctx.h): the symbols, the binding table, and
sicn_ragged_ctx_layout — where every latent, container slot and workspace block of a batch of different shapes lies and how every image
is cut into anchor and non-anchor streams — against plain Python arithmetic.  Nothing here touches a device."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from simple_image_compression_network_amd import _lib
from codec_edge_cases import ctx_geometry

ROOT = Path(__file__).resolve().parent.parent
EINVAL = -22
# the batches of tests/test_ragged_ctx_gpu.py: lat_c -> [(lat_h, lat_w)]
BATCHES = {4: [(64, 128), (2, 2), (3, 3), (1, 1), (1, 8193), (1, 1)],
           8: [(5, 1), (1, 5), (2, 3), (1, 1)],
           192: [(37, 37), (1, 1), (3, 5), (12, 16), (2, 7), (1, 2), (2, 1)]}
MAX_SYMBOLS = 0x7F000000        # the uniform coder's limit (csrc/k_codec_body.hpp, MAX_RANS_SYMBOLS)


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged_ctx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_ragged_ctx_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) == 6
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_CTX_ABI), "python binding table and sicn_ragged_ctx.h disagree"
    assert L.sicn_version() >= 9


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32).ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _layout(ws, hs, c, n_images=None, want_images=True):
    """(rc, [RaggedCtxImage], [latent bytes, slot bytes, workspace bytes])."""
    L = _lib.lib()
    n = len(ws) if n_images is None else n_images
    images = (_lib.RaggedCtxImage * max(n, 1))() if want_images else None
    totals = (ctypes.c_uint64 * 3)()
    rc = L.sicn_ragged_ctx_layout(_u32(ws), _u32(hs), c, n, images, totals)
    return rc, (list(images)[:max(n, 0)] if want_images else None), [int(v) for v in totals]


@pytest.mark.parametrize("lat_c", sorted(BATCHES))
def test_layout_equals_plain_arithmetic(lat_c):
    L = _lib.lib()
    shapes = BATCHES[lat_c]
    rc, images, totals = _layout([w for _, w in shapes], [h for h, _ in shapes], lat_c)
    assert rc == 0
    lat_off = slot_end = ws_end = 0
    for (h, w), im in zip(shapes, images):
        n = h * w * lat_c
        (na, nn), (sa, sn) = ctx_geometry(h, w, lat_c)
        assert na + nn == n
        assert (im.n_symbols, im.anchor_streams, im.nonanchor_streams) == (n, sa, sn)
        assert im.latent_offset == lat_off and lat_off % 4 == 0                # back to back: the running sum of h * w * c
        lat_off += n
        assert im.slot_bytes == -(-L.sicn_codec_ctx_max_bytes(w, h, lat_c) // 16) * 16
        assert im.slot_bytes >= 48 + 4096 + 4 * (sa + sn) + 2 * n + 256 * (sa + sn)
        assert im.slot_offset % 16 == 0 and im.slot_offset == slot_end        # 16-aligned, back to back
        slot_end = im.slot_offset + im.slot_bytes
        assert im.workspace_offset % 16 == 0 and im.workspace_offset == ws_end
        ws_end = im.workspace_offset + L.sicn_codec_ctx_workspace_bytes(w, h, lat_c, 1)   # the uniform coder's block
    assert totals == [lat_off, slot_end, ws_end]


def test_image_starts_are_at_4_byte_not_16_byte_multiples():
    shapes = BATCHES[4]
    _, images, _ = _layout([w for _, w in shapes], [h for h, _ in shapes], 4)
    assert all(im.latent_offset % 4 == 0 for im in images) and any(im.latent_offset % 16 for im in images)


def test_equal_shapes_are_the_uniform_batch():
    n = 17 * 9 * 192
    rc, images, totals = _layout([17] * 6, [9] * 6, 192)
    assert rc == 0
    assert [im.latent_offset for im in images] == [i * n for i in range(6)]
    assert len({im.slot_bytes for im in images}) == 1 and totals[0] == 6 * n


def test_offsets_are_64_bit():
    """40 images of 2^27 symbols: 5.4 G symbols, 10.9 GB of slots — arithmetic only, nothing is allocated."""
    w, h, c = 4096, 8192, 4
    rc, images, totals = _layout([w] * 40, [h] * 40, c)
    assert rc == 0
    n = w * h * c
    assert (images[0].anchor_streams, images[0].nonanchor_streams) == (4096, 4096)   # even height: the sets are halves, n / 2 / 16384 streams each
    assert images[-1].latent_offset == 39 * n > 2 ** 32
    assert images[-1].slot_offset == 39 * images[0].slot_bytes > 2 ** 33
    assert images[-1].workspace_offset == 39 * _lib.lib().sicn_codec_ctx_workspace_bytes(w, h, c, 1) > 2 ** 33
    assert totals[0] == 40 * n and totals[1] == 40 * images[0].slot_bytes


def test_limits_are_einval():
    assert _layout([4], [4], 4)[0] == 0
    assert _layout([4], [4], 4, n_images=0)[0] == EINVAL                      # n_images < 1
    assert _layout([4], [4], 4, n_images=-3)[0] == EINVAL
    assert _layout([0], [4], 4)[0] == EINVAL                                  # a latent dimension < 1
    assert _layout([4], [0], 4)[0] == EINVAL
    assert _layout([4], [4], 0)[0] == EINVAL
    assert _layout([4, 4, 0], [4, 4, 4], 4)[0] == EINVAL                      # ... in any image
    for c in (1, 2, 3, 5, 6, 7, 190, 194):                                    # lat_c & 3
        assert _layout([4], [4], c)[0] == EINVAL, c
    for c in (4, 8, 12, 192):
        assert _layout([4], [4], c)[0] == 0, c
    L = _lib.lib()
    totals = (ctypes.c_uint64 * 3)()
    assert L.sicn_ragged_ctx_layout(None, _u32([4]), 4, 1, None, totals) == EINVAL      # a null pointer
    assert L.sicn_ragged_ctx_layout(_u32([4]), None, 4, 1, None, totals) == EINVAL
    assert L.sicn_ragged_ctx_layout(_u32([4]), _u32([4]), 4, 1, None, None) == 0          # both outputs are optional


def test_an_image_above_the_uniform_coders_symbol_limit_is_einval():
    assert MAX_SYMBOLS % 4 == 0
    assert _layout([MAX_SYMBOLS // 4], [1], 4)[0] == 0
    assert _layout([MAX_SYMBOLS // 4 + 1], [1], 4)[0] == EINVAL
    assert _layout([3, MAX_SYMBOLS // 4 + 1], [3, 1], 4)[0] == EINVAL                 # ... in any image
    assert _layout([2 ** 32 - 1], [2 ** 32 - 1], 2 ** 32 - 4)[0] == EINVAL            # products that would wrap 64 bits
    rc, images, _ = _layout([MAX_SYMBOLS // 4], [1], 4)
    assert images[0].slot_bytes > 2 ** 32                                             # such a slot does not fit 32 bits


def test_total_streams_limit():
    """2^31 - 1 streams or more in all are refused: images of 2^15 streams each (totals only, nothing is allocated)."""
    w, h, c = 16384, 8192, 4                                       # 2^29 symbols: 2 x 2^14 streams
    per = 2 ** 15
    n_ok = (2 ** 31 - 2) // per                                    # 2^16 - 1 images: 2^31 - 2^15 streams
    ws, hs = np.full(n_ok + 1, w, np.uint32), np.full(n_ok + 1, h, np.uint32)
    assert _layout(ws, hs, c, n_images=n_ok, want_images=False)[0] == 0
    assert _layout(ws, hs, c, n_images=n_ok + 1, want_images=False)[0] == EINVAL


def test_calls_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    one = _u32([4])
    assert L.sicn_ragged_ctx_coder_create(one, one, 4, None, None, 0, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_coder_create(one, one, 6, None, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_coder_create(one, one, 4, None, None, 1, None) == EINVAL
    assert L.sicn_ragged_ctx_coder_create(None, one, 4, None, None, 1, ctypes.byref(h)) == EINVAL and not h.value
    assert L.sicn_ragged_ctx_coder_workspace_bytes(None) == 0
    L.sicn_ragged_ctx_coder_free(None)
    dummy = ctypes.c_void_p(16)
    assert L.sicn_ragged_ctx_encode_async(None, dummy, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
    assert L.sicn_ragged_ctx_decode_async(None, dummy, None, dummy, dummy, dummy, dummy, 1 << 20, None) == EINVAL
