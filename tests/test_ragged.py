"""CPU-only checks of the ragged-batch ABI (include/sicn_ragged.h): the symbols, the binding table, and sicn_ragged_layout — where
every image of a batch of different sizes sits at every layer boundary and how every layer is cut into work items — against a
pure-Python chain-rule computation.  Nothing here touches a device."""
import ctypes
import re
from dataclasses import replace
from pathlib import Path

import pytest

from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import CLayerDesc, REFERENCE_DESCS, eight_layer_descs

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
EINVAL = -22


def _declared_symbols():
    text = (ROOT / "include" / "sicn_ragged.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicn_ragged_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_ragged_symbol():
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) == 5
    for s in syms:
        assert hasattr(L, s), f"libsicn.so does not export {s}"
    assert set(syms) == set(_lib.RAGGED_ABI), "python binding table and sicn_ragged.h disagree"
    assert L.sicn_version() >= 6


def _layout(descs, sizes, layer, image, n_images=None):
    L = _lib.lib()
    n = len(descs)
    cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
    m = max(len(sizes), 1)
    ws = (ctypes.c_int32 * m)(*[w for w, _ in sizes])
    hs = (ctypes.c_int32 * m)(*[h for _, h in sizes])
    out = (ctypes.c_int64 * 8)()
    rc = L.sicn_ragged_layout(cd, n, ws, hs, len(sizes) if n_images is None else n_images, layer, image, out)
    return rc, list(out)


def _python_layout(descs, sizes):
    """{(layer, image): [W, H, C, offset, tensor bytes, first item, tiles_x, total items]} by the chain rule, in Python integers."""
    res = {}
    cur = [(w, h) for w, h in sizes]
    c = descs[0].IFM_CH
    off = 0
    for i, (w, h) in enumerate(cur):
        res[(-1, i)] = [w, h, c, off, None, 0, 0, 0]
        off += w * h * c
    for i in range(len(cur)):
        res[(-1, i)][4] = off
    for l, d in enumerate(descs):
        nxt = [(2 * w, 2 * h) if d.transposed else (-(-w // 2), -(-h // 2)) for w, h in cur]
        off = first = 0
        for i, ((iw, ih), (ow, oh)) in enumerate(zip(cur, nxt)):
            mw, mh = (iw, ih) if d.transposed else (ow, oh)
            tx, ty = -(-mw // 16), -(-mh // 16)
            res[(l, i)] = [ow, oh, d.OFM_CH, off, None, first, tx, None]
            off += ow * oh * d.OFM_CH
            first += tx * ty * (4 if d.transposed else 1)
        for i in range(len(cur)):
            res[(l, i)][4] = off
            res[(l, i)][7] = first
        cur = nxt
    return res


@pytest.mark.parametrize("widths", [(128, 192), (64, 96)])
def test_layout_equals_the_chain_rule(widths):
    # the spatial fields of the descriptors are ignored: these are the reference's 768 x 512 ones
    descs = eight_layer_descs(768, 512, *widths)
    ref = _python_layout(descs, SIZES)
    for layer in range(-1, 8):
        for i in range(len(SIZES)):
            rc, got = _layout(descs, SIZES, layer, i)
            assert rc == 0
            assert got == ref[(layer, i)], (layer, i)
    # the reconstruction of a 100 x 36 image is 112 x 48 (eight_layer_descs(100, 36))
    d = eight_layer_descs(100, 36)[7]
    assert _layout(descs, SIZES, 7, 4)[1][:3] == [112, 48, 3] == [d.OFM_ROW, d.OFM_COL, d.OFM_CH]
    # equal sizes: the [n][H][W][C] batch
    same = [(37, 21)] * 4
    for layer in range(-1, 8):
        w, h, c = _layout(descs, same, layer, 0)[1][:3]
        assert [_layout(descs, same, layer, i)[1][3] for i in range(4)] == [i * w * h * c for i in range(4)]


def test_item_counts_per_layer():
    descs = eight_layer_descs(768, 512)

    def counts(size):
        return [_layout(descs, [size], l, 0)[1][7] for l in range(8)]
    assert counts((131, 70)) == [15, 6, 2, 1, 4, 8, 24, 60]
    assert counts((100, 36)) == [8, 2, 1, 1, 4, 4, 8, 32]
    # in a batch the images' items follow one another
    both = [(131, 70), (100, 36)]
    assert [_layout(descs, both, l, 1)[1][5] for l in range(8)] == counts((131, 70))
    assert [_layout(descs, both, l, 1)[1][7] for l in range(8)] == [a + b for a, b in zip(counts((131, 70)), counts((100, 36)))]


def test_offsets_above_4_gib_do_not_overflow():
    descs = eight_layer_descs(768, 512)
    sizes = [(8192, 4320)] * 3
    per_image = 4096 * 2160 * 128
    for i in range(3):
        rc, got = _layout(descs, sizes, 0, i)
        assert rc == 0
        assert got[3] == i * per_image and got[4] == 3 * per_image
    assert 2 * per_image > 2 ** 31 and 3 * per_image > 2 ** 31
    sizes = [(8192, 4320)] * 5          # the last image starts above 2^32
    rc, got = _layout(descs, sizes, 0, 4)
    assert rc == 0 and got[3] == 4 * per_image > 2 ** 32
    assert got[5] == 4 * 256 * 135 and got[7] == 5 * 256 * 135


def test_limits_are_einval():
    descs = eight_layer_descs(768, 512)
    # one image whose layer-0 output reaches 2^31 bytes: 4096 x 4096 x 128, from an 8192 x 8192 input (whose own 192 MiB are fine)
    assert _layout(descs[:1], [(8192, 8192)], 0, 0)[0] == EINVAL
    assert _layout(descs[:1], [(8192, 8190)], 0, 0)[0] == 0       # 4096 x 4095 x 128 is just under
    assert _layout(descs, [(8192, 8192)], 0, 0)[0] == EINVAL
    assert _layout(descs, [(16, 16), (8192, 8192)], 0, 0)[0] == EINVAL
    assert _layout(descs, [], -1, 0, n_images=0)[0] == EINVAL
    assert _layout(descs, [(16, 16)], -1, 0, n_images=-1)[0] == EINVAL
    assert _layout(descs, [(16, 16), (0, 5)], -1, 0)[0] == EINVAL
    assert _layout(descs, [(16, 16), (5, 0)], -1, 0)[0] == EINVAL
    assert _layout(descs, [(16, 16), (-3, 5)], -1, 0)[0] == EINVAL
    # a layer the channel-generic kernels do not serve: the ragged net has no other kernel
    odd = replace(REFERENCE_DESCS[1], IFM_CH=6, OFM_CH=4, SIMD=3, PE=2, W_TILES=(4 // 2) * (150 // 3))
    assert _lib.lib().sicn_validate_desc(ctypes.byref(odd.to_c())) == 0
    assert _layout([odd], [(16, 16)], 0, 0)[0] == EINVAL
    # layer / image out of range, a chain whose channels do not meet
    assert _layout(descs, [(16, 16)], 8, 0)[0] == EINVAL
    assert _layout(descs, [(16, 16)], -2, 0)[0] == EINVAL
    assert _layout(descs, [(16, 16)], 0, 1)[0] == EINVAL
    assert _layout([descs[0], descs[3], descs[4]], [(16, 16)], 0, 0)[0] == 0
    assert _layout([descs[0], descs[4]], [(16, 16)], 0, 0)[0] == EINVAL


def test_net_create_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    out = ctypes.c_void_p()
    descs = eight_layer_descs(768, 512)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in descs])
    one = (ctypes.c_int32 * 1)(16)
    zero = (ctypes.c_int32 * 1)(0)
    handles = (ctypes.c_void_p * 8)()
    assert L.sicn_ragged_net_create(cd, handles, 8, one, one, 0, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_net_create(cd, handles, 8, zero, one, 1, ctypes.byref(out)) == EINVAL
    assert L.sicn_ragged_net_create(cd, handles, 8, one, one, 1, ctypes.byref(out)) == EINVAL      # NULL weights
    assert L.sicn_ragged_net_create(cd, None, 8, one, one, 1, ctypes.byref(out)) == EINVAL
    assert not out.value
    assert L.sicn_ragged_net_workspace_bytes(None) == 0
    assert L.sicn_ragged_net_forward(None, 0, 7, None, None, -1, None, None, 0, None) == EINVAL
    L.sicn_ragged_net_free(None)
