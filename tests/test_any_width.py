"""CPU-only checks of the channel-generic MFMA dispatch (csrc/k_mfma16c.hip): which descriptors it serves, what it would launch
on chips of several sizes, and the eight-layer topology at other channel widths.  No GPU is touched."""
import ctypes

import pytest

from simple_image_compression_network_amd import _lib
from simple_image_compression_network_amd.config import LayerDesc, REFERENCE_DESCS, eight_layer_descs


def _simd_pe(cin, cout):
    simd = 3 if cin == 3 else (8 if cin % 8 == 0 else (4 if cin % 4 == 0 else (3 if cin % 3 == 0 else 1)))
    pe = 3 if cout == 3 else (8 if cout % 8 == 0 else (4 if cout % 4 == 0 else 1))
    return simd, pe


def _desc(cin, cout, tr, w=40, h=24):
    simd, pe = _simd_pe(cin, cout)
    return LayerDesc.make(cin, cout, simd, pe, w, h, tr)


def _name(d):
    return _lib.lib().sicn_kernel_for(ctypes.byref(d.to_c())).decode()


BOTH_WAYS = [(64, 64), (192, 192), (256, 256), (192, 320), (320, 192), (96, 64), (352, 48)]


@pytest.mark.parametrize("cin,cout", BOTH_WAYS)
def test_inner_widths_go_to_the_channel_generic_mfma_kernels(cin, cout):
    assert _name(_desc(cin, cout, 0)) == "mfma_conv_any"
    assert _name(_desc(cin, cout, 1)) == "mfma_deconv_any"


def test_rgb_ends_at_other_widths_go_to_the_channel_generic_mfma_kernels():
    for cout in (192, 16):
        assert _name(_desc(3, cout, 0)) == "mfma_conv_any"
    for cin in (64, 320):
        assert _name(_desc(cin, 3, 1)) == "mfma_deconv_any"
    # the other direction of an RGB end is nobody's special case
    assert _name(_desc(3, 192, 1)) == "generic"
    assert _name(_desc(64, 3, 0)) == "generic"


def test_reference_and_hyperprior_shapes_keep_their_kernels():
    kinds = [_name(d) for d in REFERENCE_DESCS]
    assert kinds == ["l0_rgb", "mfma_conv", "mfma_conv", "mfma_conv", "mfma_deconv", "mfma_deconv", "mfma_deconv", "l7_rgb"]
    assert _name(_desc(192, 128, 0)) == "mfma_conv"
    assert _name(_desc(128, 192, 1)) == "mfma_deconv"
    assert _name(_desc(128, 128, 0)) == "mfma_conv" and _name(_desc(128, 128, 1)) == "mfma_deconv"


@pytest.mark.parametrize("cin,cout", [(6, 4), (3, 8), (12, 3), (48, 40), (32, 24), (1056, 64)])
def test_small_and_ragged_shapes_stay_on_the_generic_kernel(cin, cout):
    for tr in (0, 1):
        assert _name(_desc(cin, cout, tr)) == "generic"


def _plan(d, n_images, n_cu, **opts):
    out = (ctypes.c_int32 * 12)()
    o = _lib.make_options(**opts)
    rc = _lib.lib().sicn_debug_plan(ctypes.byref(d.to_c()), n_images, ctypes.byref(o), n_cu, out)
    return rc, list(out)


@pytest.mark.parametrize("n_cu", [256, 128, 32])
def test_debug_plan_reports_the_new_kinds_and_a_grid(n_cu):
    for tr, kind in ((0, 5), (1, 6)):
        d = _desc(192, 320, tr, w=100, h=37)
        rc, p = _plan(d, 3, n_cu)
        assert rc == 0 and p[0] == n_cu and p[2] == kind
        m_w, m_h = (d.IFM_ROW, d.IFM_COL) if tr else (d.OFM_ROW, d.OFM_COL)
        tiles = ((m_w + 15) // 16) * ((m_h + 15) // 16)
        assert p[4] == 16 and p[7] == tiles * (4 if tr else 1) and p[8] == 5 and p[9] == 3
        rc, p = _plan(d, 3, n_cu, force_generic=1)
        assert rc == 0 and p[2] == 0
    rc, p = _plan(_desc(3, 192, 0), 1, n_cu)
    assert rc == 0 and p[2] == 5 and p[7] > 0 and p[8] == 3 and p[9] == 1
    rc, p = _plan(_desc(320, 3, 1), 1, n_cu)
    assert rc == 0 and p[2] == 6 and p[7] > 0 and p[8] == 1 and p[9] == 1


def test_version_says_the_dispatch_changed():
    assert _lib.lib().sicn_version() >= 5


# nets whose layers come from both kinds of family (tests/test_any_width_gpu.py runs them): the dispatch, pinned
MIXED_DISPATCH = {
    (128, 256): ["l0_rgb", "mfma_conv", "mfma_conv", "mfma_conv_any", "mfma_deconv_any", "mfma_deconv", "mfma_deconv", "l7_rgb"],
    (192, 128): ["mfma_conv_any", "mfma_conv_any", "mfma_conv_any", "mfma_conv", "mfma_deconv", "mfma_deconv_any", "mfma_deconv_any",
                 "mfma_deconv_any"],
    (128, 64): ["l0_rgb", "mfma_conv", "mfma_conv", "mfma_conv_any", "mfma_deconv_any", "mfma_deconv", "mfma_deconv", "l7_rgb"],
}


def _mixed_links(names):
    """links that join a specialised family to a channel-generic one (the tensor changes between an internal layout and NHWC)"""
    return sum(a.endswith("_any") != b.endswith("_any") for a, b in zip(names, names[1:]))


@pytest.mark.parametrize("size", [(96, 64), (250, 131), (1920, 1080)])
def test_dispatch_of_the_nets_that_mix_kernel_families(size):
    for widths, want in MIXED_DISPATCH.items():
        assert [_name(d) for d in eight_layer_descs(size[0], size[1], *widths)] == want, widths
    # every width pair the GPU tests run: how many links join the two kinds of family
    links = {widths: _mixed_links([_name(d) for d in eight_layer_descs(size[0], size[1], *widths)])
             for widths in [(64, 96), (192, 320), (256, 256), (128, 256), (192, 128), (128, 64), (128, 192)]}
    assert links == {(64, 96): 0, (192, 320): 0, (256, 256): 0, (128, 256): 2, (192, 128): 2, (128, 64): 2, (128, 192): 0}


def test_wide_channel_counts_are_served_up_to_1024():
    for cin, cout, tr in ((1024, 1024, 0), (992, 1008, 1), (512, 640, 0), (640, 512, 1), (1024, 16, 0), (32, 1024, 1), (704, 448, 0),
                          (448, 704, 1), (512, 512, 0)):
        assert _name(_desc(cin, cout, tr)) == ("mfma_deconv_any" if tr else "mfma_conv_any")
    assert _name(LayerDesc.make(3, 1024, 3, 16, 37, 21, 0)) == "mfma_conv_any"
    assert _name(LayerDesc.make(1024, 3, 16, 3, 18, 7, 1)) == "mfma_deconv_any"
    assert _name(_desc(1056, 1024, 0)) == "generic" and _name(_desc(1024, 1040, 1)) == "generic"


def test_eight_layer_descs_at_other_widths():
    assert eight_layer_descs(768, 512) == REFERENCE_DESCS
    assert eight_layer_descs(768, 512, 128, 192) == REFERENCE_DESCS
    L = _lib.lib()
    for (w, h) in ((96, 64), (250, 131), (1920, 1080)):
        for n_ch, m_ch in ((192, 320), (64, 96), (256, 256)):
            descs = eight_layer_descs(w, h, n_ch, m_ch)
            assert len(descs) == 8
            assert [d.transposed for d in descs] == [0, 0, 0, 0, 1, 1, 1, 1]
            assert (descs[0].IFM_CH, descs[0].IFM_ROW, descs[0].IFM_COL) == (3, w, h)
            assert descs[3].OFM_CH == m_ch and descs[7].OFM_CH == 3
            assert all(d.OFM_CH == n_ch for i, d in enumerate(descs) if i not in (3, 7))
            for i, d in enumerate(descs):
                d.validate()
                assert L.sicn_validate_desc(ctypes.byref(d.to_c())) == 0
                if i:
                    p = descs[i - 1]
                    assert (d.IFM_CH, d.IFM_ROW, d.IFM_COL) == (p.OFM_CH, p.OFM_ROW, p.OFM_COL)
                assert _name(d) not in ("generic", "invalid"), (i, d)
    with pytest.raises(ValueError):
        eight_layer_descs(96, 64, 100, 192)
