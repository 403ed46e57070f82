"""GPU parity of the channel-generic MFMA kernels (csrc/k_mfma16c.hip; run with -m gpu on an MI355X): conv2d<> / deconv522<> at
channel widths the reference net does not instantiate, against the oracle and against k_generic — byte equality, the path is
integer.  Every case first asserts that the layer is NOT served by k_generic, so none of them can pass without the kernels."""
import ctypes
import os

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_mk_desc = LayerDesc.make


def _rand_params(rng, d):
    W = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
    b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
    return W, b, sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE)


def _kernel(api, d):
    return api._lib.lib().sicn_kernel_for(ctypes.byref(d.to_c())).decode()


def _assert_any(api, d):
    assert _kernel(api, d) == ("mfma_deconv_any" if d.transposed else "mfma_conv_any")


def _run_layer(api, d, words, b, x_np, gdn=None, **options):
    fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words)
    fn = api.deconv522 if d.transposed else api.conv2d
    out = fn(d, fpw, b, _dev(x_np), None, x_np.shape[0], options=options or None, gdn=gdn)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _input(rng, d, n):
    """Bytes 0 .. 127 as a ReLU layer produces them, every seventh byte of image 0 lifted to 128 .. 227: values the net never
    produces must still be exact mod 256 (the kernels read them as negative int8).  227, not 255: the numpy reference sums in
    float32 and asserts 25 * IFM_CH * max(x) * 8 < 2^24 (sicn_ref._exact_gemm_ok), which at 352 channels allows max(x) <= 238."""
    if d.IFM_CH == 3:
        return rng.integers(0, 256, (n,) + d.in_shape, dtype=np.uint8)
    x = rng.integers(0, 128, (n,) + d.in_shape, dtype=np.uint8)
    flat = x[0].reshape(-1)
    flat[::7] = 128 + flat[::7] % 100
    return x


# (cin, cout, simd, pe, w, h, transposed)
TIER_A = [
    (32, 16, 8, 16, 37, 21, 0), (64, 64, 8, 16, 66, 18, 0), (64, 96, 8, 16, 7, 5, 0), (96, 64, 12, 16, 1, 1, 0),
    (160, 160, 8, 16, 40, 22, 0), (192, 192, 12, 24, 65, 3, 0), (256, 256, 8, 16, 131, 33, 0), (192, 320, 8, 16, 45, 19, 0),
    (320, 192, 16, 16, 33, 9, 0), (128, 64, 8, 16, 70, 17, 0), (352, 48, 16, 16, 19, 40, 0),
    (32, 16, 8, 16, 21, 13, 1), (64, 64, 8, 16, 34, 10, 1), (96, 64, 12, 16, 3, 2, 1), (64, 96, 8, 16, 1, 1, 1),
    (160, 160, 8, 16, 37, 21, 1), (192, 192, 12, 24, 65, 19, 1), (256, 256, 8, 16, 70, 17, 1), (320, 192, 16, 16, 33, 9, 1),
    (192, 320, 8, 16, 9, 40, 1), (64, 128, 8, 16, 47, 18, 1), (352, 48, 16, 16, 19, 7, 1),
]
TIER_B = [
    (3, 64, 3, 8, 70, 38, 0), (3, 192, 3, 8, 129, 17, 0), (3, 16, 3, 8, 5, 3, 0), (3, 256, 1, 128, 64, 2, 0),
    (3, 320, 3, 16, 140, 150, 0), (64, 3, 8, 3, 35, 11, 1), (192, 3, 8, 3, 1, 1, 1), (256, 3, 16, 1, 33, 8, 1),
    (32, 3, 8, 3, 70, 9, 1), (320, 3, 16, 3, 70, 45, 1),
]


@pytest.mark.parametrize("case", TIER_A + TIER_B)
def test_layer_matches_oracle_random_weights(api, case):
    rng = np.random.default_rng([7] + list(case))
    d = _mk_desc(*case)
    _assert_any(api, d)
    W, b, words = _rand_params(rng, d)
    n = 2
    x = _input(rng, d, n)
    got = _run_layer(api, d, words, b, x)
    ref_fn = sicn_ref.deconv522_ref if d.transposed else sicn_ref.conv2d_ref
    for i in range(n):
        ref = ref_fn(x[i], W, b)
        assert got[i].shape == ref.shape
        assert np.array_equal(got[i], ref), f"image {i}: {np.count_nonzero(got[i] != ref)} of {ref.size} bytes differ"


# Widths the numpy reference cannot take (its float32 GEMM is exact only while 25 * IFM_CH * max(x) * 8 < 2^24): up to the 1024
# channels any_supported() serves — the longest K walks, up to 16 blocks of 64 output channels in grid.y,
# OFM_CH = 16 (mod 64) near the top (1008), an odd multiple of 32 near the top (992), the RGB ends at 1024, one-pixel layers —
# against the C oracle's direct form, which is integer arithmetic, with input bytes over all of 0 .. 255.
TIER_WIDE = [
    (1024, 1024, 16, 16, 19, 9, 0), (992, 1008, 16, 16, 17, 5, 1), (512, 640, 8, 16, 33, 18, 0), (640, 512, 16, 16, 20, 11, 1),
    (3, 1024, 3, 16, 37, 21, 0), (1024, 3, 16, 3, 18, 7, 1), (1024, 16, 16, 16, 33, 17, 0), (32, 1024, 8, 16, 18, 33, 1),
    (704, 448, 16, 16, 1, 1, 0), (448, 704, 16, 16, 1, 1, 1),
]
# three TIER_A cases again with the 227 cap lifted
TIER_A_FULL_RANGE = [(256, 256, 8, 16, 131, 33, 0), (352, 48, 16, 16, 19, 7, 1), (192, 320, 8, 16, 9, 40, 1)]
ORACLE_THREADS = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("case", TIER_WIDE + TIER_A_FULL_RANGE)
def test_wide_layer_matches_the_exact_oracle_on_full_range_bytes(api, case):
    rng = np.random.default_rng([37] + list(case))
    d = _mk_desc(*case)
    _assert_any(api, d)
    _, b, words = _rand_params(rng, d)
    n = 2
    x = rng.integers(0, 256, (n,) + d.in_shape, dtype=np.uint8)
    got = _run_layer(api, d, words, b, x)
    for i in range(n):
        ref = c_oracle.run_layer(d, words, b, x[i], "direct", threads=ORACLE_THREADS)
        assert np.count_nonzero(ref) > ref.size // 8            # not a comparison of zeros
        assert got[i].shape == ref.shape
        assert np.array_equal(got[i], ref), f"image {i}: {np.count_nonzero(got[i] != ref)} of {ref.size} bytes differ"


@pytest.mark.parametrize("case", [(256, 256, 8, 16, 480, 270, 0), (192, 320, 8, 16, 480, 270, 0),
                                  (256, 256, 8, 16, 240, 135, 1), (192, 320, 8, 16, 240, 135, 1)])
def test_full_chip_grid_agrees_with_the_generic_kernel(api, case):
    """More workgroups than CUs on both sides; the two GPU implementations share no code."""
    rng = np.random.default_rng([11] + list(case))
    d = _mk_desc(*case)
    _assert_any(api, d)
    _, b, words = _rand_params(rng, d)
    x = _input(rng, d, 1)
    fast = _run_layer(api, d, words, b, x)
    slow = _run_layer(api, d, words, b, x, force_generic=1)
    assert np.count_nonzero(fast) > fast.size // 8           # not a comparison of zeros
    assert np.array_equal(fast, slow), f"{np.count_nonzero(fast != slow)} of {fast.size} bytes differ"


@pytest.mark.parametrize("case", [(64, 64, 8, 16, 50, 20, 0), (192, 192, 12, 24, 21, 13, 1), (512, 512, 16, 16, 20, 11, 0)])
def test_pre_activation_mode_with_a_gdn(api, case):
    """relu off: the layer stores the raw byte and the GDN of matching width rewrites it (k_gdn_generic, NHWC)."""
    from simple_image_compression_network_amd.hyperprior import random_gdn_params
    rng = np.random.default_rng([13] + list(case))
    d = _mk_desc(*case)
    _assert_any(api, d)
    _, b, words = _rand_params(rng, d)
    beta, gamma = random_gdn_params(rng, d.OFM_CH)
    inverse = bool(d.transposed)
    x = _input(rng, d, 2) if d.IFM_CH <= 352 else rng.integers(0, 256, (2,) + d.in_shape, dtype=np.uint8)
    got = _run_layer(api, d, words, b, x, gdn=api.GDN(beta, gamma, inverse=inverse, shift=12))
    for i in range(2):
        pre = c_oracle.run_layer_preact(d, words, b, x[i], threads=ORACLE_THREADS)
        assert np.count_nonzero(pre & 0x80) > pre.size // 8   # the lanes the ReLU would have cleared are there
        ref = c_oracle.gdn(pre, beta, gamma, inverse, 12)
        assert np.array_equal(got[i], ref), f"image {i}: {np.count_nonzero(got[i] != ref)} bytes differ"


def _random_net(api, descs, seed):
    from simple_image_compression_network_amd.hyperprior import random_layer_params
    rng = np.random.default_rng(seed)
    params, words, biases = [], [], []
    for d in descs:
        (fw, fb), (w, b) = random_layer_params(rng, d)
        params.append((fw, fb))
        words.append(sicn_ref.pack_finn_tiles(w, d.SIMD, d.PE))
        biases.append(b)
    return api.EightLayersNet(descs=descs, params=params), words, biases


@pytest.mark.parametrize("size", [(96, 64), (250, 131)])
@pytest.mark.parametrize("widths", [(64, 96), (192, 320), (256, 256)])
def test_whole_net_at_other_widths(api, widths, size):
    descs = eight_layer_descs(size[0], size[1], *widths)
    names = [_kernel(api, d) for d in descs]
    assert "generic" not in names and "invalid" not in names, names
    assert names[0] == "mfma_conv_any" and names[7] == "mfma_deconv_any"
    net, words, biases = _random_net(api, descs, [17, *widths, *size])
    x = np.random.default_rng([19, *size]).integers(0, 256, (1, size[1], size[0], 3), dtype=np.uint8)
    out, latent = net.forward(_dev(x))
    torch.cuda.synchronize()
    ref = c_oracle.run_net(descs, words, biases, x[0], form="direct")
    assert np.count_nonzero(ref[3]) > ref[3].size // 8
    assert np.array_equal(latent[0].cpu().numpy(), ref[3]), "latent differs from the oracle"
    assert np.array_equal(out[0].cpu().numpy(), ref[7]), "reconstruction differs from the oracle"


def test_whole_net_captured_and_replayed(api):
    w, h, widths = 96, 64, (192, 320)
    descs = eight_layer_descs(w, h, *widths)
    assert "generic" not in [_kernel(api, d) for d in descs]
    net, words, biases = _random_net(api, descs, 23)
    rng = np.random.default_rng(29)
    xin = _dev(rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8))
    out = torch.empty((1,) + descs[7].out_shape, dtype=torch.uint8, device="cuda")
    lat = torch.empty((1,) + descs[3].out_shape, dtype=torch.uint8, device="cuda")
    graph = net.capture(xin, out, lat)
    for _ in range(2):
        x = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        xin.copy_(_dev(x))
        out.zero_()
        lat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref = c_oracle.run_net(descs, words, biases, x[0], form="direct")
        assert np.array_equal(lat[0].cpu().numpy(), ref[3])
        assert np.array_equal(out[0].cpu().numpy(), ref[7])


# ---- nets that mix the specialised kernel families with the channel-generic ones -------------------------------------------------
# l0_rgb / mfma_conv / mfma_deconv / l7_rgb exchange tensors in the internal GROUP / PHASE layouts, the *_any kernels read and
# write NHWC only, and link_layout (sicn_abi.hip) picks the layout of every link from the family rows.  In the nets above every
# layer is an *_any kernel; in these a GROUP-writing kernel feeds an NHWC-only one and back.
MIXED_WIDTHS = [(128, 256), (192, 128), (128, 64)]


def _mixed_links(names):
    return sum(a.endswith("_any") != b.endswith("_any") for a, b in zip(names, names[1:]))


def _assert_prefixes(net, xin, ref_layers, what):
    """Every prefix 0 .. l of the chain against the reference's layer l (ref_layers[image][l]): the last layer of a call writes NHWC,
    every link in front of it carries the layout the chain picked, so a wrong link names its layer."""
    for l in range(len(net.descs)):
        got, _ = net.run_layers(0, l, xin)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for i, ref in enumerate(ref_layers):
            assert np.array_equal(got[i], ref[l]), \
                f"{what}: layers 0..{l}, image {i}: {np.count_nonzero(got[i] != ref[l])} of {ref[l].size} bytes differ"


@pytest.mark.parametrize("size", [(96, 64), (250, 131)])
@pytest.mark.parametrize("widths", MIXED_WIDTHS)
def test_mixed_family_net_matches_oracle_layer_by_layer(api, widths, size):
    descs = eight_layer_descs(size[0], size[1], *widths)
    names = [_kernel(api, d) for d in descs]
    assert "generic" not in names and "invalid" not in names, names
    assert _mixed_links(names) == 2, names
    net, words, biases = _random_net(api, descs, [43, *widths, *size])
    x = np.random.default_rng([47, *widths, *size]).integers(0, 256, (2, size[1], size[0], 3), dtype=np.uint8)
    xin = _dev(x)
    ref = [c_oracle.run_net(descs, words, biases, x[i], form="direct", threads=ORACLE_THREADS) for i in range(2)]
    assert all(np.count_nonzero(r[3]) > r[3].size // 8 and np.count_nonzero(r[7]) > r[7].size // 8 for r in ref)
    _assert_prefixes(net, xin, ref, f"{widths} {size}")
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(latent[i].cpu().numpy(), ref[i][3]), f"image {i}: latent differs from the oracle"
        assert np.array_equal(out[i].cpu().numpy(), ref[i][7]), f"image {i}: reconstruction differs from the oracle"


def test_mixed_family_net_captured_and_replayed(api):
    w, h, widths = 250, 131, (128, 256)
    descs = eight_layer_descs(w, h, *widths)
    assert _mixed_links([_kernel(api, d) for d in descs]) == 2
    net, words, biases = _random_net(api, descs, 53)
    rng = np.random.default_rng(59)
    xin = _dev(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8))
    out = torch.empty((2,) + descs[7].out_shape, dtype=torch.uint8, device="cuda")
    lat = torch.empty((2,) + descs[3].out_shape, dtype=torch.uint8, device="cuda")
    graph = net.capture(xin, out, lat)
    for _ in range(2):
        x = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        xin.copy_(_dev(x))
        out.zero_()
        lat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for i in range(2):
            ref = c_oracle.run_net(descs, words, biases, x[i], form="direct", threads=ORACLE_THREADS)
            assert np.array_equal(lat[i].cpu().numpy(), ref[3])
            assert np.array_equal(out[i].cpu().numpy(), ref[7])


@pytest.mark.parametrize("igdn_on_layer_7", [False, True], ids=["relu_on_7", "igdn_on_7"])
def test_mixed_family_net_with_activations(api, igdn_on_layer_7):
    """A (128, 256) net with a GDN behind layers 0 .. 2 and an IGDN behind 4 .. 6, as hyperprior.py builds them: the activation
    kernel rewrites the lanes in whatever layout the layer wrote — GROUP behind layers 0 and 1, NHWC behind 2 and 4, PHASE or
    GROUP behind 5 and 6.  With an IGDN on layer 7 as well, l7_rgb (the only family that cannot store the lane before the ReLU)
    gives way to the generic kernel, and the link in front of it changes to NHWC."""
    from simple_image_compression_network_amd.hyperprior import random_gdn_params, random_layer_params
    w, h, widths = 96, 64, (128, 256)
    descs = eight_layer_descs(w, h, *widths)
    names = [_kernel(api, d) for d in descs]
    assert names == ["l0_rgb", "mfma_conv", "mfma_conv", "mfma_conv_any", "mfma_deconv_any", "mfma_deconv", "mfma_deconv", "l7_rgb"]
    rng = np.random.default_rng([61, int(igdn_on_layer_7)])
    params, words, biases, gdns, gdn_np = [], [], [], [], []
    for l, d in enumerate(descs):
        (fw, fb), (wt, bt) = random_layer_params(rng, d)
        params.append((fw, fb))
        words.append(sicn_ref.pack_finn_tiles(wt, d.SIMD, d.PE))
        biases.append(bt)
        if l in (0, 1, 2, 4, 5, 6) or (l == 7 and igdn_on_layer_7):
            beta, gamma = random_gdn_params(rng, d.OFM_CH)
            gdn_np.append((beta, gamma, l >= 4))
            gdns.append(api.GDN(beta, gamma, inverse=l >= 4, shift=12))
        else:
            gdn_np.append(None)
            gdns.append(None)
    net = api.EightLayersNet(descs=descs, params=params, gdn=gdns)
    x = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ref = []
    for i in range(2):
        a, layers = x[i], []
        for l, d in enumerate(descs):
            if gdn_np[l] is None:
                a = c_oracle.run_layer(d, words[l], biases[l], a, "direct", threads=ORACLE_THREADS)
            else:
                beta, gamma, inverse = gdn_np[l]
                a = c_oracle.gdn(c_oracle.run_layer_preact(d, words[l], biases[l], a, threads=ORACLE_THREADS), beta, gamma, inverse, 12)
            layers.append(a)
        ref.append(layers)
    assert all(np.count_nonzero(r[3]) > r[3].size // 8 and np.count_nonzero(r[7]) > r[7].size // 8 for r in ref)
    xin = _dev(x)
    _assert_prefixes(net, xin, ref, "activations" + (" + IGDN on layer 7" if igdn_on_layer_7 else ""))
    out, latent = net.forward(xin)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(latent[i].cpu().numpy(), ref[i][3]), f"image {i}: latent differs from the oracle"
        assert np.array_equal(out[i].cpu().numpy(), ref[i][7]), f"image {i}: reconstruction differs from the oracle"


def test_batch_is_a_true_batch(api):
    d = _mk_desc(160, 160, 8, 16, 66, 18, 0)
    _assert_any(api, d)
    rng = np.random.default_rng(31)
    _, b, words = _rand_params(rng, d)
    x = _input(rng, d, 5)
    together = _run_layer(api, d, words, b, x)
    for i in range(5):
        alone = _run_layer(api, d, words, b, x[i:i + 1])
        assert np.array_equal(together[i], alone[0]), i
    assert len({together[i].tobytes() for i in range(5)}) == 5
