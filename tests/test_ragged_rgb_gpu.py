"""GPU parity of the packed RGB ends of a ragged net (include/sicn_ragged_rgb.h, csrc/k_ragged_rgb.hip; run with -m gpu on an MI355X):
conv 3 -> N and deconv N -> 3 on the packed-K kernels.  Everything is byte equality — the path is integer — against (a) the GENERIC
net on the same weight handles and (b) the C oracle's direct form.  Random weights and biases and full-range bytes; small images
throughout.  Every library call of this file runs between guard bands of 256 patterned bytes on both sides of `out` and `tap_out`,
over outputs that were filled with random bytes, so that a byte written outside and a byte not written both show."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import LayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
# conv 3 -> N: the four leading images leave the next one at byte phases 3, 1, 2, 1; odd and even widths; tile edges at 31 / 32 / 33
# (16 / 16 / 17 output positions); more than one tile in both directions
CONV_SIZES = [(1, 1), (2, 1), (1, 3), (3, 3), (31, 31), (32, 32), (33, 33), (31, 33), (33, 32), (32, 31), (65, 35),
              (1, 1), (33, 1), (2, 67), (100, 36), (131, 70)]
DECONV_SIZES = [(1, 1), (16, 16), (17, 15), (15, 17), (33, 2), (2, 33), (18, 18), (50, 18)]
TINY = [(8, 8), (1, 1), (7, 5), (3, 8), (5, 2)]
GUARD = 256
PATTERN = ((np.arange(GUARD) * 37 + 11) & 255).astype(np.uint8)
KERNELS = {"generic": ["mfma_conv_any"] * 4 + ["mfma_deconv_any"] * 4,
           "packed": ["mfma_conv_rgb_packed"] + ["mfma_conv_any"] * 3 + ["mfma_deconv_any"] * 3 + ["mfma_deconv_rgb_packed"]}


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _weights_of(api, d, rng):
    """Random nibble weights and bias for descriptor `d`: (device handle, oracle words, bias)."""
    W = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
    b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
    words = sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE)
    return api.DeviceWeights(d, api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words), b), words, b


def _conv_desc(n, w=16, h=16):
    return LayerDesc.make(3, n, 3, 8, w, h, 0)


def _deconv_desc(n, w=16, h=16):
    return LayerDesc.make(n, 3, 8, 3, w, h, 1)


@pytest.fixture(scope="module")
def eight(api):
    """The eight layers at (128, 192) with random weights: (device handles, [(words, bias)])."""
    rng = np.random.default_rng([211, 128, 192])
    made = [_weights_of(api, d, rng) for d in eight_layer_descs(16, 16)]
    return [m[0] for m in made], [(m[1], m[2]) for m in made]


def _guarded(api, net, first, last, xin, tap_layer=-1, stream=None):
    """sicn_ragged_net_forward into buffers between guard bands, over random bytes; returns (out, tap or None) without the bands."""
    def buf(n):
        t = torch.randint(0, 256, (n + 2 * GUARD,), dtype=torch.uint8, device="cuda")
        t[:GUARD] = torch.from_numpy(PATTERN).cuda()
        t[-GUARD:] = torch.from_numpy(PATTERN).cuda()
        return t
    out = buf(net.nbytes(last))
    tap = buf(net.nbytes(tap_layer)) if tap_layer >= 0 else None
    ws = net.workspace()
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = api._lib.lib().sicn_ragged_net_forward(net._h, first, last, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr() + GUARD),
                                                tap_layer, ctypes.c_void_p(tap.data_ptr() + GUARD if tap is not None else 0),
                                                ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    pat = torch.from_numpy(PATTERN).cuda()
    for name, t in (("out", out), ("tap_out", tap)):
        if t is not None:
            assert torch.equal(t[:GUARD], pat), f"bytes in front of {name} were written"
            assert torch.equal(t[-GUARD:], pat), f"bytes behind {name} were written"
    return out[GUARD:-GUARD], (tap[GUARD:-GUARD] if tap is not None else None)


def _pack_random(net, rng, layer=-1):
    xs = [rng.integers(0, 256, shp, dtype=np.uint8) for shp in net.shapes(layer)]
    return xs, net.pack([torch.from_numpy(x) for x in xs], layer)


def _check_single_layer(api, mk, sizes, seed):
    """One-layer nets of both forms on one weight handle, one call each: PACKED == GENERIC == the oracle's direct form per image."""
    rng = np.random.default_rng(seed)
    dev, words, bias = _weights_of(api, mk(), rng)
    nets = {form: api.RaggedNet(sizes, shared_weights=[dev], descs=[mk()], rgb_ends=form) for form in ("packed", "generic")}
    want = "mfma_deconv_rgb_packed" if mk().transposed else "mfma_conv_rgb_packed"
    assert nets["packed"].kernel_for(0) == want and nets["generic"].kernel_for(0) == want.replace("rgb_packed", "any")
    xs, xin = _pack_random(nets["packed"], rng)
    got = {form: _guarded(api, net, 0, 0, xin)[0] for form, net in nets.items()}
    assert torch.equal(got["packed"], got["generic"]), "PACKED differs from GENERIC"
    nonzero = 0
    for i, (x, v) in enumerate(zip(xs, nets["packed"].views(0, got["packed"]))):
        ref = c_oracle.run_layer(mk(sizes[i][0], sizes[i][1]), words, bias, x, "direct", threads=16)
        g = v.cpu().numpy()
        assert g.shape == ref.shape, (i, g.shape, ref.shape)
        assert np.array_equal(g, ref), f"image {i} {sizes[i]}: {np.count_nonzero(g != ref)} of {ref.size} bytes differ from the oracle"
        nonzero += np.count_nonzero(ref)
    assert nonzero > got["packed"].numel() // 8          # not a comparison of zeros
    return nets["packed"]


@pytest.mark.parametrize("n", [16, 64, 80, 128, 192])
def test_conv_rgb_alone_every_byte_phase_and_tile_edge(api, n):
    net = _check_single_layer(api, lambda w=16, h=16: _conv_desc(n, w, h), CONV_SIZES, [223, n])
    starts = {o % 4 for o in net._offsets[0]}
    rows = {(o + 3 * w * y) % 4 for o, (w, h) in zip(net._offsets[0], CONV_SIZES) for y in range(min(h, 4))}
    assert starts == {0, 1, 2, 3} and rows == {0, 1, 2, 3}          # every byte phase of an image's start and of a row's start


def test_conv_rgb_1024_channels(api):
    _check_single_layer(api, lambda w=16, h=16: _conv_desc(1024, w, h), TINY, [227])


@pytest.mark.parametrize("n", [32, 64, 96, 128, 192])
def test_deconv_rgb_alone(api, n):
    """96: a half-empty last K chunk."""
    _check_single_layer(api, lambda w=16, h=16: _deconv_desc(n, w, h), DECONV_SIZES, [229, n])


def test_deconv_rgb_1024_channels(api):
    _check_single_layer(api, lambda w=16, h=16: _deconv_desc(1024, w, h), TINY, [233])


def test_activations_behind_and_in_front_of_the_rgb_ends(api):
    """conv 3 -> 128 + GDN (the kernel stores raw lanes) then conv 128 -> 128; deconv 128 -> 128 + IGDN then deconv 128 -> 3 + IGDN."""
    from simple_image_compression_network_amd import hyperprior
    rng = np.random.default_rng(239)
    d8 = eight_layer_descs(16, 16)
    for descs, inverse, sizes in (([d8[0], d8[1]], False, CONV_SIZES[:8]), ([d8[6], d8[7]], True, DECONV_SIZES[:7])):
        made = [_weights_of(api, d, rng) for d in descs]
        params = [hyperprior.random_gdn_params(rng, d.OFM_CH) for d in descs]
        gdn = [api.GDN(p[0], p[1], inverse=inverse, shift=12) for p in params]
        if not inverse:
            gdn[1] = None
        nets = {form: api.RaggedNet(sizes, shared_weights=[m[0] for m in made], descs=descs, gdn=gdn, rgb_ends=form)
                for form in ("packed", "generic")}
        assert [nets["packed"].kernel_for(l) for l in range(2)] == (["mfma_deconv_any", "mfma_deconv_rgb_packed"] if inverse else
                                                                     ["mfma_conv_rgb_packed", "mfma_conv_any"])
        xs, xin = _pack_random(nets["packed"], rng)
        got = {form: _guarded(api, net, 0, 1, xin, tap_layer=0) for form, net in nets.items()}
        assert torch.equal(got["packed"][0], got["generic"][0]) and torch.equal(got["packed"][1], got["generic"][1])
        # the oracle: lanes before the ReLU, then the activation
        net = nets["packed"]
        taps, outs = net.views(0, got["packed"][1]), net.views(1, got["packed"][0])
        for i, x in enumerate(xs):
            cur = x
            for l, (d, m, p, g) in enumerate(zip(descs, made, params, gdn)):
                dl = LayerDesc.make(d.IFM_CH, d.OFM_CH, d.SIMD, d.PE, cur.shape[1], cur.shape[0], d.transposed)
                if g is None:
                    cur = c_oracle.run_layer(dl, m[1], m[2], cur, "direct", threads=16)
                else:
                    cur = c_oracle.gdn(c_oracle.run_layer_preact(dl, m[1], m[2], cur, threads=16), p[0], p[1], inverse, 12)
                have = (taps if l == 0 else outs)[i].cpu().numpy()
                assert np.array_equal(have, cur), f"image {i} {sizes[i]}, layer {l}: differs from the oracle"


def _forward_both(api, dev, sizes, images):
    res = {}
    for form in ("packed", "generic"):
        net = api.RaggedNet(sizes, shared_weights=dev, rgb_ends=form)
        assert [net.kernel_for(l) for l in range(8)] == KERNELS[form]
        out, lat = _guarded(api, net, 0, 7, net.pack([torch.from_numpy(x) for x in images]), tap_layer=3)
        res[form] = (out, lat, net)
    assert torch.equal(res["packed"][0], res["generic"][0]), "reconstruction: PACKED differs from GENERIC"
    assert torch.equal(res["packed"][1], res["generic"][1]), "latent: PACKED differs from GENERIC"
    out, lat, net = res["packed"]
    return [v.cpu().numpy() for v in net.views(7, out)], [v.cpu().numpy() for v in net.views(3, lat)]


def test_eight_layers_random_weights_packed_generic_tuned_kernels_and_oracle(api, eight):
    dev, host = eight
    images = [np.random.default_rng([241, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    outs, lats = _forward_both(api, dev, SIZES, images)
    assert sum(np.count_nonzero(a) for a in lats) > sum(a.size for a in lats) // 8
    for i, (size, x) in enumerate(zip(SIZES, images)):
        alone = api.EightLayersNet(descs=eight_layer_descs(*size), shared_weights=dev)
        out, lat = alone.forward(torch.from_numpy(x[None]).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(lats[i], lat[0].cpu().numpy()), f"image {i} {size}: latent differs from EightLayersNet"
        assert np.array_equal(outs[i], out[0].cpu().numpy()), f"image {i} {size}: reconstruction differs from EightLayersNet"
        ref = c_oracle.run_net(eight_layer_descs(*size), [w for w, _ in host], [b for _, b in host], x, form="direct", threads=16)
        assert np.array_equal(lats[i], ref[3]) and np.array_equal(outs[i], ref[7]), f"image {i} {size}: differs from the oracle"


def test_eight_layers_param_weights_against_the_oracle(api):
    dev = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    z = np.load(ROOT / "tests" / "golden" / "param_weights.npz")
    words, biases = [z[f"w{n}_words"] for n in range(8)], [z[f"b{n}"] for n in range(8)]
    images = [np.random.default_rng([251, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    outs, lats = _forward_both(api, dev, SIZES, images)
    for i, (size, x) in enumerate(zip(SIZES, images)):
        ref = c_oracle.run_net(eight_layer_descs(*size), words, biases, x, form="direct", threads=16)
        assert np.array_equal(lats[i], ref[3]), f"image {i} {size}: latent differs from the oracle"
        assert np.array_equal(outs[i], ref[7]), f"image {i} {size}: reconstruction differs from the oracle"


def test_seventy_tiny_images(api, eight):
    """1 x 1 .. 8 x 8: one work item per image in both RGB ends, so every item of a launch looks up another row."""
    dev, host = eight
    sizes = [(1 + i % 8, 1 + (i // 8) % 8) for i in range(70)]
    images = [np.random.default_rng([257, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(sizes)]
    outs, lats = _forward_both(api, dev, sizes, images)
    for i, (size, x) in enumerate(zip(sizes, images)):
        ref = c_oracle.run_net(eight_layer_descs(*size), [w for w, _ in host], [b for _, b in host], x, form="direct", threads=1)
        assert np.array_equal(lats[i], ref[3]) and np.array_equal(outs[i], ref[7]), f"image {i} {size}: differs from the oracle"
        assert outs[i].shape == (16 * -(-size[1] // 16), 16 * -(-size[0] // 16), 3)


def test_order_of_the_batch_does_not_change_an_image(api, eight):
    dev, _ = eight
    order = sorted(range(len(SIZES)), key=lambda i: SIZES[i][0] * SIZES[i][1])
    images = [np.random.default_rng([263, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    res = []
    for idx in (order, order[::-1]):
        outs, lats = _forward_both(api, dev, [SIZES[i] for i in idx], [images[i] for i in idx])
        res.append({i: (outs[k], lats[k]) for k, i in enumerate(idx)})
    for i in range(len(SIZES)):
        assert np.array_equal(res[0][i][0], res[1][i][0]) and np.array_equal(res[0][i][1], res[1][i][1]), SIZES[i]


def test_layer_ranges(api, eight):
    """first = last = 7 written straight into `out`; layer 0 as the tap layer; first = last = 0."""
    dev, host = eight
    nets = {form: api.RaggedNet(SIZES, shared_weights=dev, rgb_ends=form) for form in ("packed", "generic")}
    rng = np.random.default_rng(269)
    x6, in6 = _pack_random(nets["packed"], rng, 6)
    xs, xin = _pack_random(nets["packed"], rng)
    got = {}
    for form, net in nets.items():
        got[form] = (_guarded(api, net, 7, 7, in6)[0], _guarded(api, net, 0, 1, xin, tap_layer=0), _guarded(api, net, 0, 0, xin)[0])
    p, g = got["packed"], got["generic"]
    assert torch.equal(p[0], g[0]) and torch.equal(p[1][0], g[1][0]) and torch.equal(p[1][1], g[1][1]) and torch.equal(p[2], g[2])
    assert torch.equal(p[1][1], p[2])                    # layer 0 tapped == layer 0 alone
    net = nets["packed"]
    for i, size in enumerate(SIZES):
        d = eight_layer_descs(*size)
        ref0 = c_oracle.run_layer(d[0], host[0][0], host[0][1], xs[i], "direct", threads=16)
        assert np.array_equal(net.views(0, p[2])[i].cpu().numpy(), ref0), f"image {i} {size}: layer 0"
        ref1 = c_oracle.run_layer(d[1], host[1][0], host[1][1], ref0, "direct", threads=16)
        assert np.array_equal(net.views(1, p[1][0])[i].cpu().numpy(), ref1), f"image {i} {size}: layer 1 behind the tapped layer 0"
        ref7 = c_oracle.run_layer(d[7], host[7][0], host[7][1], x6[i], "direct", threads=16)
        assert np.array_equal(net.views(7, p[0])[i].cpu().numpy(), ref7), f"image {i} {size}: layer 7"


def test_forward_captured_on_one_stream_and_replayed(api, eight):
    dev, _ = eight
    net = api.RaggedNet(SIZES, shared_weights=dev, rgb_ends="packed")
    generic = api.RaggedNet(SIZES, shared_weights=dev, rgb_ends="generic")
    rng = np.random.default_rng(271)
    _, xin = _pack_random(net, rng)
    out = torch.empty(net.nbytes(7), dtype=torch.uint8, device="cuda")
    lat = torch.empty(net.nbytes(3), dtype=torch.uint8, device="cuda")
    net.forward(xin, out, lat)                                 # warm-up: module load, workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            net.forward(xin, out, lat)
    for _ in range(2):
        _, fresh = _pack_random(net, rng)
        want_out, want_lat = generic.forward(fresh)            # eager, the other form, into buffers of its own
        torch.cuda.synchronize()
        xin.copy_(fresh)
        out.random_(0, 256)
        lat.random_(0, 256)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out) and torch.equal(lat, want_lat)
        assert np.count_nonzero(lat.cpu().numpy()) > lat.numel() // 8


def test_kernel_for_of_every_layer_in_both_forms(api, eight):
    dev, _ = eight
    L = api._lib.lib()
    for form in ("packed", "generic"):
        net = api.RaggedNet(SIZES, shared_weights=dev, rgb_ends=form)
        assert net.rgb_ends == form
        assert [net.kernel_for(l) for l in range(8)] == KERNELS[form]
        for bad in (-1, 8):
            assert L.sicn_ragged_net_kernel_for(net._h, bad) is None
            with pytest.raises(ValueError):
                net.kernel_for(bad)
    assert [api.RaggedNet(SIZES, shared_weights=dev).kernel_for(l) for l in range(8)] == KERNELS["packed"]     # the default
    # the cut the packed net launches: a quarter of the generic items in layer 7, through the net's own arrays
    q = (ctypes.c_int64 * 3)()
    items = {}
    for form, code in api._lib.RAGGED_RGB_ENDS.items():
        assert L.sicn_ragged_rgb_layout(net._cdescs, 8, net._widths, net._heights, len(SIZES), code, 7, len(SIZES) - 1, q) == 0
        items[form] = q[2]
    assert items["generic"] == 4 * items["packed"]
