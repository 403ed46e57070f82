"""GPU parity of the planar RGB boundaries of a ragged net (include/sicn_ragged_planar.h; run with -m gpu on an MI355X): conv 3 -> N
reading [3][h][w] planes and deconv N -> 3 writing them at sizes of the caller's choice.  Everything is byte equality — the path is
integer.  The reference in every case is the interleaved PACKED net on the same weight handles, fed the permuted bytes and with its
output permuted and sliced on the host; single layers are also held to the C oracle's direct form.  Random weights and biases and
full-range bytes; small images throughout.  Every forward of this file runs between guard bands of 256 patterned bytes on both sides
of `out` and `tap_out`, over outputs that were filled with random bytes, so that a byte written outside and a byte not written both
show."""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import CLayerDesc, LayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
# conv 3 -> N: odd plane sizes in front bring the plane and row starts to every byte phase; tile edges at 31 / 32 / 33 (16 / 16 / 17
# output positions); more than one tile both ways
CONV_SIZES = [(1, 1), (2, 1), (1, 3), (3, 3), (5, 1), (31, 31), (32, 32), (33, 33), (31, 33), (33, 32), (32, 31), (65, 35),
              (1, 1), (33, 1), (2, 67), (100, 36)]
DECONV_MAPS = [(1, 1), (16, 16), (17, 15), (33, 2), (2, 33), (50, 18)]
GUARD = 256
PATTERN = ((np.arange(GUARD) * 37 + 11) & 255).astype(np.uint8)
EINVAL = -22
KERNELS = ["mfma_conv_rgb_planar"] + ["mfma_conv_any"] * 3 + ["mfma_deconv_any"] * 3 + ["mfma_deconv_rgb_planar"]
KERNELS_INTERLEAVED = ["mfma_conv_rgb_packed"] + KERNELS[1:7] + ["mfma_deconv_rgb_packed"]


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
    """The eight layers at (128, 192) with random weights: the device handles."""
    rng = np.random.default_rng([311, 128, 192])
    return [_weights_of(api, d, rng)[0] for d in eight_layer_descs(16, 16)]


@pytest.fixture(scope="module")
def eight_ref(api, eight):
    """The reference of the eight-layer cases, computed once and left unchanged: the interleaved PACKED net over SIZES on `eight`,
    one seeded input.  -> (images [h][w][3], latent bytes, reconstructions [OH][OW][3], cropped to the images' sizes)."""
    net = api.RaggedNet(SIZES, shared_weights=eight)
    images = [np.random.default_rng([313, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    out, lat = net.forward(net.pack([torch.from_numpy(x) for x in images]))
    crop = net.cropped(out)
    torch.cuda.synchronize()
    assert np.count_nonzero(lat.cpu().numpy()) > lat.numel() // 8
    return (images, lat.cpu(), [v.cpu().numpy() for v in net.views(7, out)], [v.cpu().numpy() for v in net.crop_views(crop)])


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


def _planar(x):
    """[h][w][3] -> [3][h][w], contiguous (numpy)."""
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def _pack_planar(net, images):
    return net.pack([torch.from_numpy(_planar(x)) for x in images])


# ---- conv 3 -> N, planar in ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64, 192])
def test_conv_planar_in_every_byte_phase_and_tile_edge(api, n):
    rng = np.random.default_rng([317, n])
    dev, words, bias = _weights_of(api, _conv_desc(n), rng)
    ref = api.RaggedNet(CONV_SIZES, shared_weights=[dev], descs=[_conv_desc(n)])
    net = api.RaggedNet(CONV_SIZES, shared_weights=[dev], descs=[_conv_desc(n)], rgb_layout="planar")
    assert net.kernel_for(0) == "mfma_conv_rgb_planar" and ref.kernel_for(0) == "mfma_conv_rgb_packed"
    assert net.planar_in and not net.planar_out
    assert net.shapes(-1) == [(3, h, w) for w, h in CONV_SIZES] and net.shapes(0) == ref.shapes(0)
    assert net._offsets[0] == ref._offsets[0] and net.nbytes(-1) == ref.nbytes(-1)
    # the coverage, from the offsets: the start of each of the three planes and the starts of the rows meet all four byte phases
    planes = [{(o + c * w * h) % 4 for o, (w, h) in zip(net._offsets[0], CONV_SIZES)} for c in range(3)]
    rows = {(o + (c * h + y) * w) % 4 for o, (w, h) in zip(net._offsets[0], CONV_SIZES) for c in range(3) for y in range(min(h, 4))}
    assert planes == [{0, 1, 2, 3}] * 3 and rows == {0, 1, 2, 3}
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in CONV_SIZES]
    want = _guarded(api, ref, 0, 0, ref.pack([torch.from_numpy(x) for x in images]))[0]
    got = _guarded(api, net, 0, 0, _pack_planar(net, images))[0]
    assert torch.equal(got, want), "planar in differs from the interleaved net"
    nonzero = 0
    for i, (x, v) in enumerate(zip(images, net.views(0, got))):
        o = c_oracle.run_layer(_conv_desc(n, *CONV_SIZES[i]), words, bias, x, "direct", threads=16)
        assert np.array_equal(v.cpu().numpy(), o), f"image {i} {CONV_SIZES[i]}: differs from the oracle"
        nonzero += np.count_nonzero(o)
    assert nonzero > got.numel() // 8          # not a comparison of zeros


# ---- deconv N -> 3, planar out ------------------------------------------------------------------------------------------------------
# (input map, cut): (1, 1), (2w - 1, 2h), (2w, 2h - 1), (2w - 15, 2h - 15) and the full size, on one-tile and many-tile maps
CUTS = [((1, 1), (1, 1)), ((16, 16), (31, 32)), ((17, 15), (34, 29)), ((33, 2), (66, 4)), ((2, 33), (3, 66)), ((50, 18), (85, 21)),
        ((50, 18), (1, 1)), ((16, 16), (17, 17)), ((17, 15), (34, 30)), ((33, 2), (66, 3))]


@pytest.mark.parametrize("n", [32, 96, 192])
@pytest.mark.parametrize("cut", [False, True])
def test_deconv_planar_out_at_the_chain_rule_sizes_and_cut(api, n, cut):
    """96: a half-empty last K chunk.  Every byte of the tensor is written (the buffers are random before) and none of the guards."""
    rng = np.random.default_rng([331, n])
    dev, words, bias = _weights_of(api, _deconv_desc(n), rng)
    maps = [m for m, _ in CUTS] if cut else DECONV_MAPS
    out_sizes = [c for _, c in CUTS] if cut else None
    assert set(maps) == set(DECONV_MAPS)
    ref = api.RaggedNet(maps, shared_weights=[dev], descs=[_deconv_desc(n)])
    net = api.RaggedNet(maps, shared_weights=[dev], descs=[_deconv_desc(n)], rgb_layout="planar", out_sizes=out_sizes)
    assert net.kernel_for(0) == "mfma_deconv_rgb_planar" and net.planar_out and not net.planar_in
    sizes = out_sizes if cut else [(2 * w, 2 * h) for w, h in maps]
    assert net.shapes(0) == [(3, h, w) for w, h in sizes] and net.nbytes(0) == sum(3 * w * h for w, h in sizes)
    xs = [rng.integers(0, 256, shp, dtype=np.uint8) for shp in ref.shapes(-1)]
    xin = ref.pack([torch.from_numpy(x) for x in xs])
    want = [v.cpu().numpy() for v in ref.views(0, _guarded(api, ref, 0, 0, xin)[0])]
    got = _guarded(api, net, 0, 0, xin)[0]
    for i, ((w, h), v) in enumerate(zip(sizes, net.views(0, got))):
        assert v.is_contiguous() and tuple(v.shape) == (3, h, w)
        assert np.array_equal(v.cpu().numpy(), _planar(want[i][:h, :w])), f"image {i}: map {maps[i]} cut to {(w, h)}"
        o = c_oracle.run_layer(_deconv_desc(n, *maps[i]), words, bias, xs[i], "direct", threads=16)
        assert np.array_equal(v.cpu().numpy(), _planar(o[:h, :w])), f"image {i}: differs from the oracle"


# ---- the eight layers -----------------------------------------------------------------------------------------------------------------
def _check_eight(api, net, got_out, got_lat, ref):
    images, lat, _, cropped = ref
    assert torch.equal(got_lat.cpu(), lat), "latent: the planar net differs from the interleaved one"
    for i, (v, want) in enumerate(zip(net.views(7, got_out), cropped)):
        assert np.array_equal(v.cpu().numpy(), _planar(want)), f"image {i} {SIZES[i]}: reconstruction"


def test_eight_layers_random_weights(api, eight, eight_ref):
    net = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar")
    assert [net.kernel_for(l) for l in range(8)] == KERNELS
    assert net.out_sizes == SIZES and net.shapes(7) == [(3, h, w) for w, h in SIZES] and net.nbytes(7) == net.nbytes(-1)
    out, lat = _guarded(api, net, 0, 7, _pack_planar(net, eight_ref[0]), tap_layer=3)
    _check_eight(api, net, out, lat, eight_ref)
    assert net.cropped(out) is out                      # the output already has the images' sizes
    with pytest.raises(ValueError, match="dst"):        # nothing is copied: a destination is refused, not left unwritten
        net.cropped(out, dst=torch.empty_like(out))
    assert [tuple(v.shape) for v in net.crop_views(out)] == net.shapes(7)
    # at the chain-rule sizes: the interleaved reconstruction whole, and no crop to be had
    full = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar", out_sizes=[(16 * -(-w // 16), 16 * -(-h // 16)) for w, h in SIZES])
    out, _ = _guarded(api, full, 0, 7, _pack_planar(full, eight_ref[0]))
    for i, v in enumerate(full.views(7, out)):
        assert np.array_equal(v.cpu().numpy(), _planar(eight_ref[2][i])), f"image {i} {SIZES[i]}"
    with pytest.raises(ValueError):
        full.cropped(out)


@pytest.mark.parametrize("with_gdn", [False, True])
def test_eight_layers_param_weights_and_the_main_nets_gdn_list(api, with_gdn):
    from simple_image_compression_network_amd import hyperprior
    dev = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    gdn = None
    if with_gdn:
        gdn = [None if g is None else api.GDN(g[0], g[1], inverse=g[2], shift=g[3]) for g in hyperprior.hyper_parameters(16, 16, 0, True)["gdn_np"]]
        assert gdn[0] is not None and gdn[7] is None
    ref = api.RaggedNet(SIZES, shared_weights=dev, gdn=gdn)
    net = api.RaggedNet(SIZES, shared_weights=dev, gdn=gdn, rgb_layout="planar")
    images = [np.random.default_rng([337, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(SIZES)]
    w_out, w_lat = ref.forward(ref.pack([torch.from_numpy(x) for x in images]))
    want = [v.cpu().numpy() for v in ref.crop_views(ref.cropped(w_out))]
    out, lat = _guarded(api, net, 0, 7, _pack_planar(net, images), tap_layer=3)
    assert torch.equal(lat, w_lat) and np.count_nonzero(lat.cpu().numpy()) > 0
    for i, v in enumerate(net.views(7, out)):
        assert np.array_equal(v.cpu().numpy(), _planar(want[i])), f"image {i} {SIZES[i]}"


def test_seventy_tiny_images(api, eight):
    """1 x 1 .. 8 x 8: one work item per image in both RGB ends, every plane start at another phase."""
    sizes = [(1 + i % 8, 1 + (i // 8) % 8) for i in range(70)]
    images = [np.random.default_rng([347, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(sizes)]
    ref = api.RaggedNet(sizes, shared_weights=eight)
    net = api.RaggedNet(sizes, shared_weights=eight, rgb_layout="planar")
    w_out, w_lat = ref.forward(ref.pack([torch.from_numpy(x) for x in images]))
    want = [v.cpu().numpy() for v in ref.views(7, w_out)]
    out, lat = _guarded(api, net, 0, 7, _pack_planar(net, images), tap_layer=3)
    assert torch.equal(lat, w_lat)
    for i, ((w, h), v) in enumerate(zip(sizes, net.views(7, out))):
        assert np.array_equal(v.cpu().numpy(), _planar(want[i][:h, :w])), f"image {i} {sizes[i]}"


def test_layer_ranges_and_taps(api, eight, eight_ref):
    images, lat, _, cropped = eight_ref
    ref = api.RaggedNet(SIZES, shared_weights=eight)
    net = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar")
    xin = _pack_planar(net, images)
    # (0, 3) then (4, 7): the latent between them is today's bytes
    mid, _ = _guarded(api, net, 0, 3, xin)
    assert torch.equal(mid.cpu(), lat)
    out, _ = _guarded(api, net, 4, 7, mid.contiguous())
    _check_eight(api, net, out, mid, eight_ref)
    # (0, 0) alone: the interleaved net's layer 0
    want0 = _guarded(api, ref, 0, 0, ref.pack([torch.from_numpy(x) for x in images]))[0]
    assert torch.equal(_guarded(api, net, 0, 0, xin)[0], want0)
    # tap_layer = 3 gives today's bytes; tap_layer = 7 writes the planar form and equals `out`
    out3, tap3 = _guarded(api, net, 0, 7, xin, tap_layer=3)
    assert torch.equal(tap3.cpu(), lat) and torch.equal(out3, out)
    out7, tap7 = _guarded(api, net, 0, 7, xin, tap_layer=7)
    assert torch.equal(tap7, out7) and torch.equal(out7, out)
    assert tap7.numel() == net.nbytes(7) == sum(3 * w * h for w, h in SIZES)
    # an inner tap in front of the planar end, and the last layer alone into `out`
    want6 = _guarded(api, ref, 0, 6, ref.pack([torch.from_numpy(x) for x in images]))[0]
    out6, tap6 = _guarded(api, net, 0, 7, xin, tap_layer=6)
    assert torch.equal(tap6, want6) and torch.equal(out6, out)
    assert torch.equal(_guarded(api, net, 7, 7, want6.contiguous())[0], out)
    # a workspace too small is refused with nothing enqueued
    ws = net.workspace()
    probe = torch.zeros(net.nbytes(7), dtype=torch.uint8, device="cuda")
    rc = api._lib.lib().sicn_ragged_net_forward(net._h, 0, 7, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(probe.data_ptr()), -1, None,
                                                ctypes.c_void_p(ws.data_ptr()), ws.numel() // 2 - 1, None)
    torch.cuda.synchronize()
    assert rc == -28 and not probe.any()


# ---- archives and the hyperprior codec --------------------------------------------------------------------------------------------
def test_archives_are_the_interleaved_nets_and_decode_to_the_planar_forward(api, eight, eight_ref):
    images = eight_ref[0]
    ref = api.RaggedNet(SIZES, shared_weights=eight)
    net = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar")
    xin = _pack_planar(net, images)
    b = net.compress_archive(xin)
    assert b == ref.compress_archive(ref.pack([torch.from_numpy(x) for x in images]))
    assert net.compress(xin) == ref.compress(ref.pack([torch.from_numpy(x) for x in images]))
    fwd, _ = net.forward(xin)
    assert torch.equal(net.decompress_archive(b), fwd)
    assert torch.equal(net.decompress(net.compress(xin)), fwd)
    made = api.RaggedNet.from_archive(b, shared_weights=eight, rgb_layout="planar")
    assert made.sizes == SIZES and made.planar_out and made.shapes(7) == net.shapes(7)
    assert torch.equal(made.decompress_archive(b), fwd)
    sel = [1, 4, 5]
    part = api.RaggedNet.from_archive(b, images=sel, shared_weights=eight, rgb_layout="planar")
    got = part.views(7, part.decompress_archive(b, images=sel))
    for k, i in enumerate(sel):
        assert torch.equal(got[k], net.views(7, fwd)[i])


def test_hyperprior_codec_planar(api):
    from simple_image_compression_network_amd import hyperprior
    sizes = [(35, 35), (100, 36), (17, 33)]
    images = [np.random.default_rng([349, i]).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(sizes)]
    ref = hyperprior.RaggedHyperpriorCodec(sizes, seed=3)
    cod = hyperprior.RaggedHyperpriorCodec(sizes, seed=3, rgb_layout="planar")
    assert [cod.main.kernel_for(l) for l in range(8)] == KERNELS and cod.h_a.rgb_layout == "interleaved"
    ref.encode(ref.main.pack([torch.from_numpy(x) for x in images]))
    cod.encode(_pack_planar(cod.main, images))
    assert cod.containers() == ref.containers() and cod.archive() == ref.archive()
    want = [v.cpu().numpy() for v in ref.main.crop_views(ref.main.cropped(ref.decode()))]
    got = cod.decode()
    cod.check()
    for i, v in enumerate(cod.main.views(7, got)):
        assert np.array_equal(v.cpu().numpy(), _planar(want[i])), f"image {i} {sizes[i]}"
    for refused in (lambda: cod.roi([None] * 3), lambda: cod.moving_roi([(0, 8, 8)]), lambda: cod.decode(rois=[None] * 3)):
        with pytest.raises(ValueError, match="planar"):
            refused()


# ---- a captured graph -----------------------------------------------------------------------------------------------------------------
def test_forward_captured_on_one_stream_and_replayed(api, eight):
    net = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar")
    ref = api.RaggedNet(SIZES, shared_weights=eight)
    rng = np.random.default_rng(353)
    xin = torch.empty(net.nbytes(-1), dtype=torch.uint8, device="cuda")
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
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in SIZES]
        w_out, w_lat = ref.forward(ref.pack([torch.from_numpy(x) for x in images]))      # eager, the other layout, buffers of its own
        want = [v.cpu().numpy() for v in ref.crop_views(ref.cropped(w_out))]
        torch.cuda.synchronize()
        xin.copy_(_pack_planar(net, images))
        out.random_(0, 256)
        lat.random_(0, 256)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lat, w_lat)
        for i, v in enumerate(net.views(7, out)):
            assert np.array_equal(v.cpu().numpy(), _planar(want[i])), f"image {i} {SIZES[i]}"


# ---- names and refusals ---------------------------------------------------------------------------------------------------------------
def test_kernel_for(api, eight):
    d8 = eight_layer_descs(16, 16)
    assert [api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar").kernel_for(l) for l in range(8)] == KERNELS
    for kw in (dict(), dict(rgb_layout="interleaved")):
        assert [api.RaggedNet(SIZES, shared_weights=eight, **kw).kernel_for(l) for l in range(8)] == KERNELS_INTERLEAVED
    # one planar end each; a chain without an RGB end has none
    front = api.RaggedNet(SIZES, shared_weights=eight[:4], descs=d8[:4], rgb_layout="planar")
    assert [front.kernel_for(l) for l in range(4)] == KERNELS[:4] and front.planar_in and not front.planar_out
    back = api.RaggedNet([(2, 3), (1, 1)], shared_weights=eight[4:], descs=d8[4:], rgb_layout="planar")
    assert [back.kernel_for(l) for l in range(4)] == KERNELS[4:] and back.planar_out and not back.planar_in
    assert back.out_sizes is None and back.shapes(3) == [(3, 48, 32), (3, 16, 16)]          # no conv 3 -> N in front: the chain-rule sizes
    inner = api.RaggedNet(SIZES, shared_weights=eight[1:3], descs=d8[1:3], rgb_layout="planar")
    assert [inner.kernel_for(l) for l in range(2)] == KERNELS[1:3] and not inner.planar_in and not inner.planar_out
    L = api._lib.lib()
    for bad in (-1, 8):
        assert L.sicn_ragged_net_kernel_for(front._h, bad) is None


def test_roi_entry_points_refuse_a_planar_net(api, eight):
    net = api.RaggedNet(SIZES, shared_weights=eight, rgb_layout="planar")
    b = net.compress_archive(_pack_planar(net, [np.zeros((h, w, 3), np.uint8) for w, h in SIZES]))
    rects = [None] * len(SIZES)
    for refused in (lambda: net.moving_roi([(1, 8, 8)]), lambda: api.RaggedRoi(net, rects), lambda: api.MovingRoi(net, [(1, 8, 8)]),
                    lambda: net.decompress_archive(b, rois=rects)):
        with pytest.raises(ValueError, match="planar"):
            refused()
    # one planar end is enough
    front = api.RaggedNet(SIZES, shared_weights=eight[:4], descs=eight_layer_descs(16, 16)[:4], rgb_layout="planar")
    assert front.planar_in and not front.planar_out
    with pytest.raises(ValueError, match="planar"):
        api.RaggedRoi(front, rects)


def test_create_planar_refusal_codes(api, eight):
    """The refusals of sicn_ragged_net_create_planar over real weight handles: the good call succeeds, each bad one is SICN_EINVAL with
    nothing created."""
    L = api._lib.lib()
    d8 = eight_layer_descs(16, 16)
    n_img = 2
    ws, hs = (ctypes.c_int32 * n_img)(35, 100), (ctypes.c_int32 * n_img)(35, 36)
    rule_w, rule_h = (ctypes.c_int32 * n_img)(48, 112), (ctypes.c_int32 * n_img)(48, 48)

    def create(descs, weights, gdn=None, rgb_ends=1, pin=0, pout=0, ow=None, oh=None):
        n = len(descs)
        cd = (CLayerDesc * n)(*[d.to_c() for d in descs])
        handles = (ctypes.c_void_p * n)(*[w.handle for w in weights])
        gh = None if gdn is None else (ctypes.c_void_p * n)(*[(g.handle if g is not None else None) for g in gdn])
        h = ctypes.c_void_p(0)
        rc = L.sicn_ragged_net_create_planar(cd, handles, gh, n, ws, hs, n_img, rgb_ends, pin, pout, ow, oh, ctypes.byref(h))
        if rc == 0:
            assert h.value
            L.sicn_ragged_net_free(h)
        else:
            assert not h.value
        return rc
    from simple_image_compression_network_amd import hyperprior
    rng = np.random.default_rng(359)
    p3, p128 = hyperprior.random_gdn_params(rng, 3), hyperprior.random_gdn_params(rng, 128)
    igdn = api.GDN(p3[0], p3[1], inverse=True, shift=12)
    gdn0 = api.GDN(p128[0], p128[1], inverse=False, shift=12)
    assert create(d8, eight, pin=1, pout=1, ow=ws, oh=hs) == 0
    assert create(d8, eight, pin=1, pout=1) == 0 and create(d8, eight, pin=1) == 0 and create(d8, eight, pout=1, ow=rule_w, oh=rule_h) == 0
    assert create(d8, eight, gdn=[gdn0] + [None] * 7, pin=1, pout=1) == 0                    # a GDN behind the planar conv is fine
    assert create(d8, eight) == 0 and create(d8, eight, rgb_ends=0) == 0                     # sicn_ragged_net_create_rgb
    for bad in (2, -1):
        assert create(d8, eight, pin=bad) == EINVAL and create(d8, eight, pout=bad) == EINVAL
    assert create(d8[1:], eight[1:], pin=1) == EINVAL                                        # layer 0 is not conv 3 -> N
    assert create(d8[:7], eight[:7], pout=1) == EINVAL                                       # the last layer is not deconv N -> 3
    assert create(d8[4:], eight[4:], pin=1) == EINVAL
    assert create(d8, eight, rgb_ends=0, pin=1) == EINVAL and create(d8, eight, rgb_ends=0, pout=1) == EINVAL
    assert create(d8, eight, gdn=[None] * 7 + [igdn], pout=1) == EINVAL                      # an IGDN on the planar-out layer
    assert create(d8, eight, gdn=[None] * 7 + [igdn]) == 0
    assert create(d8, eight, ow=ws, oh=hs) == EINVAL                                         # sizes with INTERLEAVED out
    assert create(d8, eight, pout=1, ow=ws) == EINVAL and create(d8, eight, pout=1, oh=hs) == EINVAL
    for w2, h2 in (((48, 113), (48, 48)), ((48, 112), (49, 48)), ((0, 112), (48, 48)), ((48, 112), (48, 0)), ((48, -1), (48, 48))):
        assert create(d8, eight, pout=1, ow=(ctypes.c_int32 * 2)(*w2), oh=(ctypes.c_int32 * 2)(*h2)) == EINVAL
