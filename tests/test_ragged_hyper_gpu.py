"""GPU checks of library 0.8 (include/sicn_ragged_hyper.h; run with -m gpu on an MI355X): GDN / IGDN layers in a ragged net, the ragged
crop, and hyperprior.RaggedHyperpriorCodec — the hyperprior configuration over images of different sizes.  Everything is byte
equality: against the C oracle stage by stage, against EightLayersNet / HyperpriorCodec on every image alone, against numpy slicing."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from oracle.hyper_pipeline import hyper_pipeline_ref
from simple_image_compression_network_amd.config import CLayerDesc, eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height), as test_ragged_gpu.py
TEN = SIZES + [(96, 64), (176, 144)]
EINVAL = -22
GUARD = 4096
SEED = 7


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def hyperprior(api):
    from simple_image_compression_network_amd import hyperprior as _hp
    return _hp


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(rng, sizes):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]


def _layer_input(rng, shape):
    """tests/test_ragged_gpu.py::_layer_input: bytes as a ReLU layer produces them with every seventh lifted to 128 .. 227; RGB: any."""
    if shape[2] == 3:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    x = rng.integers(0, 128, shape, dtype=np.uint8)
    flat = x.reshape(-1)
    flat[::7] = 128 + flat[::7] % 100
    return x


def _random_weights(api, widths, seed):
    """(device weights, [(FINN words, bias)]) of the 8 layers at `widths`."""
    rng = np.random.default_rng(seed)
    dev, host = [], []
    for d in eight_layer_descs(16, 16, *widths):
        W = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
        b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
        words = sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE)
        dev.append(api.DeviceWeights(d, api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, words), b))
        host.append((words, b))
    return dev, host


@pytest.fixture(scope="module")
def random_weights(api):
    return {widths: _random_weights(api, widths, [171, *widths]) for widths in [(128, 192), (64, 96)]}


@pytest.fixture(scope="module")
def param(api):
    """The PARAM tables: device weights shared by every net of this module, and the oracle's (words, bias)."""
    z = np.load(ROOT / "tests" / "golden" / "param_weights.npz")
    dev = [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]
    return dev, [z[f"w{n}_words"] for n in range(8)], [z[f"b{n}"] for n in range(8)]


def _oracle_layer(d, words, bias, x, gdn_np):
    if gdn_np is None:
        return c_oracle.run_layer(d, words, bias, x, "direct", threads=16)
    beta, gamma, inverse, shift = gdn_np
    return c_oracle.gdn(c_oracle.run_layer_preact(d, words, bias, x, threads=16), beta, gamma, inverse, shift)


# ---- 1. single GDN / IGDN layers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", range(7))
@pytest.mark.parametrize("widths", [(128, 192), (64, 96)])
def test_single_gdn_layer_on_eight_sizes_in_one_call(api, hyperprior, random_weights, widths, layer):
    """(128, 192): k_gdn serves the activation; (64, 96): the generic activation kernel."""
    dev, host = random_weights[widths]
    descs = eight_layer_descs(16, 16, *widths)
    rng = np.random.default_rng([173, *widths, layer])
    beta, gamma = hyperprior.random_gdn_params(rng, descs[layer].OFM_CH)
    inverse = bool(descs[layer].transposed)
    gdn = [None] * 8
    gdn[layer] = api.GDN(beta, gamma, inverse=inverse, shift=12)
    net = api.RaggedNet(SIZES, shared_weights=dev, n_ch=widths[0], m_ch=widths[1], gdn=gdn)
    xs = [_layer_input(rng, shp) for shp in net.shapes(layer - 1)]
    got, _ = net.run_layers(layer, layer, net.pack([torch.from_numpy(x) for x in xs], layer - 1))
    torch.cuda.synchronize()
    words, bias = host[layer]
    differs_from_relu = 0
    for i, (x, v) in enumerate(zip(xs, net.views(layer, got))):
        d = eight_layer_descs(*SIZES[i], *widths)[layer]
        pre = c_oracle.run_layer_preact(d, words, bias, x, threads=16)
        ref = c_oracle.gdn(pre, beta, gamma, inverse, 12)
        g = v.cpu().numpy()
        assert g.shape == ref.shape, (i, g.shape, ref.shape)
        assert np.array_equal(g, ref), f"image {i} {SIZES[i]}: {np.count_nonzero(g != ref)} of {ref.size} bytes differ"
        differs_from_relu += np.count_nonzero(ref != np.where(pre >= 128, 0, pre))
    assert differs_from_relu > got.numel() // 8          # the activation is not the ReLU on these bytes


# ---- 2. the whole eight-layer net ------------------------------------------------------------------------------------------------------
def test_whole_gdn_net_equals_the_uniform_net_and_the_oracle(api, hyperprior, param):
    dev, words, biases = param
    gdn_np = hyperprior.hyper_parameters(*TEN[0], SEED)["gdn_np"]
    assert [g is not None for g in gdn_np] == [True, True, True, False, True, True, True, False]
    gdn = [None if g is None else api.GDN(g[0], g[1], inverse=g[2], shift=g[3]) for g in gdn_np]
    images = _images(np.random.default_rng(179), TEN)
    net = api.RaggedNet(TEN, shared_weights=dev, gdn=gdn)
    packed = net.pack([torch.from_numpy(x) for x in images])
    out, lat = net.forward(packed)
    y_again, tap1 = net.run_layers(0, 3, packed, tap_layer=1)           # tapping a GDN layer: the activated bytes
    torch.cuda.synchronize()
    assert torch.equal(y_again, lat)
    outs, lats = [v.cpu().numpy() for v in net.views(7, out)], [v.cpu().numpy() for v in net.views(3, lat)]
    taps = [v.cpu().numpy() for v in net.views(1, tap1)]
    for i, (size, x) in enumerate(zip(TEN, images)):
        alone = api.EightLayersNet(descs=eight_layer_descs(*size), shared_weights=dev, gdn=gdn)
        o, l = alone.forward(_dev(x[None]))
        torch.cuda.synchronize()
        assert np.array_equal(lats[i], l[0].cpu().numpy()), f"image {i} {size}: latent differs from EightLayersNet"
        assert np.array_equal(outs[i], o[0].cpu().numpy()), f"image {i} {size}: reconstruction differs from EightLayersNet"
        a, ref = x, []
        for d, w, b, g in zip(eight_layer_descs(*size), words, biases, gdn_np):
            a = _oracle_layer(d, w, b, a, g)
            ref.append(a)
        assert np.array_equal(taps[i], ref[1]), f"image {i} {size}: tapped GDN layer differs from the oracle"
        assert np.array_equal(lats[i], ref[3]), f"image {i} {size}: latent differs from the oracle"
        assert np.array_equal(outs[i], ref[7]), f"image {i} {size}: reconstruction differs from the oracle"
    # gdn given, every entry None: today's RaggedNet
    plain_out, plain_lat = api.RaggedNet(TEN, shared_weights=dev).forward(packed)
    none_out, none_lat = api.RaggedNet(TEN, shared_weights=dev, gdn=[None] * 8).forward(packed)
    torch.cuda.synchronize()
    assert torch.equal(plain_out, none_out) and torch.equal(plain_lat, none_lat)
    assert not torch.equal(plain_lat, lat)


# ---- 3. the ragged crop ---------------------------------------------------------------------------------------------------------------
def _crop_case(api, src_shapes, dst_shapes, c, seed):
    rng = np.random.default_rng([181, seed])
    crop = api.RaggedCrop(src_shapes, dst_shapes, c)
    srcs = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in src_shapes]
    src = _dev(np.concatenate([a.reshape(-1) for a in srcs]))
    before = src.clone()
    buf = torch.full((GUARD + crop.dst_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = buf[GUARD:GUARD + crop.dst_bytes]
    assert crop.run(src, dst) is dst
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all()), "bytes around dst were written"
    assert torch.equal(src, before), "src was written"
    for i, (a, v, (h, w)) in enumerate(zip(srcs, crop.views(dst), dst_shapes)):
        assert tuple(v.shape) == (h, w, c)
        assert np.array_equal(v.cpu().numpy(), a[:h, :w]), f"image {i}: {a.shape} -> {(h, w, c)}"
    # without dst: a tensor of its own, same bytes
    assert torch.equal(crop.run(src), dst)
    return crop, src, dst


def _up(v, k):
    return k * -(-v // k)


def test_crop_scale_maps_reconstructions_and_odd_channels(api):
    lat = [(-(-h // 16), -(-w // 16)) for w, h in TEN]
    _crop_case(api, [(_up(h, 4), _up(w, 4)) for h, w in lat], lat, 192, 0)         # h_s(z) -> the latents' shapes
    rec = [(h, w) for w, h in TEN]
    _crop_case(api, [(_up(h, 16), _up(w, 16)) for h, w in rec], rec, 3, 1)         # reconstructions -> the images' sizes (byte path)
    _crop_case(api, [(9, 7), (4, 4), (20, 3)], [(8, 7), (4, 3), (1, 1)], 5, 2)
    # C = 8: some images have 16-byte rows and offsets and are copied as vectors, their neighbours are not
    _crop_case(api, [(3, 4), (2, 3), (4, 2), (5, 6), (3, 8)], [(3, 2), (2, 3), (3, 2), (4, 4), (2, 6)], 8, 30)
    same = [(18, 2), (5, 5), (1, 9)]
    _, src, dst = _crop_case(api, same, same, 192, 3)                              # identity
    assert torch.equal(src, dst)
    _, src, dst = _crop_case(api, same, same, 3, 4)
    assert torch.equal(src, dst)


def test_crop_rows_around_a_work_item_and_seventy_one_row_images(api):
    r = api._lib.RAGGED_CROP_ROWS
    heights = [r - 1, r, r + 1, 1, 2 * r, 2 * r + 1]
    for c, seed in ((192, 5), (3, 6), (16, 7)):
        _crop_case(api, [(h + 1, 6) for h in heights], [(h, 5) for h in heights], c, seed)
        _crop_case(api, [(h, 6) for h in heights], [(h, 6) for h in heights], c, seed + 10)
    _crop_case(api, [(2, 1 + i % 5) for i in range(70)], [(1, 1 + i % 5) for i in range(70)], 192, 8)
    _crop_case(api, [(1, 2 + i % 7) for i in range(70)], [(1, 1 + i % 7) for i in range(70)], 3, 9)


@pytest.mark.parametrize("c", [192, 3])
def test_crop_of_equal_sizes_is_sicn_crop_nhwc(api, c):
    n, hs, ws, h, w = 4, 12, 14, 11, 13
    crop, src, dst = _crop_case(api, [(hs, ws)] * n, [(h, w)] * n, c, 20 + c)
    want = torch.empty(n * h * w * c, dtype=torch.uint8, device="cuda")
    api._lib.check(api._lib.lib().sicn_crop_nhwc(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(want.data_ptr()), n, hs, ws, h, w, c,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "sicn_crop_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(dst, want)


def test_ragged_net_cropped_gives_the_images_sizes(api, param):
    dev, _, _ = param
    net = api.RaggedNet(SIZES, shared_weights=dev)
    out, _ = net.forward(net.pack([torch.from_numpy(x) for x in _images(np.random.default_rng(191), SIZES)]))
    cut = net.cropped(out)
    torch.cuda.synchronize()
    assert cut.numel() == net.nbytes(-1)
    for (w, h), full, v in zip(SIZES, net.views(7, out), net.crop_views(cut)):
        assert tuple(v.shape) == (h, w, 3) and torch.equal(v, full[:h, :w])


# (src (h, w), dst (h, w)): one byte; 9 rows = two work items, the second one row; 17 rows cut to 9, rows of 16 c and 8 c bytes
CORNER = [((1, 1), (1, 1)), ((9, 5), (9, 4)), ((17, 16), (9, 8))]


def _corner_case(api, shapes, c, seed, misalign=0):
    """RaggedCrop, RaggedCut at x0 = y0 = 0 and the C entry points of the crop: one result, the slices of every image."""
    L = api._lib.lib()
    src_shapes, dst_shapes = [s for s, _ in shapes], [d for _, d in shapes]
    rng = np.random.default_rng([182, seed])
    srcs = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in src_shapes]
    flat = np.concatenate([np.zeros(misalign, np.uint8)] + [a.reshape(-1) for a in srcs])
    src = _dev(flat)[misalign:]
    assert src.data_ptr() % 16 == misalign
    crop = api.RaggedCrop(src_shapes, dst_shapes, c)
    cut = api.RaggedCut(src_shapes, [(0, 0, w, h) for h, w in dst_shapes], c)
    assert (crop.src_bytes, crop.dst_bytes) == (cut.src_bytes, cut.dst_bytes) == (src.numel(), sum(h * w * c for h, w in dst_shapes))
    a, b = crop.run(src), cut.run(src)
    n = len(shapes)
    i32 = ctypes.c_int32 * n
    handle = ctypes.c_void_p()
    api._lib.check(L.sicn_ragged_crop_create(i32(*[w for _, w in src_shapes]), i32(*[h for h, _ in src_shapes]),
                                             i32(*[w for _, w in dst_shapes]), i32(*[h for h, _ in dst_shapes]), c, n, ctypes.byref(handle)),
                   "sicn_ragged_crop_create")
    d = torch.full((crop.dst_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.sicn_ragged_crop_run(handle, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(d.data_ptr()),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    L.sicn_ragged_crop_free(handle)
    assert rc == 0
    assert torch.equal(a, b) and torch.equal(a, d)
    for i, (x, v, (h, w)) in enumerate(zip(srcs, crop.views(a), dst_shapes)):
        assert torch.equal(v.cpu(), torch.from_numpy(x)[:h, :w]), f"image {i}: {x.shape} -> {(h, w, c)}"
    return src, a


def test_crop_is_the_cut_at_the_corner(api):
    """The three images as one batch at 3 channels — every row byte by byte: 24-byte rows in the third image, no offset a multiple
    of 16 — and at 16 channels — every row as 16-byte vectors: offsets 0, 16 and 736.  (One batch has one channel count, so the
    byte path and the vector path of the same three shapes are two batches.)  Then the crop that cuts nothing, a plain copy, and
    the vector batch from a source one byte past a 16-byte boundary, which the kernel must copy byte by byte."""
    _corner_case(api, CORNER, 3, 0)
    _corner_case(api, CORNER, 16, 1)
    src, dst = _corner_case(api, [((8, 16), (8, 16))], 1, 2)
    assert torch.equal(src, dst)
    _corner_case(api, CORNER, 16, 3, misalign=1)


# ---- 4 - 6. the whole codec -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coded(api, hyperprior):
    """use_gdn -> (codec, images, containers, reconstruction) of one encode + decode of the ten sizes with seed 7, made once."""
    made = {}

    def get(use_gdn):
        if use_gdn not in made:
            codec = hyperprior.RaggedHyperpriorCodec(TEN, seed=SEED, use_gdn=use_gdn)
            images = _images(np.random.default_rng(193), TEN)
            codec.encode(codec.main.pack([torch.from_numpy(x) for x in images]))
            out = codec.decode()
            codec.check()
            made[use_gdn] = (codec, images, codec.containers(), out.clone())
        return made[use_gdn]
    return get


@pytest.mark.parametrize("use_gdn", [True, False])
def test_whole_codec_equals_the_oracle_pipeline_stage_by_stage(hyperprior, param, coded, use_gdn):
    from simple_image_compression_network_amd import codec as codec_mod
    _, words, biases = param
    codec, images, containers, out = coded(use_gdn)
    stages = {"y": codec.main.views(3, codec.y), "z": codec.h_a.views(1, codec.z), "s": codec.main.views(3, codec.s),
              "y_hat": codec.main.views(3, codec.y_hat), "recon": codec.main.views(7, out)}
    sizes = codec.bytes_per_image()
    for i, (size, x) in enumerate(zip(TEN, images)):
        zshape = stages["z"][i].shape
        ss = codec_mod.auto_stream_symbols(zshape[0] * zshape[1] * zshape[2])
        hp = hyperprior.hyper_parameters(*size, SEED, use_gdn)       # the same draws for every size; the descs are this image's
        ref = hyper_pipeline_ref(x, eight_layer_descs(*size), words, biases, hp, size, ss, threads=16)
        for name in ("y", "z", "s", "recon"):
            assert np.array_equal(stages[name][i].cpu().numpy(), ref[name]), f"image {i} {size}: {name}"
        assert np.array_equal(stages["y_hat"][i].cpu().numpy(), ref["y"]), f"image {i} {size}: y_hat"
        assert containers[i][0] == ref["z_container"], f"image {i} {size}: z container"
        assert containers[i][1] == ref["y_container"], f"image {i} {size}: y container"
        assert sizes[i] == len(ref["z_container"]) + len(ref["y_container"])


@pytest.mark.parametrize("size", [(100, 36), (96, 64), (176, 144)])
def test_containers_equal_the_uniform_codec(hyperprior, coded, size):
    codec, images, containers, _ = coded(True)
    i = TEN.index(size)
    hc = hyperprior.HyperpriorCodec(*size, 1, seed=SEED)
    hc.encode(_dev(images[i][None]))
    hc.check()
    zs, ys = hc.z_coder.sizes()[0], hc.y_coder.sizes()[0]
    assert hc.z_coder.slots[0, :zs].cpu().numpy().tobytes() == containers[i][0]
    assert hc.y_coder.slots[0, :ys].cpu().numpy().tobytes() == containers[i][1]


def test_a_second_codec_decodes_from_the_containers_alone(hyperprior, coded):
    codec, images, containers, out = coded(True)
    other = hyperprior.RaggedHyperpriorCodec(TEN, seed=SEED)
    got = other.decode(z_containers=[z for z, _ in containers], y_containers=[y for _, y in containers])
    other.check()
    torch.cuda.synchronize()
    assert torch.equal(got, out) and torch.equal(other.y_hat, codec.y)
    assert np.count_nonzero(got.cpu().numpy()) > got.numel() // 8


def test_permuting_the_batch_permutes_the_containers(hyperprior, coded):
    _, images, containers, _ = coded(True)
    perm = [9, 3, 0, 7, 5, 1, 8, 2, 6, 4]
    codec = hyperprior.RaggedHyperpriorCodec([TEN[i] for i in perm], seed=SEED)
    codec.encode(codec.main.pack([torch.from_numpy(images[i]) for i in perm]))
    assert codec.containers() == [containers[i] for i in perm]


def test_a_flipped_y_payload_byte_is_reported_for_its_image_only(api, hyperprior, coded):
    codec, images, containers, _ = coded(True)
    bad = 5
    ys = [y for _, y in containers]
    broken = bytearray(ys[bad])
    broken[-3] ^= 0x04
    ys[bad] = bytes(broken)
    other = hyperprior.RaggedHyperpriorCodec(TEN, seed=SEED)
    other.decode(z_containers=[z for z, _ in containers], y_containers=ys)
    with pytest.raises(api._lib.SicnError) as e:
        other.check()
    assert e.value.image == bad and f"image {bad}" in str(e.value)
    for i, (a, b) in enumerate(zip(other.main.views(3, other.y_hat), codec.main.views(3, codec.y))):
        if i != bad:
            assert torch.equal(a, b), f"image {i}"


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------
def test_analysis_hyper_stacks_and_crop_captured_in_one_graph(hyperprior):
    codec = hyperprior.RaggedHyperpriorCodec(SIZES, seed=SEED)
    rng = np.random.default_rng(197)
    xin = codec.main.pack([torch.from_numpy(x) for x in _images(rng, SIZES)])

    def enqueue():
        codec.main.run_layers(0, 3, xin, out=codec.y)
        codec.h_a.run_layers(0, 1, codec.y, out=codec.z)
        codec.h_s.run_layers(0, 1, codec.z, out=codec.s_full)
        codec.crop.run(codec.s_full, codec.s)
    enqueue()                                                  # warm-up: module load, workspaces
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            enqueue()
    eager = hyperprior.RaggedHyperpriorCodec(SIZES, seed=SEED)
    for _ in range(2):
        fresh = codec.main.pack([torch.from_numpy(x) for x in _images(rng, SIZES)])
        eager.main.run_layers(0, 3, fresh, out=eager.y)
        eager.h_a.run_layers(0, 1, eager.y, out=eager.z)
        eager._scale_map(eager.z)
        torch.cuda.synchronize()
        xin.copy_(fresh)
        for t in (codec.y, codec.z, codec.s_full, codec.s):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(codec.y, eager.y) and torch.equal(codec.z, eager.z) and torch.equal(codec.s, eager.s)
        assert np.count_nonzero(codec.s.cpu().numpy()) > codec.s.numel() // 8


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_gdn_of_another_channel_count_is_einval_and_creates_nothing(api, hyperprior, param):
    dev, _, _ = param
    L = api._lib.lib()
    beta, gamma = hyperprior.random_gdn_params(np.random.default_rng(199), 192)
    g192 = api.GDN(beta, gamma)
    with pytest.raises(api._lib.SicnError) as e:
        api.RaggedNet(SIZES, shared_weights=dev, gdn=[g192] + [None] * 7)         # layer 0 has 128 channels
    assert e.value.code == EINVAL
    descs = eight_layer_descs(16, 16)
    cd = (CLayerDesc * 8)(*[d.to_c() for d in descs])
    handles = (ctypes.c_void_p * 8)(*[w.handle for w in dev])
    ghandles = (ctypes.c_void_p * 8)()
    ghandles[6] = g192.handle                                                     # layer 6 has 128 channels too
    one = (ctypes.c_int32 * 1)(16)
    out = ctypes.c_void_p()
    assert L.sicn_ragged_net_create_gdn(cd, handles, ghandles, 8, one, one, 1, ctypes.byref(out)) == EINVAL
    assert not out.value
    ghandles[6], ghandles[3] = None, g192.handle                                  # layer 3 has 192: accepted
    assert L.sicn_ragged_net_create_gdn(cd, handles, ghandles, 8, one, one, 1, ctypes.byref(out)) == 0
    assert out.value
    L.sicn_ragged_net_free(out)


def test_crop_run_with_a_null_tensor_is_einval_and_launches_nothing(api):
    L = api._lib.lib()
    crop = api.RaggedCrop([(4, 4)], [(3, 3)], 16)
    src = torch.full((crop.src_bytes,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((crop.dst_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.sicn_ragged_crop_run(crop._h, None, ctypes.c_void_p(dst.data_ptr()), stream) == EINVAL
    assert L.sicn_ragged_crop_run(crop._h, ctypes.c_void_p(src.data_ptr()), None, stream) == EINVAL
    assert L.sicn_ragged_crop_run(None, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), stream) == EINVAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    assert L.sicn_ragged_crop_run(crop._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7).all())
