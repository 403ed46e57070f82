"""GPU parity of ragged batches (include/sicn_ragged.h, csrc/k_ragged.hip; run with -m gpu on an MI355X): images of different sizes
through ONE launch per layer.  Everything is byte equality — the path is integer — against the numpy reference per layer, against
the tuned kernels of EightLayersNet on every image alone, and against the C oracle."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 33), (35, 35), (100, 36), (131, 70), (33, 1), (2, 67)]      # (width, height)
ENOSPC = -28
GUARD = 4096


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_weights(api, widths, seed):
    """Random nibble weights and bias of the 8 layers at `widths`: (device weights shared by every net of a test, [(W, b)])."""
    rng = np.random.default_rng(seed)
    descs = eight_layer_descs(16, 16, *widths)
    dev, host = [], []
    for d in descs:
        W = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
        b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
        fpw = api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, sicn_ref.pack_finn_tiles(W, d.SIMD, d.PE))
        dev.append(api.DeviceWeights(d, fpw, b))
        host.append((W, b))
    return dev, host


@pytest.fixture(scope="module")
def random_weights(api):
    return {widths: _random_weights(api, widths, [71, *widths]) for widths in [(128, 192), (64, 96)]}


@pytest.fixture(scope="module")
def param_weights(api):
    """The PARAM tables on the device, shared by the ragged nets and the per-size EightLayersNets of this module."""
    return [api.DeviceWeights(d, w, b) for d, (w, b) in zip(eight_layer_descs(16, 16), api.load_param_weights())]


def _layer_input(rng, shape):
    """tests/test_any_width_gpu.py::_input, for every image: bytes 0 .. 127 as a ReLU layer produces them, every seventh byte lifted
    to 128 .. 227 (the kernels read those as negative int8; 227 keeps the float32 GEMM of the numpy reference exact); RGB: 0 .. 255."""
    if shape[2] == 3:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    x = rng.integers(0, 128, shape, dtype=np.uint8)
    flat = x.reshape(-1)
    flat[::7] = 128 + flat[::7] % 100
    return x


def _images(rng, sizes):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]


def _alone(api, weights, size, x, widths=(128, 192)):
    """(reconstruction, latent) of one image through EightLayersNet of its own size."""
    net = api.EightLayersNet(descs=eight_layer_descs(size[0], size[1], *widths), shared_weights=weights)
    out, lat = net.forward(_dev(x[None]))
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), lat[0].cpu().numpy()


def _ragged_forward(net, images):
    out, lat = net.forward(net.pack([torch.from_numpy(x) for x in images]))
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in net.views(7, out)], [v.cpu().numpy() for v in net.views(3, lat)]


@pytest.mark.parametrize("layer", range(8))
@pytest.mark.parametrize("widths", [(128, 192), (64, 96)])
def test_single_layer_on_eight_sizes_in_one_call(api, random_weights, widths, layer):
    dev, host = random_weights[widths]
    net = api.RaggedNet(SIZES, shared_weights=dev, n_ch=widths[0], m_ch=widths[1])
    rng = np.random.default_rng([73, *widths, layer])
    xs = [_layer_input(rng, shp) for shp in net.shapes(layer - 1)]
    got, _ = net.run_layers(layer, layer, net.pack([torch.from_numpy(x) for x in xs], layer - 1))
    torch.cuda.synchronize()
    W, b = host[layer]
    ref_fn = sicn_ref.deconv522_ref if net.descs[layer].transposed else sicn_ref.conv2d_ref
    nonzero = 0
    for i, (x, v) in enumerate(zip(xs, net.views(layer, got))):
        ref = ref_fn(x, W, b)
        g = v.cpu().numpy()
        assert g.shape == ref.shape, (i, g.shape, ref.shape)
        assert np.array_equal(g, ref), f"image {i} {SIZES[i]}: {np.count_nonzero(g != ref)} of {ref.size} bytes differ"
        nonzero += np.count_nonzero(ref)
    assert nonzero > got.numel() // 8            # not a comparison of zeros


def test_whole_net_equals_the_tuned_kernels_and_the_oracle(api, param_weights):
    sizes = SIZES + [(256, 256)]
    images = _images(np.random.default_rng(79), sizes)
    net = api.RaggedNet(sizes, shared_weights=param_weights)
    outs, lats = _ragged_forward(net, images)
    z = np.load(ROOT / "tests" / "golden" / "param_weights.npz")
    words, biases = [z[f"w{n}_words"] for n in range(8)], [z[f"b{n}"] for n in range(8)]
    for i, (size, x) in enumerate(zip(sizes, images)):
        out, lat = _alone(api, param_weights, size, x)
        assert outs[i].shape == out.shape and lats[i].shape == lat.shape
        assert np.array_equal(lats[i], lat), f"image {i} {size}: latent differs from EightLayersNet"
        assert np.array_equal(outs[i], out), f"image {i} {size}: reconstruction differs from EightLayersNet"
        ref = c_oracle.run_net(eight_layer_descs(*size), words, biases, x, form="direct", threads=16)
        assert np.array_equal(lats[i], ref[3]), f"image {i} {size}: latent differs from the oracle"
        assert np.array_equal(outs[i], ref[7]), f"image {i} {size}: reconstruction differs from the oracle"


def test_whole_net_random_weights_equals_the_tuned_kernels(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    sizes = SIZES + [(256, 256)]
    images = _images(np.random.default_rng(83), sizes)
    outs, lats = _ragged_forward(api.RaggedNet(sizes, shared_weights=dev), images)
    assert sum(np.count_nonzero(a) for a in lats) > sum(a.size for a in lats) // 8
    for i, (size, x) in enumerate(zip(sizes, images)):
        out, lat = _alone(api, dev, size, x)
        assert np.array_equal(lats[i], lat), f"image {i} {size}: latent"
        assert np.array_equal(outs[i], out), f"image {i} {size}: reconstruction"


def test_equal_sizes_are_the_batched_call_byte_for_byte(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    w, h = 37, 21
    x = np.random.default_rng(89).integers(0, 256, (4, h, w, 3), dtype=np.uint8)
    batch = api.EightLayersNet(descs=eight_layer_descs(w, h), shared_weights=dev)
    out, lat = batch.forward(_dev(x))
    net = api.RaggedNet([(w, h)] * 4, shared_weights=dev)
    packed = net.pack([torch.from_numpy(a) for a in x])
    assert torch.equal(packed, _dev(x).reshape(-1))            # the layout itself
    rout, rlat = net.forward(packed)
    torch.cuda.synchronize()
    assert torch.equal(rout, out.reshape(-1)) and torch.equal(rlat, lat.reshape(-1))
    assert np.count_nonzero(rlat.cpu().numpy()) > rlat.numel() // 8


def test_one_image(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    x = _images(np.random.default_rng(97), [(131, 70)])
    outs, lats = _ragged_forward(api.RaggedNet([(131, 70)], shared_weights=dev), x)
    out, lat = _alone(api, dev, (131, 70), x[0])
    assert np.array_equal(outs[0], out) and np.array_equal(lats[0], lat)


def test_deep_table_of_seventy_tiny_images(api, random_weights):
    """1 x 1 .. 8 x 8: one work item per image and layer (four in a deconv), so every item of a launch looks up another row."""
    dev, _ = random_weights[(128, 192)]
    sizes = [(1 + i % 8, 1 + (i // 8) % 8) for i in range(70)]
    images = _images(np.random.default_rng(101), sizes)
    net = api.RaggedNet(sizes, shared_weights=dev)
    outs, lats = _ragged_forward(net, images)
    alone = {}
    for i, (size, x) in enumerate(zip(sizes, images)):
        out, lat = _alone(api, dev, size, x)
        alone[i] = (out, lat)
        assert np.array_equal(lats[i], lat), f"image {i} {size}: latent"
        assert np.array_equal(outs[i], out), f"image {i} {size}: reconstruction"
    # the first and the last image of the batch, explicitly
    for i in (0, 69):
        assert np.array_equal(outs[i], alone[i][0]) and np.array_equal(lats[i], alone[i][1])
        assert outs[i].shape == (16 * -(-sizes[i][1] // 16), 16 * -(-sizes[i][0] // 16), 3)


def test_order_of_the_batch_does_not_change_an_image(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    order = sorted(range(len(SIZES)), key=lambda i: SIZES[i][0] * SIZES[i][1])
    images = _images(np.random.default_rng(103), SIZES)
    res = {}
    for name, idx in (("smallest first", order), ("largest first", order[::-1])):
        outs, lats = _ragged_forward(api.RaggedNet([SIZES[i] for i in idx], shared_weights=dev), [images[i] for i in idx])
        res[name] = {i: (outs[k], lats[k]) for k, i in enumerate(idx)}
    for i in range(len(SIZES)):
        a, b = res["smallest first"][i], res["largest first"][i]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), SIZES[i]
    big = order[-1]                                            # first of one batch, last of the other: against the image alone
    out, lat = _alone(api, dev, SIZES[big], images[big])
    assert np.array_equal(res["largest first"][big][0], out) and np.array_equal(res["largest first"][big][1], lat)
    small = order[0]
    out, lat = _alone(api, dev, SIZES[small], images[small])
    assert np.array_equal(res["largest first"][small][0], out) and np.array_equal(res["largest first"][small][1], lat)


def _raw_forward(api, net, xin, out, tap, ws, ws_bytes):
    return api._lib.lib().sicn_ragged_net_forward(net._h, 0, 7, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), 3,
                                                  ctypes.c_void_p(tap.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_workspace_too_small_and_guard_bands(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    net = api.RaggedNet(SIZES, shared_weights=dev)
    images = _images(np.random.default_rng(107), SIZES)
    xin = net.pack([torch.from_numpy(x) for x in images])
    need = int(api._lib.lib().sicn_ragged_net_workspace_bytes(net._h))
    assert need == 2 * (-(-max(net.nbytes(l) for l in range(7)) // 256) * 256)
    bufs = {k: torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            for k, n in (("out", net.nbytes(7)), ("tap", net.nbytes(3)), ("ws", need))}
    # one byte short: SICN_ENOSPC, and nothing was enqueued — no buffer changes
    assert _raw_forward(api, net, xin, bufs["out"], bufs["tap"], bufs["ws"], need - 1) == ENOSPC
    torch.cuda.synchronize()
    assert all(bool((b == 0xA5).all()) for b in bufs.values())
    assert _raw_forward(api, net, xin, bufs["out"], bufs["tap"], bufs["ws"], need) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[-GUARD:] == 0xA5).all()), f"bytes behind {k} were written"
    want_out, want_lat = net.forward(xin)
    torch.cuda.synchronize()
    assert torch.equal(bufs["out"][:-GUARD], want_out) and torch.equal(bufs["tap"][:-GUARD], want_lat)
    assert not bool((bufs["out"][:-GUARD] == 0xA5).all())


def test_forward_captured_on_one_stream_and_replayed(api, random_weights):
    dev, _ = random_weights[(128, 192)]
    net = api.RaggedNet(SIZES, shared_weights=dev)
    rng = np.random.default_rng(109)
    xin = net.pack([torch.from_numpy(x) for x in _images(rng, SIZES)])
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
        fresh = net.pack([torch.from_numpy(x) for x in _images(rng, SIZES)])
        want_out, want_lat = net.forward(fresh)                # eager, into buffers of its own
        torch.cuda.synchronize()
        xin.copy_(fresh)
        out.zero_()
        lat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_out) and torch.equal(lat, want_lat)
        assert np.count_nonzero(lat.cpu().numpy()) > lat.numel() // 8
