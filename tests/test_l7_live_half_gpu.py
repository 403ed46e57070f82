"""Layer 7 with one live region: where layer 6 ran at most 4 accumulator columns in the same call, all it computed sits in the
channels 0 .. 63 and layer 7 (k_l7<1>, csrc/k_rgb.hip) neither fetches nor multiplies the other half.  Every byte that leaves the
chain must be what it was: held to the oracle (c_oracle.run_net, direct form) and to the same layers run one by one through the
per-layer entry points, which compute and read every channel.
wave_tile = 128 and persistent_grid = 8 put the wide family, and with it the 3-column layer 6, on tiny images
(tests/test_live_columns_gpu.py).  Two sizes, 3 images each:
  132 x 68: layer 7 sees 72 x 40 (132 -> 66 -> 33 -> 17 -> 9 -> 18 -> 36 -> 72, 68 -> 34 -> 17 -> 9 -> 5 -> 10 -> 20 -> 40) = three
            strips of 32 columns, the last one partial (8 columns: the slow epilogue path), and 10 whole steps of 4 rows;
  128 x 72: layer 7 sees 64 x 40 = two whole strips (the fast-row epilogue) and 10 whole steps.
An 8-layer net doubles a latent three times before layer 7, so the height layer 7 sees is always a multiple of 8: a partial last step
and a strip of 2 columns (66 x 34 behind a deconv on 33 x 17), with the one-chunk run of 9 steps, are in
tests/test_live_geometry_gpu.py.
The ring of the kernel holds 368 positions: the prologue fills 8 rows of 36, every step adds 144, so the SECOND step of any chunk
already wraps.  The default cut on these sizes is one step per chunk (plan_l7: two workgroups per CU are more chunks than there are
steps), which never gets that far; strip_chunks = 2 cuts the 10 steps into 5 + 5, strip_chunks = 3 into 4 + 4 + 2: every chunk wraps,
and every chunk but the first starts with the pass that stores nothing."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPTIONS = {"wave_tile": 128, "persistent_grid": 8}
N_IMG = 3
SIZES = {"132x68": (132, 68), "128x72": (128, 72)}
GOLDEN = Path(__file__).resolve().parent / "golden" / "param_weights.npz"


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


def _descs(size):
    return eight_layer_descs(*SIZES[size])


def _images(size, seed=1):
    w, h = SIZES[size]
    return np.random.default_rng(seed).integers(0, 256, (N_IMG, h, w, 3), dtype=np.uint8)


def _random_net(seed, n_dead):
    """as tests/test_live_columns_gpu.py: n_dead random input channels of every 128-channel input are zero, the bias differs per channel"""
    rng = np.random.default_rng(seed)
    net = []
    for d in _descs("132x68"):
        w = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
        if d.IFM_CH == 128 and n_dead:
            w[:, :, :, rng.permutation(128)[:n_dead]] = 0
        b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
        net.append((w, b))
    return net


def _param_net():
    return [(w, b) for w, b, _ in sicn_ref.load_param_fixture(GOLDEN)]


WEIGHTS = {
    "param": _param_net,
    "random_dead112": lambda: _random_net(112, 112),
    "random_dead80": lambda: _random_net(80, 80),       # 48 live: layer 7 is given, and reads, all 48 bytes that 3 columns leave
    "random_dead48": lambda: _random_net(48, 48),
    "dense": lambda: _random_net(5, 0),
}
_NETS, _ORACLE = {}, {}


def _weights(name):
    if name not in _NETS:
        _NETS[name] = WEIGHTS[name]()
    return _NETS[name]


def _words(size, net):
    return [sicn_ref.pack_finn_tiles(w, d.SIMD, d.PE) for d, (w, _) in zip(_descs(size), net)]


def _build(api, name, size, **options):
    net = _weights(name)
    descs = _descs(size)
    params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, wd), b) for d, wd, (_, b) in zip(descs, _words(size, net), net)]
    w, h = SIZES[size]
    return api.EightLayersNet(w, h, params=params, options=dict(OPTIONS, **options)), params


def _oracle(name, size):
    """every layer's output of every image, computed once per weight set and size and never changed"""
    if (name, size) not in _ORACLE:
        net, x = _weights(name), _images(size)
        _ORACLE[name, size] = [c_oracle.run_net(_descs(size), _words(size, net), [b for _, b in net], x[i], form="direct", threads=16)
                               for i in range(N_IMG)]
    return _ORACLE[name, size]


def _halves(net, first=0, last=7, tap=3):
    from simple_image_compression_network_amd import _lib
    h = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().sicn_debug_net_input_halves(net._h, first, last, tap, N_IMG, h), "sicn_debug_net_input_halves")
    return list(h)


def _same(got, want, what):
    got = got.cpu().numpy()
    for i in range(N_IMG):
        if not np.array_equal(got[i], want[i]):
            bad = np.argwhere(got[i] != want[i])
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(f"{what}, image {i}: {len(bad)} wrong bytes; first: got {got[i][y, xx, c]} want {want[i][y, xx, c]} "
                                 f"at ({y}, {xx}, {c}); rows {sorted({int(v) for v in bad[:, 0]})[:12]}")


def _check_forward(net, name, size, what):
    out, latent = net.forward(torch.from_numpy(_images(size)).cuda())
    torch.cuda.synchronize()
    ref = _oracle(name, size)
    _same(latent, [r[3] for r in ref], f"{what}: latent")
    _same(out, [r[7] for r in ref], f"{what}: reconstruction")
    return out, latent


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", ["param", "random_dead112", "random_dead80"])
def test_one_half_is_the_oracle_and_the_layers_one_by_one(api, name, size):
    net, params = _build(api, name, size)
    assert _halves(net) == [2] * 7 + [1]
    out, latent = _check_forward(net, name, size, f"{name} {size}")
    t = torch.from_numpy(_images(size)).cuda()
    single = []
    for d, (w, b) in zip(_descs(size), params):   # every channel computed and read, nothing permuted
        t = (api.deconv522 if d.transposed else api.conv2d)(d, w, b, t, None, N_IMG, options=OPTIONS)
        single.append(t)
    torch.cuda.synchronize()
    assert torch.equal(latent, single[3]) and torch.equal(out, single[7]), f"{name} {size}: the net differs from its layers run one by one"


@pytest.mark.parametrize("chunks", [2, 3])
def test_param_in_forced_chunks(api, chunks):
    """10 steps as 5 + 5 or 4 + 4 + 2 (the module's docstring): the pass that stores nothing and the ring wrap in every chunk"""
    net, _ = _build(api, "param", "132x68", strip_chunks=chunks)
    assert _halves(net) == [2] * 7 + [1]
    _check_forward(net, "param", "132x68", f"param, {chunks} chunks")


def test_param_workspace_content_does_not_matter(api):
    """the two planes of every phase that layer 7 does not read are whatever the workspace held"""
    x = torch.from_numpy(_images("132x68")).cuda()
    net, _ = _build(api, "param", "132x68")
    assert _halves(net)[7] == 1
    ws = net.workspace(N_IMG)
    res = []
    for fill in (None, 77):
        if fill is None:
            ws.fill_(0xFF)
        else:
            ws.copy_(torch.from_numpy(np.random.default_rng(fill).integers(0, 256, ws.numel(), dtype=np.uint8)))
        out, latent = net.forward(x)
        torch.cuda.synchronize()
        res.append((out.clone(), latent.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ref = _oracle("param", "132x68")
    _same(res[0][0], [r[7] for r in ref], "reconstruction")
    _same(res[1][1], [r[3] for r in ref], "latent")


@pytest.mark.parametrize("name", ["random_dead48", "dense"])
def test_five_or_eight_columns_keep_both_halves(api, name):
    net, _ = _build(api, name, "132x68")
    assert _halves(net) == [2] * 8
    _check_forward(net, name, "132x68", name)


def test_param_tapped_layer_6_keeps_both_halves(api):
    """a tapped layer computes every column and hands its output over in NHWC"""
    net, _ = _build(api, "param", "132x68")
    assert _halves(net, 4, 7, 6) == [2] * 8 and _halves(net, 4, 7, -1) == [2] * 7 + [1]
    ref = _oracle("param", "132x68")
    src = torch.from_numpy(np.stack([r[3] for r in ref])).cuda()
    out, tap = net.run_layers(4, 7, src, tap_layer=6)
    torch.cuda.synchronize()
    _same(tap, [r[6] for r in ref], "tap 6")
    _same(out, [r[7] for r in ref], "layer 7 behind tap 6")
    out, _ = net.run_layers(4, 7, src)
    torch.cuda.synchronize()
    _same(out, [r[7] for r in ref], "layers 4 .. 7, one half")


def test_param_layer_7_alone_keeps_both_halves(api):
    """the first layer of a call reads the caller's NHWC tensor: nothing is known of who wrote it"""
    net, _ = _build(api, "param", "132x68")
    assert _halves(net, 7, 7, -1) == [2] * 8
    ref = _oracle("param", "132x68")
    out, _ = net.run_layers(7, 7, torch.from_numpy(np.stack([r[6] for r in ref])).cuda())
    torch.cuda.synchronize()
    _same(out, [r[7] for r in ref], "layer 7 alone")


def test_param_force_generic_keeps_both_halves(api):
    net, _ = _build(api, "param", "132x68", force_generic=1)
    assert _halves(net) == [2] * 8
    _check_forward(net, "param", "132x68", "force_generic")


def test_param_in_a_captured_graph(api):
    size = "132x68"
    net, _ = _build(api, "param", size)
    descs = _descs(size)
    xin = torch.from_numpy(_images(size)).cuda()
    out = torch.empty((N_IMG,) + descs[7].out_shape, dtype=torch.uint8, device="cuda")
    latent = torch.empty((N_IMG,) + descs[3].out_shape, dtype=torch.uint8, device="cuda")
    graph = net.capture(xin, out, latent)
    ref = _oracle("param", size)
    for _ in range(2):
        out.zero_()
        latent.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(latent, [r[3] for r in ref], "latent")
        _same(out, [r[7] for r in ref], "reconstruction")
