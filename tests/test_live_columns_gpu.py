"""Live columns: a 128 -> 128 layer on the wide persistent kernels computes only the accumulator columns whose channels the next layer
reads (csrc/sicn_live.h, csrc/k_mfma16x_live.hip).  The net permutes the channels between the two layers in its weight images, so every
byte that leaves the chain must be what it was: held here to the oracle (c_oracle.run_net, direct form) and to the same layers run one
by one through the per-layer entry points, which always compute every channel.
wave_tile = 128, persistent_grid = 8 and 3 images of 132 x 68 throughout (as tests/test_wide_regfile_gpu.py): layer 1's output is
33 x 17 = 2 x 2 tiles of 16 x 32 positions, 12 tiles on 8 workgroups, so both the first-tile path and the hand-over path are taken; layer 6
(36 x 20 inputs) has 2 x 2 tiles too, layers 2 and 5 one tile per image."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from oracle import c_oracle, sicn_ref
from simple_image_compression_network_amd.config import eight_layer_descs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPTIONS = {"wave_tile": 128, "persistent_grid": 8}
N_IMG, W, H = 3, 132, 68
WIDE = (1, 2, 5, 6)          # the 128 -> 128 layers; layer l + 1 is the consumer whose zero input channels let layer l skip columns
GOLDEN = Path(__file__).resolve().parent / "golden" / "param_weights.npz"


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from simple_image_compression_network_amd import api as _api
    return _api


DESCS = eight_layer_descs(W, H)


def _images(seed):
    return np.random.default_rng(seed).integers(0, 256, (N_IMG, H, W, 3), dtype=np.uint8)


def _random_net(seed, n_dead):
    """[(W[o][ky][kx][c] int8 in -8 .. 7, bias int8)] per layer; n_dead random input channels of every 128-channel input are zero; the
    bias differs per channel, so that a bias that did not follow its channel's permutation is readable"""
    rng = np.random.default_rng(seed)
    net = []
    for d in DESCS:
        w = rng.integers(-8, 8, (d.OFM_CH, 5, 5, d.IFM_CH)).astype(np.int8)
        if d.IFM_CH == 128 and n_dead:
            w[:, :, :, rng.permutation(128)[:n_dead]] = 0
        b = rng.integers(-128, 128, d.OFM_CH).astype(np.int8)
        net.append((w, b))
    return net


def _param_net():
    return [(w, b) for w, b, _ in sicn_ref.load_param_fixture(GOLDEN)]


def _words(net):
    return [sicn_ref.pack_finn_tiles(w, d.SIMD, d.PE) for d, (w, _) in zip(DESCS, net)]


def _build(api, net, gdn=None):
    words = _words(net)
    params = [(api.FixedPointWeights(d.SIMD, 4, d.PE, d.W_TILES, wd), b) for d, wd, (_, b) in zip(DESCS, words, net)]
    return api.EightLayersNet(W, H, params=params, options=OPTIONS, gdn=gdn), params


def _columns(net, first=0, last=7, tap=3):
    from simple_image_compression_network_amd import _lib
    cols, live = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().sicn_debug_net_columns(net._h, first, last, tap, N_IMG, cols, live), "sicn_debug_net_columns")
    return list(cols), list(live)


_ORACLE = {}


def _oracle(key, net, x):
    """every layer's output of every image, computed once per weight set"""
    if key not in _ORACLE:
        words = _words(net)
        _ORACLE[key] = [c_oracle.run_net(DESCS, words, [b for _, b in net], x[i], form="direct", threads=16) for i in range(N_IMG)]
    return _ORACLE[key]


def _same(got, want, what):
    got = got.cpu().numpy()
    for i in range(N_IMG):
        if not np.array_equal(got[i], want[i]):
            bad = np.argwhere(got[i] != want[i])
            y, xx, c = (int(v) for v in bad[0])
            raise AssertionError(f"{what}, image {i}: {len(bad)} wrong bytes in channels {sorted({int(v) for v in bad[:, 2]})[:16]}; "
                                 f"first: got {got[i][y, xx, c]} want {want[i][y, xx, c]} at ({y}, {xx}, {c})")


def _layer_by_layer(api, params, x):
    """the same weights through sicn_conv2d_opt / sicn_deconv522_opt, one layer at a time: every channel computed, nothing permuted"""
    t = torch.from_numpy(x).cuda()
    outs = []
    for d, (w, b) in zip(DESCS, params):
        t = (api.deconv522 if d.transposed else api.conv2d)(d, w, b, t, None, N_IMG, options=OPTIONS)
        outs.append(t)
    torch.cuda.synchronize()
    return outs


CASES = {
    # name: (weights, columns expected of layers 1, 2, 5, 6)
    "param": (_param_net, (5, 5, 5, 3)),
    "random_dead48": (lambda: _random_net(48, 48), (5, 5, 5, 5)),
    "random_dead47": (lambda: _random_net(47, 47), (8, 8, 8, 8)),       # 81 live = 6 columns: the next width that is built
    "random_dead112": (lambda: _random_net(112, 112), (3, 3, 3, 3)),    # 1 live column, rounded up to 3
    "random_dead80": (lambda: _random_net(80, 80), (3, 3, 3, 3)),       # 48 live: every position that 3 columns compute is read
    "dense": (lambda: _random_net(5, 0), (8, 8, 8, 8)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_latent_and_reconstruction_are_the_oracles(api, case):
    make, want_cols = CASES[case]
    weights = make()
    x = _images(1)
    net, params = _build(api, weights)
    cols, _ = _columns(net)
    assert tuple(cols[l] for l in WIDE) == want_cols and all(cols[l] == 8 for l in (0, 3, 4, 7)), cols
    out, latent = net.forward(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    ref = _oracle(case, weights, x)
    _same(latent, [r[3] for r in ref], f"{case}: latent")
    _same(out, [r[7] for r in ref], f"{case}: reconstruction")
    single = _layer_by_layer(api, params, x)
    assert torch.equal(latent, single[3]) and torch.equal(out, single[7]), f"{case}: the net differs from its layers run one by one"


def test_param_plan(api):
    net, _ = _build(api, _param_net())
    cols, live = _columns(net)
    assert live == [80, 80, 80, 192, 80, 80, 48, 3] and cols == [8, 5, 5, 8, 8, 5, 3, 8], (cols, live)
    # a tapped layer keeps every column, and with it the standard images on both sides of the tap
    cols, live = _columns(net, 0, 7, 1)
    assert cols[1] == 8 and live[1] == 128 and cols[2] == 5, (cols, live)
    # the last layer of a call leaves the chain
    cols, _ = _columns(net, 4, 6, -1)
    assert cols == [8, 8, 8, 8, 8, 5, 8, 8], cols


def test_param_workspace_content_does_not_matter(api):
    """the bytes of the columns nobody computed are whatever the workspace held: they meet zero weights"""
    x = torch.from_numpy(_images(1)).cuda()
    net, _ = _build(api, _param_net())
    res = []
    for fill in (0x00, 0xA5):
        net.workspace(N_IMG).fill_(fill)
        out, latent = net.forward(x)
        torch.cuda.synchronize()
        res.append((out.clone(), latent.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ref = _oracle("param", _param_net(), _images(1))
    _same(res[1][0], [r[7] for r in ref], "reconstruction")


def test_param_in_a_captured_graph(api):
    x = _images(1)
    net, _ = _build(api, _param_net())
    xin = torch.from_numpy(x).cuda()
    out = torch.empty((N_IMG,) + DESCS[7].out_shape, dtype=torch.uint8, device="cuda")
    latent = torch.empty((N_IMG,) + DESCS[3].out_shape, dtype=torch.uint8, device="cuda")
    graph = net.capture(xin, out, latent)
    ref = _oracle("param", _param_net(), x)
    for _ in range(2):
        out.zero_()
        latent.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(latent, [r[3] for r in ref], "latent")
        _same(out, [r[7] for r in ref], "reconstruction")


@pytest.mark.parametrize("tap", WIDE)
def test_param_tap_is_the_layers_output(api, tap):
    x = _images(1)
    net, _ = _build(api, _param_net())
    ref = _oracle("param", _param_net(), x)
    first, last = (0, 3) if tap < 4 else (4, 7)
    src = torch.from_numpy(x).cuda() if first == 0 else torch.from_numpy(np.stack([r[3] for r in ref])).cuda()
    out, t = net.run_layers(first, last, src, tap_layer=tap)
    torch.cuda.synchronize()
    _same(t, [r[tap] for r in ref], f"tap {tap}")
    _same(out, [r[last] for r in ref], f"layer {last} behind tap {tap}")


def test_param_analysis_and_synthesis(api):
    x = _images(1)
    net, _ = _build(api, _param_net())
    ref = _oracle("param", _param_net(), x)
    latent = net.analysis(torch.from_numpy(x).cuda())
    out = net.synthesis(latent)
    torch.cuda.synchronize()
    _same(latent, [r[3] for r in ref], "analysis")
    _same(out, [r[7] for r in ref], "synthesis")


def test_gdn_on_layer_1_keeps_every_column(api):
    """the activation mixes channels: layer 1 computes all of them, and the bytes are those of the layers run one by one with the
    same activation (the per-layer entry points never skip anything)"""
    rng = np.random.default_rng(9)
    beta = rng.integers(1, 65536, 128).astype(np.uint32)
    gamma = rng.integers(0, 128, (128, 128)).astype(np.uint8)
    g = api.GDN(beta, gamma, False, 12)
    x = _images(3)
    net, params = _build(api, _param_net(), gdn=[None, g] + [None] * 6)
    cols, live = _columns(net)
    assert cols[1] == 8 and live[1] == 128 and cols[2] == 5, (cols, live)
    out, latent = net.forward(torch.from_numpy(x).cuda())
    t = torch.from_numpy(x).cuda()
    for l, (d, (w, b)) in enumerate(zip(DESCS, params)):
        t = (api.deconv522 if d.transposed else api.conv2d)(d, w, b, t, None, N_IMG, options=OPTIONS, gdn=g if l == 1 else None)
        if l == 3:
            lat = t
    torch.cuda.synchronize()
    assert torch.equal(latent, lat) and torch.equal(out, t)
